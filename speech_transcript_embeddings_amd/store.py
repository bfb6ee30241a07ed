r"""Flat parameter storage in HBM.

Every parameter of the model tree becomes a view into ONE fp32 master buffer;
trainable parameters that receive gradients come first, so their gradients,
Adam moments and the fused optimizer work on contiguous ranges:

  [ encoder params with grad | head params with grad | trainable-without-grad | frozen ]
    \_____ grad / exp_avg / exp_avg_sq cover this prefix ____/

The encoder / head split mirrors the reference's two AdamW param groups
(ref:training/trainer_unfreeze.py:1496-1511: names containing 'text_encoder' or
'audio_encoder' get lr/50).  Parameters the reference never gives a gradient
(text pooler, masked_spec_embed without SpecAugment: grad None -> AdamW skips them)
sit in the third segment.

A bf16 shadow with the same offsets holds the MFMA operands.  The fused optimizer
refreshes it for updated ranges; anything else that writes parameters (load_state_dict,
a torch optimizer) bumps the tensor version counter and the shadow is re-cast lazily.

Fused groups (q/k/v weights and biases, key/value of the cross-modal attentions) are
laid out adjacently so one GEMM serves them and one dW GEMM writes their gradients.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import ops

ALIGN = 8  # elements: 32 B for fp32, 16 B for the bf16 shadow


def _fuse_groups(names):
    """Return name -> tuple(group) for parameters that must be adjacent."""
    groups = {}
    sets = [("attention.self.query", "attention.self.key", "attention.self.value"),
            ("self_attn.linear_q", "self_attn.linear_k", "self_attn.linear_v"),
            ("attention.q_proj", "attention.k_proj", "attention.v_proj"),
            ("_attention.key", "_attention.value")]
    nameset = set(names)
    for n in names:
        for trio in sets:
            for leaf in ("weight", "bias"):
                head = trio[0] + "." + leaf
                if n.endswith(head):
                    prefix = n[: -len(head)]
                    grp = tuple(prefix + t + "." + leaf for t in trio)
                    if all(g in nameset for g in grp):
                        for g in grp:
                            groups[g] = grp
    return groups


@dataclass
class Slot:
    name: str
    offset: int
    numel: int
    shape: tuple
    segment: str

    @property
    def has_grad(self) -> bool:
        """The parameter receives gradients: it lies in the prefix the gradient buffer, the Adam
        moments and the fused optimizer cover."""
        return self.segment in ("enc", "head")


@dataclass(frozen=True)
class Form:
    """A derived operand form of a weight (or of an adjacent fused group), cached by ParamStore._form."""
    source: str             # "shadow" (bf16 W), "master" (fp32 W), or "wt": built from wt(), rebuilt whenever that is
    build: object           # (source matrix, previous value or None) -> value, written over the previous one
    prebuilt: bool = False  # refresh_transposes[_in] rebuild it right after an optimizer step


def _twice(wt, old):
    n, k = wt.shape
    dst = old if old is not None else torch.empty((n, 2 * k), device=wt.device, dtype=wt.dtype)
    ops.copy2d(dst[:, :k], wt)
    ops.copy2d(dst[:, k:], wt)
    return dst


def _mx8(src, old):
    return ops.mx8_quant(src, *(old or (None, None)))


# the public accessors of the same names document each form; a new operand form is one more row
FORMS = {"wt": Form("shadow", lambda w, old: ops.transpose16(w, old), prebuilt=True),
         "w2": Form("master", lambda p, old: ops.split_bf16(p, 2, 0, old), prebuilt=True),
         "wt2": Form("wt", _twice),
         "wq": Form("shadow", _mx8),
         "wtq": Form("wt", _mx8)}


class ParamStore:
    def __init__(self, model: torch.nn.Module, device, has_grad: set[str]):
        named = list(model.named_parameters())
        names = [n for n, _ in named]
        params = dict(named)
        groups = _fuse_groups(names)

        def seg_of(n, p):
            if not p.requires_grad:
                return "frozen"
            if n not in has_grad:
                return "nograd"
            return "enc" if ("text_encoder" in n or "audio_encoder" in n) else "head"

        order = {"enc": [], "head": [], "nograd": [], "frozen": []}
        seen = set()
        for n, p in named:
            if n in seen:
                continue
            grp = groups.get(n, (n,))
            segs = {seg_of(g, params[g]) for g in grp}
            if len(segs) != 1:
                grp = (n,)
            for g in grp:
                order[seg_of(g, params[g])].append(g)
                seen.add(g)
        self.slots: dict[str, Slot] = {}
        off = 0
        self.seg_range = {}
        for seg in ("enc", "head", "nograd", "frozen"):
            start = off
            for n in order[seg]:
                p = params[n]
                grp = groups.get(n)
                if grp is None or n == grp[0]:
                    off = (off + ALIGN - 1) // ALIGN * ALIGN
                self.slots[n] = Slot(n, off, p.numel(), tuple(p.shape), seg)
                off += p.numel()
            off = (off + ALIGN - 1) // ALIGN * ALIGN
            self.seg_range[seg] = (start, off)
        self.numel = off
        self.n_grad = self.seg_range["head"][1]
        self.device = torch.device(device)
        self.master = torch.zeros(self.numel, device=self.device, dtype=torch.float32)
        self.shadow = torch.zeros(self.numel, device=self.device, dtype=torch.bfloat16)
        self.grad = torch.zeros(self.n_grad, device=self.device, dtype=torch.float32)
        # re-seat every parameter as a view of the flat buffer (module trees may be built on
        # the meta device: values are initialised afterwards, directly in HBM)
        for n, s in self.slots.items():
            p = params[n]
            view = self.master[s.offset:s.offset + s.numel].view(s.shape)
            if p.device.type != "meta":
                with torch.no_grad():
                    view.copy_(p.detach().to(self.device, torch.float32))
            owner, leaf = (model.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1]) if "." in n \
                else (model, n)
            newp = torch.nn.Parameter(view, requires_grad=p.requires_grad)
            owner._parameters[leaf] = newp
            params[n] = newp
        self.params = params
        self._versions = {}
        self._cache = {form: {} for form in FORMS}   # form -> (name, count) -> (value, token, builds), see _form()
        self._members = {}     # (name, count) -> names of the parameters in that fused group
        self.opt_epoch = 0     # fused optimizer steps so far (each refreshes the shadow of every trained weight)
        self._prebuilt = None  # (event, stream, streams that waited): forms rebuilt by refresh_transposes
        self.sync_shadow(force=True)

    # ------------------------------------------------------------------ views
    def p(self, name):
        s = self.slots[name]
        return self.master[s.offset:s.offset + s.numel].view(s.shape)

    def w(self, name, rows=None):
        """bf16 shadow as a 2-D [out, in] matrix (conv weights [out,in,1] flattened)."""
        s = self.slots[name]
        v = self.shadow[s.offset:s.offset + s.numel]
        return v.view(s.shape[0], -1) if rows is None else v.view(rows, -1)

    def g(self, name):
        s = self.slots[name]
        if not s.has_grad:
            return None
        return self.grad[s.offset:s.offset + s.numel].view(s.shape)

    def fused(self, first: str, count: int, which: str):
        """Adjacent group starting at `first` as one tensor: which in {'w','p','g'}."""
        s = self.slots[first]
        n = s.numel * count
        if which == "w":
            return self.shadow[s.offset:s.offset + n].view(s.shape[0] * count, -1)
        if which == "p":
            base = self.master[s.offset:s.offset + n]
            return base.view(s.shape[0] * count, *s.shape[1:]) if len(s.shape) > 1 else base
        if not s.has_grad:
            return None
        base = self.grad[s.offset:s.offset + n]
        return base.view(s.shape[0] * count, *s.shape[1:]) if len(s.shape) > 1 else base

    # ------------------------------------------------- derived operand forms
    def _token(self, name, count):
        """What a form built from the shadow or the master was built against: the _version of every
        parameter of the group (it moves on a write outside the optimizer) and, for a weight that
        receives gradients, opt_epoch (the fused optimizer rewrites the shadow without it)."""
        names = self._members.get((name, count))
        if names is None:
            s = self.slots[name]
            names = self._members[name, count] = (name,) if count == 1 else tuple(
                n for n, t in self.slots.items() if s.offset <= t.offset < s.offset + s.numel * count)
        return tuple(self.params[n]._version for n in names), self.opt_epoch if self.slots[name].has_grad else None

    def _form(self, form, name, count):
        """The cache entry (value, token, builds) of one FORMS row for the weight `name` (count > 1:
        the adjacent fused group starting there), rebuilt first if it is stale.  An entry is valid
        while its token is the current one: _token() for a form built from the shadow or the
        master, the number of wt() builds for a form built from wt().  A rebuild writes into the
        entry's buffers.  refresh_transposes may still be writing a prebuilt form's buffer on its
        stream, so before that buffer is returned or overwritten the current stream waits for it."""
        f = FORMS[form]
        if f.source == "wt":
            src, _, token = self._form("wt", name, count)
        else:
            token = self._token(name, count)
        ent = self._cache[form].get((name, count))
        if ent is not None:
            if f.prebuilt:
                self._wait_prebuilt()
            if ent[1] == token:
                return ent
        if f.source != "wt":
            src = self.fused(name, count, "w" if f.source == "shadow" else "p").flatten(1)   # conv weights [out,in,1]
        old, builds = (ent[0], ent[2]) if ent is not None else (None, 0)
        ent = self._cache[form][name, count] = (f.build(src, old), token, builds + 1)
        return ent

    def _wait_prebuilt(self):
        if self._prebuilt is None:
            return
        ev, stream, waited = self._prebuilt
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream != stream.cuda_stream and cur.cuda_stream not in waited:
            cur.wait_event(ev)
            waited.add(cur.cuda_stream)

    def cached(self, form: str) -> int:
        """How many (name, count) entries of a form ('wt', 'w2', 'wt2', 'wq', 'wtq') are cached."""
        return len(self._cache[form])

    def wt(self, name: str, count: int = 1):
        """Wᵀ as a contiguous bf16 [in, out] matrix (the KC operand of dX = dY·W; `count` > 1:
        the adjacent fused group starting at `name`, e.g. Q|K|V -> [in, 3·out]).  Built from the
        bf16 shadow by the transpose kernel and cached; rebuilt when the shadow changed: after
        a fused optimizer step for weights that receive gradients, or when a parameter was
        written outside the optimizer (its _version moved)."""
        return self._form("wt", name, count)[0]

    def w2(self, name: str, count: int = 1):
        """W as [W_bf16 | W_bf16] [out, 2·in] (the B operand of ops.linear_x2: the text encoder's
        precise forward, activations split hi | lo against the bf16 weight twice).  Built from the
        fp32 master; cached with wt()'s invalidation rules; refresh_transposes rebuilds the trained
        ones after an optimizer step."""
        return self._form("w2", name, count)[0]

    def wt2(self, name: str, count: int = 1):
        """[Wᵀ | Wᵀ] bf16 [in, 2·out]: the KC operand of a dX GEMM over a [dy_hi | dy_lo] split image
        (dy to ~fp32 against the bf16 weight).  Rebuilt from wt() whenever that is."""
        return self._form("wt2", name, count)[0]

    def wq(self, name: str, count: int = 1):
        """W as MX-fp8 (e4m3 [out, in] + E8M0 scales [out, in/32]), the B operand of the MX-fp8
        forward GEMMs (model fp8_gemm=True, BASELINE config 5).  Quantised from the bf16 shadow
        and cached with wt()'s invalidation rules (optimizer step for trained weights, _version
        for writes outside it)."""
        return self._form("wq", name, count)[0]

    def wtq(self, name: str, count: int = 1):
        """Wᵀ as MX-fp8 (e4m3 [in, out] + E8M0 scales [in, out/32], blocks of 32 along `out`): the B
        operand of the opt-in MX-fp8 input-gradient GEMMs dX = dY·W (engine.fp8_bwd).  Quantised
        from wt() and rebuilt whenever wt() rebuilds its transpose."""
        return self._form("wtq", name, count)[0]

    def _stale_prebuilt(self, inside=lambda slot: True):
        """(form, name, count) of every cached prebuilt form of a weight the fused optimizer has
        updated since the form was built."""
        return [(form, *key) for form, f in FORMS.items() if f.prebuilt
                for key, ent in self._cache[form].items()
                if self.slots[key[0]].has_grad and ent[1][1] != self.opt_epoch and inside(self.slots[key[0]])]

    def refresh_transposes(self, stream):
        """Rebuild on `stream` every cached Wᵀ of a weight the fused optimizer just updated
        (26 transposes per c2 step), right after the optimizer step, so they overlap the next
        forward instead of sitting on the backward's critical path.  A stream that later takes
        one of them from wt() first waits for this work (one event)."""
        if stream is None or self.device.type != "cuda":
            return
        stale = self._stale_prebuilt()
        if not stale:
            return
        stream.wait_stream(torch.cuda.current_stream(self.device))   # the optimizer's shadow writes
        self._prebuilt = None                 # the rebuilds below must not wait on the previous event
        with torch.cuda.stream(stream):
            for key in stale:
                self._form(*key)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._prebuilt = (ev, stream, set())

    def refresh_transposes_in(self, runs):
        """refresh_transposes for the weights inside the flat-buffer runs [(a, b), ...], on the
        current stream (TrainStep(overlap_optimizer=True): the optimizer stream, right after the
        AdamW of that block, so the block's event covers its transposes too and no consumer waits
        on a global rebuild event)."""
        if self.device.type != "cuda":
            return
        self._prebuilt = None
        for key in self._stale_prebuilt(lambda slot: any(a <= slot.offset < b for a, b in runs)):
            self._form(*key)

    def trainable_layer(self, name: str) -> bool:
        return self.slots[name].has_grad

    # ----------------------------------------------------------------- shadow
    def sync_shadow(self, force=False):
        """Re-cast the bf16 shadow of any parameter modified outside the fused optimizer."""
        if self.device.type != "cuda":
            return  # meta / cpu stores only serve module-tree inspection; no kernel can run there
        for n, s in self.slots.items():
            v = self.params[n]._version
            if force or self._versions.get(n) != v:
                src = self.master[s.offset:s.offset + s.numel]
                dst = self.shadow[s.offset:s.offset + s.numel]
                ops.cast_bf16(src, dst)
                self._versions[n] = self.params[n]._version

    def weights_token(self):
        """A value that changes whenever a weight does: the sum of the parameters' _version counters
        (they only grow; a write outside the optimizer moves one) and opt_epoch (the fused optimizer
        writes the flat buffers without them).  What an AudioStateStore records to know it is stale."""
        return sum(p._version for p in self.params.values()), self.opt_epoch

    def mark_synced(self):
        """The fused optimizer refreshed the shadow of every trained parameter."""
        for n in self.slots:
            self._versions[n] = self.params[n]._version
        self.opt_epoch += 1

    # ------------------------------------------------------------------ grads
    def attach_grads(self):
        """Point .grad of every gradient-receiving parameter at its slice of the flat buffer.
        Returns True if the buffer must be zeroed first (grads were reset to None)."""
        names = [n for n, s in self.slots.items() if s.has_grad]
        reset = any(self.params[n].grad is None for n in names)
        if reset:
            self.grad.zero_()
            for n in names:
                self.params[n].grad = self.g(n)
        return reset
