"""Per-kernel parity of the tail of the training step, each entry point alone against a float64
torch restatement of its contract in include/ste.h, at the smallest shapes that enter every branch:
the pooling / cross-modal / alignment heads (csrc/heads.hip, csrc/align.hip), normalise ->
similarity -> InfoNCE, the XLM-R embedding gather / scatter, the row-sparse word-table exchange and
the fused clip + AdamW (csrc/embed_optim.hip).

Tolerances are those of tests/test_w2v2_kernels_gpu.py, imported from there:
* fp32 elementwise outputs and short sums: relative L2 < 1e-6 against fp64 (F32_TOL);
* bf16 outputs: |out - ref| <= 2^-8·|ref| + 1e-5·max|ref| (_assert_bf16_close);
* pure moves and index outputs: torch.equal;
* reductions and chains of several fp32 roundings: max(1e-6, 10·e32) (_margin), e32 the error of
  plain fp32 torch on the same inputs against the same fp64 reference (never from the kernel);
* AdamW also elementwise, max|out - ref| / max|ref|, under the same rule;
* a sum whose true value is 0 (the pooling scorer's db2 = Σ_l dscore_l) has no relative error: its
  error, and fp32 torch's, are taken relative to Σ|terms|, which is what an fp32 sum's rounding
  scales with.
Every scalar a kernel receives as float reaches the reference as float(np.float32(x)).

Which shape reaches which branch (the arithmetic):
* adamw: grid_for(n) caps the grid at 8192 blocks, stride = 8192·256·4 = 8,388,608 elements, and the
  bulk loop runs while i + stride + 3 < n.  n = 20,971,527 = 2.5·stride + 7: every thread's first
  index i0 < stride gives i0 + stride + 3 < n (one bulk iteration, two groups), then i0 + 2·stride
  < n for i0 < stride/2 + 7 (the one-group loop for half the grid), and the thread at
  i0 = stride/2 + 4 is left the last 3 elements (the scalar tail).  Launches of <= 4,000,000
  elements have stride >= n - 3 and never enter the bulk loop (test_kernels_gpu.py's
  split-invariance case compares the two bit for bit).
* sumsq: 2048 blocks x 256 threads x 4 = 2,097,152 elements per grid stride; the fp32 -> fp64 flush
  needs 64 strides = 134,217,728 elements.  n = 4,194,309: two strides and a 5-element tail, no
  flush; n = 138,412,037 = 66 strides + 5: every thread flushes once, after its 64th iteration, and
  runs two more (the first two threads a third: a group and a 1-element tail).
* text_embed_bwd: ids staged in LDS for rows <= 16384 (B·L = 16384: 64 KiB of dynamic LDS, the
  boundary), read from global memory at 16400; D = 1024: four quads per lane, D = 260: the 65th
  quad on lane 0's second pass; L = 300 > 256: the forward's thread loop.
* rows_extract / _accumulate: D = 1028 > 256·4 takes a second pass of the column loop.
* l2norm / pair_sim_bwd: cols 768 and 1000 > 256 threads (3 / 4 passes, ragged last);
  a zero row and a row of norm 1e-20 take the eps clamp of both kernels.
* similarity: P = 770 leaves k + kk < P false in the last step for kk >= 2; P = 1: for kk >= 1;
  (1, 1, 1) and (16, 32, 768): one partial tile and whole tiles.
* pair_loss: B = 300 > 256 threads: 44 threads take two pairs; the backward runs 2 blocks.
* inbatch_ce / pair_metrics: NB = 300 columns > 256 threads.
* xattn: dh = P/nh = 24: 6 quads, RG = 256/6 = 42 row groups, threads 252..255 idle; dh = 8: RG = 128
  row groups > S = 1, 5 (most groups get no row); dh = 256: 64 quads, RG = 4; S = 257 > 256: the
  score / softmax thread loops.
* attn_pool_bwd: Hh = 1024: 256 column quads, one row group; Hh = 4: one quad, 256 row groups over
  16-row chunks (240 idle); H = 260: the 65th quad; L = 70: a ragged last 16-row chunk.
* align_attn: L = 9: a block with one query of 8; T = 300 > 256: the key thread loop; T = 17: a
  ragged 16-key block in the kv kernel; L = 70: two 64-query chunks there; d = 192: 16·192 = 12·256,
  every accumulator slot of the kv kernel used.
* the limits: align_attn T = 2048: 8·2048·4 B dynamic + 8 KiB static = 72 KiB of LDS per block;
  mean_pool L = 16384: 64 KiB + 32 B; attn_pool_fwd L = 8192: 32 KiB + 8 KiB; each is first checked
  against the per-block limit the runtime reports (160 KiB on an MI355X).

Measured on an MI355X, kernel error / e32 (bound = max(1e-6, 10·e32)), the case closest to its
bound per output (every case prints its pair):
  adamw n=20,971,527 clipped     p 3.8e-8 / 3.8e-8 (max 9.7e-8 / 9.7e-8)   m 2.9e-8 / 3.8e-8   v 2.7e-8 / 3.8e-8
  adamw n=20,971,527 unclipped   p 2.5e-8 / 2.5e-8 (max 4.4e-8 / 4.4e-8)   m 3.2e-8 / 3.7e-8   v 2.7e-8 / 3.8e-8
  adamw n in 1..1027, worst      p 9.1e-8 / 9.1e-8 (n=1)   m 6.3e-8 / 7.6e-8 (n=4)   v 3.2e-8 / 3.2e-8 (n=4)
  sumsq n=138,412,037            1.3e-10 relative, ordered partials and atomics (bound 1e-7); 0.04 s, the
                                 longest case after adamw n=20,971,527 clipped (1.0 s); the file takes 4 s
  text_embed_bwd (50,328,8)      dword 2.8e-7 / 2.8e-7   dpos 1.3e-7 / 1.2e-7   dtype0 1.3e-7 / 9.8e-8
  similarity (17,33,770)         5.5e-7 / 2.7e-7
  pair_loss                      loss 9.6e-8 / 9.6e-8   ds_pos 6.6e-8 / 7.2e-8   ds_neg 7.0e-8 / 8.2e-8   dalign 2.6e-8 / 1.2e-7
  inbatch_ce                     loss 4.7e-8 / 4.0e-8   dS 3.5e-7 / 8.1e-8
  pair_metrics                   Σ sigmoid 1.6e-9 / 3.4e-9 and 1.8e-9 / 9.8e-10
  xattn P=1024 S=5               probs, out, dv 2.8e-7 / 2.2e-7   dq 7.5e-7 / 3.5e-7   dk 7.6e-7 / 3.4e-7
  xattn P=32 S=257 nq=2          colsum 4.1e-7 / 8.2e-8
  attn_pool (2,70,260,4)         weights 9.2e-8 / 8.1e-8   pooled 9.2e-8 / 1.4e-7   dh 9.5e-8 / 8.5e-8   db1 2.1e-6 / 9.5e-7
                                 dt + dt_lo 2.1e-6 / 2.9e-7 (bound 2.9e-6 + 2^-18)
  attn_pool (2,17,8,1024)        dw2 5.0e-7 / 6.3e-7   dt (fp32) 4.9e-7 / 6.4e-7   db2 / Σ|dscore| 1.4e-7 / 1.4e-8
  attn_pool_fwd L=8192           weights 6.1e-8 / 1.1e-7   pooled 1.8e-7 / 2.1e-6
  mean_pool L=16384              bf16 1.3e-7 / 4.7e-8   fp32 2.2e-7 / 8.3e-8 (2.1e-6 / 8.3e-8 with the single running
                                 sum the kernel had before this file: the two-level sum in mean_pool_fwd_kernel)
  align_attn (1,70,17,768)       probs 3.0e-7 / 1.4e-7   dkv 3.2e-7 / 2.1e-7;   T=2048: 1.5e-7 / 1.1e-7 and 1.6e-7 / 1.3e-7
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kref import drop_scale
from test_w2v2_kernels_gpu import BF16, DEV, ERR_SHAPE, F32, F32_TOL, F64, _assert_bf16_close, _margin, _p, _rel, _s

pytestmark = pytest.mark.gpu
ERR_ARG = 1001         # STE_ERR_ARG (include/ste.h)
I32, I64 = torch.int32, torch.int64
ACT_NONE, ACT_TANH_BWD_OUT, ACT_RELU_BWD = 0, 13, 14


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops
    return ops


def f32(x):
    """A scalar as the kernel receives it (a float argument)."""
    return float(np.float32(x))


def _lds_limit():
    """The per-block shared-memory limit as the runtime reports it."""
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).shared_memory_per_block)


def _grads(fn, inputs, dt, douts):
    """Outputs (tuple) and input gradients of fn evaluated in dtype dt on the CPU; douts: one
    upstream gradient per output (None: not differentiated)."""
    xs = [None if x is None else x.detach().cpu().to(dt).requires_grad_() for x in inputs]
    outs = fn(*xs)
    tot = sum((o * d.detach().cpu().to(dt)).sum() for o, d in zip(outs, douts) if d is not None)
    gs = torch.autograd.grad(tot, [x for x in xs if x is not None], allow_unused=True)
    it = iter(gs)
    return [o.detach() for o in outs], [None if x is None else next(it) for x in xs]


# ------------------------------------------------------------------ optimizer
N_BULK = 20_971_527                                  # 2.5 x 8,388,608 + 7 (module docstring)
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, step=5)


def _adamw_ref(p, g, m, v, dt, *, lr, beta1, beta2, eps, wd, step, sumsq=None, max_norm=1.0):
    """clip_grad_norm_ + torch.optim.AdamW.step (decoupled decay) in dtype dt."""
    lr, b1, b2, eps, wd, max_norm = (f32(x) for x in (lr, beta1, beta2, eps, wd, max_norm))
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    coef = 1.0 if sumsq is None else min(1.0, max_norm / (math.sqrt(sumsq) + f32(1e-6)))
    g = g * coef
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    den = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p * (1 - lr * wd) - (lr / (1 - b1 ** step)) * (m / den), m, v


def _dev_err(out, ref):
    """(relative L2, max|out - ref| / max|ref|) in fp64 on the device."""
    d = out.double() - ref
    return float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300))


def _adamw_case(ops, n, clip, seed):
    torch.manual_seed(seed)
    p = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV) * 0.01
    m = torch.randn(n, device=DEV) * 1e-3
    v = torch.rand(n, device=DEV) * 1e-5
    kw = dict(ADAM)
    ss = acc = pb = None
    if clip:
        acc = torch.zeros(1, device=DEV, dtype=F64)
        ops.sumsq(g, acc, torch.empty(ops.SUMSQ_PARTS, device=DEV, dtype=F64))
        ss = float((g.double() ** 2).sum())
        kw["max_norm"] = 0.5 * math.sqrt(ss)                      # below the norm: the clip is active
        pb = torch.full((n,), 7.0, device=DEV, dtype=BF16)
    else:
        kw.update(wd=0.0, step=1)
    ref = _adamw_ref(p, g, m, v, F64, sumsq=ss, **kw)
    t32 = _adamw_ref(p, g, m, v, F32, sumsq=ss, **kw)
    ops.adamw(p, g, m, v, pb, sumsq_acc=acc, **kw)
    for name, out, r, t in zip("pmv", (p, m, v), ref, t32):
        (l2, mx), (l2_32, mx_32) = _dev_err(out, r), _dev_err(t, r)
        _margin(l2, l2_32, f"adamw {name} n={n} clip={clip} (relative L2)")
        _margin(mx, mx_32, f"adamw {name} n={n} clip={clip} (max error / max|ref|)")
    if clip:
        assert torch.equal(pb, p.bfloat16())


@pytest.mark.parametrize("clip", [True, False])
def test_adamw_bulk(ops, clip):
    """p, m, v against fp64 at n = 2.5 grid strides + 7: the bulk two-group loop with its
    non-temporal accesses, the one-group loop and the scalar tail in one launch; once clipped (the
    coefficient from ste_sumsq's accumulator, with weight decay and the bf16 shadow) and once with
    sumsq = NULL, wd = 0, step = 1, p_bf16 = NULL."""
    _adamw_case(ops, N_BULK, clip, 11)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_adamw_small(ops, n):
    """Only a scalar tail (1, 3), one whole group (4), a group and a tail (5), many blocks (1027)."""
    _adamw_case(ops, n, True, n)
    _adamw_case(ops, n, False, n + 1)


def _sumsq(ops, g, with_part, pre=0.0):
    acc = torch.full((1,), pre, device=DEV, dtype=F64)
    ops.sumsq(g, acc, torch.empty(ops.SUMSQ_PARTS, device=DEV, dtype=F64) if with_part else None)
    return float(acc[0])


@pytest.mark.parametrize("with_part", [True, False])
@pytest.mark.parametrize("n", [1, 3, 5, 2048 * 1024 * 2 + 5])
def test_sumsq(ops, n, with_part):
    """Σ g² in fp64, ordered partials and fp64 atomics: the scalar tail alone (1, 3), a group and a
    tail (5; multiples of 2^-10, whose squares and sums are exact in fp32, so the result is exact)
    and two grid strides without a flush; the result is added to the accumulator."""
    torch.manual_seed(n)
    if n <= 5:
        g = torch.randint(-64, 65, (n,)).float().mul(2.0 ** -10).to(DEV)
        g[0] = 33 * 2.0 ** -10
    else:
        g = torch.randn(n, device=DEV) * 1e-3
    ref = float((g.double() ** 2).sum())
    got = _sumsq(ops, g, with_part)
    if n <= 5:
        assert got == ref
    assert abs(got - ref) / ref < 1e-7, (got, ref)
    assert abs(_sumsq(ops, g, with_part, pre=ref) - 2 * ref) / ref < 2e-7          # += into *acc


def test_sumsq_flush(ops):
    """n = 66 grid strides + 5 (554 MB): the smallest size at which a thread's fp32 partial is
    flushed into its fp64 sum (after 64 iterations) and goes on; randn·1e-3 plus a few 1e3 outliers
    (in the first stride, inside and after the flush window and in the scalar tail), against an
    fp64 reference summed in chunks."""
    n = 64 * 2048 * 1024 + 2 * 2048 * 1024 + 5
    torch.manual_seed(12)
    g = torch.randn(n, device=DEV).mul_(1e-3)
    g[torch.tensor([0, 2048 * 1024 * 31 + 77, 2048 * 1024 * 65 + 1234, n - 2], device=DEV)] = 1e3
    ref = 0.0
    for c in g.split(1 << 24):
        ref += float((c.double() ** 2).sum())
    for with_part in (True, False):
        got = _sumsq(ops, g, with_part)
        print(f"sumsq n={n} part={with_part}: relative error {abs(got - ref) / ref:.3e}")
        assert abs(got - ref) / ref < 1e-7, (got, ref)


def test_optim_error_returns(lib):
    """Host-side returns (no launch): step < 1 and a 4-byte-offset slice -> STE_ERR_ARG; n = 0 -> 0
    with nothing written."""
    n = 16
    p, g, m, v = (torch.full((n + 4,), float(i + 1), device=DEV) for i in range(4))
    pb = torch.full((n + 4,), 7.0, device=DEV, dtype=BF16)
    acc = torch.full((1,), 3.0, device=DEV, dtype=F64)
    hp = [f32(x) for x in (1e-3, 0.9, 0.999, 1e-8, 0.01)]
    adamw = lib.fn("ste_adamw")
    assert adamw(_p(p), _p(g), _p(m), _p(v), _p(pb), n, *hp, 0, None, 1.0, _s(lib)) == ERR_ARG
    assert adamw(_p(p[1:]), _p(g[1:]), _p(m), _p(v), _p(pb), n, *hp, 1, None, 1.0, _s(lib)) == ERR_ARG
    assert adamw(_p(p), _p(g), _p(m), _p(v), _p(pb[1:]), n, *hp, 1, None, 1.0, _s(lib)) == ERR_ARG   # 2-byte offset
    assert adamw(_p(p), _p(g), _p(m), _p(v), _p(pb), 0, *hp, 1, _p(acc), 1.0, _s(lib)) == 0
    assert lib.fn("ste_sumsq")(_p(g[1:]), n, _p(acc), None, _s(lib)) == ERR_ARG
    assert lib.fn("ste_sumsq")(_p(g), 0, _p(acc), None, _s(lib)) == 0
    torch.cuda.synchronize()
    for i, t in enumerate((p, g, m, v)):
        assert torch.equal(t, torch.full_like(t, float(i + 1)))
    assert torch.equal(pb, torch.full_like(pb, 7.0)) and float(acc[0]) == 3.0


# ------------------------------------------------------------------ embedding
PAD = 1


def _embed_ids(B, L, V, seed):
    """Leading pads (row 0), an all-pad row (row 1), padded tails (rows >= 2), ids repeated within
    and across rows (V is small; id 3 is planted twice in row 0 and once in row 2)."""
    ids = torch.randint(2, V, (B, L), generator=torch.Generator().manual_seed(seed))
    if L > 2:
        ids[0, :2] = PAD
        ids[0, 2] = ids[0, L - 1] = 3
    if B > 1:
        ids[1] = PAD
    if B > 2:
        ids[2:, L - L // 4:] = PAD
        ids[2, 0] = 3
    return ids


@pytest.mark.parametrize("B,L,D,V", [(1, 1, 4, 7), (2, 300, 8, 7), (3, 17, 1024, 7), (2, 33, 260, 7),
                                     (64, 256, 8, 50), (50, 328, 8, 50)])
def test_text_embed(ops, B, L, D, V):
    """Gather and position ids, then the ordered scatter: dword / dpos / dtype0 accumulate into a
    prefill, each may be NULL, two runs are bit-identical.  B·L = 16384 is the last size with the ids
    in LDS (64 KiB), 16400 reads them from global memory; see the module docstring for the rest."""
    torch.manual_seed(B * L + D)
    ids = _embed_ids(B, L, V, B * L)
    NP = L + PAD + 1
    word, pos, typ = torch.randn(V, D), torch.randn(NP, D), torch.randn(1, D)
    nz = (ids != PAD).long()
    pref = torch.cumsum(nz, 1) * nz + PAD
    out = torch.full((B * L, D), 7.0, device=DEV)
    pid = torch.full((B * L,), -7, dtype=I32, device=DEV)
    ids_d = ids.to(DEV)
    ops.text_embed_fwd(ids_d, PAD, word.to(DEV), pos.to(DEV), typ.to(DEV), out, pid)
    assert torch.equal(pid.cpu().view(B, L).long(), pref)
    ref = word.double()[ids] + pos.double()[pref] + typ.double()[0]
    assert _rel(out, ref.view(B * L, D)) < F32_TOL

    do = torch.randn(B * L, D)
    do_d = do.to(DEV)
    pre = dict(dword=torch.randn(V, D), dpos=torch.randn(NP, D), dtype0=torch.randn(1, D))

    def scatter(dt):
        keep = (ids.view(-1) != PAD).nonzero().view(-1)
        dw = pre["dword"].to(dt, copy=True).index_add_(0, ids.view(-1)[keep], do.to(dt)[keep])
        dp = pre["dpos"].to(dt, copy=True).index_add_(0, pref.view(-1)[keep], do.to(dt)[keep])
        return dict(dword=dw, dpos=dp, dtype0=pre["dtype0"].to(dt) + do.to(dt).sum(0, keepdim=True))

    def run(has=("dword", "dpos", "dtype0")):
        o = {n: (pre[n].to(DEV) if n in has else None) for n in pre}
        ops.text_embed_bwd(ids_d, pid, do_d, PAD, o["dword"], o["dpos"], o["dtype0"])
        return o

    ref, t32 = scatter(F64), scatter(F32)
    o1, o2 = run(), run()
    for n in pre:
        assert torch.equal(o1[n], o2[n]), n
        _margin(_rel(o1[n], ref[n]), _rel(t32[n], ref[n]), f"text_embed_bwd {n} B={B} L={L} D={D}")
    assert torch.equal(o1["dword"][PAD].cpu(), pre["dword"][PAD])        # padding_idx rows get nothing
    assert torch.equal(o1["dpos"][PAD].cpu(), pre["dpos"][PAD])
    for skip in pre:
        o = run(tuple(n for n in pre if n != skip))
        for n in pre:
            assert o[n] is None or torch.equal(o[n], o1[n]), (skip, n)


def test_text_embed_error_returns(lib):
    """L > 2048, D % 4 != 0 and (backward) D > 1024 are refused before any launch."""
    t = torch.zeros(4096, device=DEV)
    ids = torch.full((4096,), 2, dtype=I64, device=DEV)
    pid = torch.zeros(4096, dtype=I32, device=DEV)
    fwd, bwd = lib.fn("ste_text_embed_fwd"), lib.fn("ste_text_embed_bwd")
    assert fwd(_p(ids), 1, 2049, 4, PAD, _p(t), _p(t), _p(t), _p(t), _p(pid), _s(lib)) == ERR_SHAPE
    assert fwd(_p(ids), 1, 4, 6, PAD, _p(t), _p(t), _p(t), _p(t), _p(pid), _s(lib)) == ERR_SHAPE
    assert bwd(_p(ids), _p(pid), _p(t), 1, 2, 6, PAD, _p(t), _p(t), _p(t), None, 0, _s(lib)) == ERR_SHAPE
    assert bwd(_p(ids), _p(pid), _p(t), 1, 2, 1028, PAD, _p(t), _p(t), _p(t), None, 0, _s(lib)) == ERR_SHAPE
    assert bwd(_p(ids), _p(pid), _p(t), 0, 2, 8, PAD, _p(t), _p(t), _p(t), None, 0, _s(lib)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


@pytest.mark.parametrize("D", [4, 1028])
def test_rows_exchange(ops, D):
    """rows_extract: the unique non-pad ids claim exactly cap slots, their rows move out (grad row
    and flag back to 0); n = 0 and all-pad ids: count 0, every slot -1, rows zero, grad untouched.
    rows_accumulate: grad[id] += 0.25·row, -1 slots skipped.  D = 1028: a second column pass."""
    torch.manual_seed(D)
    V = 40
    grad0 = torch.randn(V, D, device=DEV)

    def extract(ids, cap):
        grad, flags = grad0.clone(), torch.zeros(V, dtype=I32, device=DEV)
        out_ids = torch.full((cap,), 99, dtype=I32, device=DEV)
        rows, count = torch.full((cap, D), 7.0, device=DEV), torch.full((1,), 99, dtype=I32, device=DEV)
        ops.rows_extract(ids, PAD, grad, flags, out_ids, rows, count)
        assert int(flags.abs().sum()) == 0
        return grad, out_ids, rows, int(count[0])

    uniq = [5, 7, 9, 30]
    ids = torch.tensor([5, 7, 5, PAD, 9, 7, 30, PAD, 5], dtype=I64, device=DEV)
    grad, out_ids, rows, count = extract(ids, len(uniq))          # cap exactly the unique count
    assert count == len(uniq) and sorted(out_ids.tolist()) == uniq
    assert torch.equal(rows, grad0[out_ids.long()])
    keep = torch.ones(V, dtype=torch.bool, device=DEV)
    keep[uniq] = False
    assert torch.equal(grad[keep], grad0[keep]) and float(grad[~keep].abs().max()) == 0.0

    scale = 0.25
    acc = grad0.clone()
    ops.rows_accumulate(acc, out_ids, rows, scale)
    refacc = grad0.double()
    refacc[out_ids.long()] += f32(scale) * rows.double()
    assert torch.equal(acc[keep], grad0[keep])
    assert _rel(acc[~keep], refacc[~keep]) < F32_TOL

    for none in (torch.empty(0, dtype=I64, device=DEV), torch.full((6,), PAD, dtype=I64, device=DEV)):
        grad, out_ids, rows, count = extract(none, 3)
        assert count == 0 and out_ids.tolist() == [-1, -1, -1]
        assert float(rows.abs().max()) == 0.0 and torch.equal(grad, grad0)
        ops.rows_accumulate(grad, out_ids, torch.ones_like(rows), scale)   # every slot empty
        assert torch.equal(grad, grad0)


# ------------------------------------------------------------------ loss chain
@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 768), (3, 1000)])
def test_l2norm(ops, rows, cols):
    """F.normalize(eps = 1e-12) rows and its backward, row by row: 3 and 4 column passes of the 256
    threads; row 1 all zero (y = 0, norm = 0, dx = dy·1e12, as F.normalize's fp64 backward gives) and
    row 2 of norm 1e-20 (clamped too: y = x·1e12); at 5 rows, row 3 of norm 1e-13."""
    torch.manual_seed(rows * 31 + cols)
    x = torch.randn(rows, cols) * (0.5 + torch.rand(rows, 1))
    if rows >= 3:
        x[1] = 0.0
        u = torch.randn(cols).double()
        x[2] = (u / u.norm() * 1e-20).float()
    if rows >= 5:                                     # below eps but not negligible: y = x·1e12 has norm 0.1, and only
        u = torch.randn(cols).double()                # the clamp branch of the backward gives dx = dy·1e12 there
        x[3] = (u / u.norm() * 1e-13).float()
    dy = torch.randn(rows, cols)
    xr = x.double().requires_grad_()
    yr = F.normalize(xr, p=2, dim=1, eps=1e-12)
    (dxr,) = torch.autograd.grad((yr * dy.double()).sum(), xr)
    y, norms = torch.full((rows, cols), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    ops.l2norm_fwd(x.to(DEV), y, norms)
    dx = torch.full((rows, cols), 7.0, device=DEV)
    ops.l2norm_bwd(y, norms, dy.to(DEV), dx)
    assert _rel(norms, x.double().norm(dim=1)) < F32_TOL
    for r in range(rows):
        if rows >= 3 and r == 1:
            assert float(y[r].abs().max()) == 0.0 and float(norms[r]) == 0.0
        else:
            assert _rel(y[r], yr[r]) < F32_TOL, r
        # a 1-vector's gradient is exactly 0: its error is taken relative to dy/|x|
        scale = dxr[r].norm() if cols > 1 else (dy[r].double() / x[r].double().norm()).norm()
        assert float((dx[r].double().cpu() - dxr[r]).norm() / scale) < F32_TOL, r
    if rows >= 3:
        assert float(norms[2]) < 1e-12
        nclamp = 4 if rows >= 5 else 3
        assert _rel(dx[1:nclamp], dy[1:nclamp].double() * 1e12) < F32_TOL


def test_l2norm_similarity_pair_error_returns(lib):
    """Nonpositive sizes are refused before any launch."""
    t = torch.zeros(64, device=DEV)
    s = _s(lib)
    for rows, cols in ((0, 4), (4, 0), (-1, 4)):
        assert lib.fn("ste_l2norm_fwd")(_p(t), rows, cols, _p(t), _p(t), s) == ERR_SHAPE
        assert lib.fn("ste_l2norm_bwd")(_p(t), _p(t), _p(t), rows, cols, _p(t), s) == ERR_SHAPE
    for B, NT, P in ((0, 2, 4), (2, 0, 4), (2, 2, 0)):
        assert lib.fn("ste_similarity")(_p(t), _p(t), B, NT, P, _p(t), s) == ERR_SHAPE
    assert lib.fn("ste_pair_loss_fwd")(_p(t), 8, 2, None, 0, 1, 0.1, 0.5, 0.0, _p(t), _p(t), _p(t), s) == ERR_SHAPE
    assert lib.fn("ste_pair_loss_bwd")(_p(t), _p(t), None, 0, 1, 0.1, 0.5, 0.0, None, _p(t), _p(t), None, s) == ERR_SHAPE
    assert lib.fn("ste_pair_sim_bwd")(_p(t), _p(t), _p(t), _p(t), _p(t), 0, 4, _p(t), _p(t), _p(t), s) == ERR_SHAPE
    assert lib.fn("ste_pair_sim_bwd")(_p(t), _p(t), _p(t), _p(t), _p(t), 2, 0, _p(t), _p(t), _p(t), s) == ERR_SHAPE
    # inbatch_ce: row0 + B > NB; pair_metrics: ldS < off_neg + NB; rowmat: P % 4 != 0
    assert lib.fn("ste_inbatch_ce")(_p(t), 8, 3, 4, 2, 0.1, 1.0, None, _p(t), _p(t), 8, s) == ERR_SHAPE
    assert lib.fn("ste_pair_metrics")(_p(t), 7, 4, 4, 0.1, None, 0, 1.0, _p(t), s) == ERR_SHAPE
    assert lib.fn("ste_rowmat_f32")(_p(t), 2, 1, _p(t), 2, 2, 6, _p(t), s) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


@pytest.mark.parametrize("B,NT,P", [(1, 1, 1), (17, 33, 770), (16, 32, 768)])
def test_similarity(ops, B, NT, P):
    """S = A·Tᵀ on the fp32 MFMA: a single partial tile with a one-element k step, ragged tiles with
    P % 4 = 2 (the k + kk < P guard), whole tiles."""
    torch.manual_seed(B + NT + P)
    a, t = torch.randn(B, P), torch.randn(NT, P)
    S = torch.full((B, NT), 7.0, device=DEV)
    ops.similarity(a.to(DEV), t.to(DEV), S)
    ref = a.double() @ t.double().t()
    _margin(_rel(S, ref), _rel(a @ t.t(), ref), f"similarity B={B} NT={NT} P={P}")


def _pair_loss(S, off_neg, align, tau, aw, gamma):
    """AlignmentAwareInfoNCE in the dtype of S -> (loss, s_pos, s_neg)."""
    B = S.shape[0]
    i = torch.arange(B)
    sp, sn = S[i, i], S[i, off_neg + i]
    x = (sn - sp) / tau
    ce = torch.logaddexp(x, torch.zeros_like(x))                  # softplus, stable at |x| = 2000
    if align is not None:
        ce = ce * (1 - aw * torch.sigmoid(align.mean(1)))
    return ce.mean() + gamma * F.relu(sn).mean(), sp, sn


@pytest.mark.parametrize("L,has_align,gamma,has_gscale,has_dalign", [(9, True, 0.35, False, True), (1, True, 0.35, True, True),
                                                                     (9, False, 0.35, False, False),
                                                                     (9, True, 0.0, True, False)])
def test_pair_loss(ops, L, has_align, gamma, has_gscale, has_dalign):
    """B = 300 pairs (a thread loop in the forward, two blocks in the backward) read from the
    diagonals of a padded S (ldS = 2B + 8, off_neg = B + 4); (s_neg - s_pos)/tau = +2000 and -2000
    (softplus 2000 and 0, no inf / NaN), one s_neg exactly 0 (relu' = 0); align NULL, gamma = 0,
    gscale given and dalign NULL."""
    torch.manual_seed(L * 7 + int(gamma * 100) + has_gscale)
    B, tau, aw = 300, 0.05, 0.5
    ldS, off_neg = 2 * B + 8, B + 4
    S = torch.randn(B, ldS) * 0.3
    S[0, 0], S[0, off_neg] = 0.0, 100.0
    S[1, 1], S[1, off_neg + 1] = 0.0, -100.0
    S[2, off_neg + 2] = 0.0
    align = torch.randn(B, L) if has_align else None
    gs = 128.0 if has_gscale else 1.0
    tau_, aw_, gamma_ = f32(tau), f32(aw), f32(gamma)

    def fn(S, align):
        return _pair_loss(S, off_neg, align, tau_, aw_, gamma_)

    one = torch.ones(())
    (lref, spr, snr), (dS, dal) = _grads(fn, (S, align), F64, (one, None, None))
    (l32, _, _), (dS32, dal32) = _grads(fn, (S, align), F32, (one, None, None))
    i = torch.arange(B)
    sp, sn, loss = (torch.full((n,), 7.0, device=DEV) for n in (B, B, 1))
    S_d, al_d = S.to(DEV), None if align is None else align.to(DEV)
    ops.pair_loss_fwd(S_d, off_neg, al_d, B, L, tau, aw, gamma, sp, sn, loss)
    assert torch.equal(sp.cpu(), S[i, i]) and torch.equal(sn.cpu(), S[i, off_neg + i])
    assert math.isfinite(float(loss))
    _margin(abs(float(loss) - float(lref)) / abs(float(lref)), abs(float(l32) - float(lref)) / abs(float(lref)),
            f"pair_loss L={L} align={has_align} gamma={gamma}")
    dsp, dsn = torch.full((B,), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    dalign = torch.full((B, L), 7.0, device=DEV) if has_dalign else None
    gscale = torch.tensor([gs], device=DEV) if has_gscale else None
    ops.pair_loss_bwd(sp, sn, al_d, B, L, tau, aw, gamma, gscale, dsp, dsn, dalign)
    assert bool(torch.isfinite(dsp).all()) and bool(torch.isfinite(dsn).all())
    _margin(_rel(dsp, gs * dS[i, i]), _rel(dS32[i, i], dS[i, i]), "pair_loss ds_pos")
    _margin(_rel(dsn, gs * dS[i, off_neg + i]), _rel(dS32[i, off_neg + i], dS[i, off_neg + i]), "pair_loss ds_neg")
    # row 2: s_neg = 0 gets no relu gradient: ds_neg = -ds_pos there, as in rows with s_neg < 0
    assert float(dsn[2]) == -float(dsp[2])
    if has_dalign:
        _margin(_rel(dalign, gs * dal), _rel(dal32, dal), "pair_loss dalign")


@pytest.mark.parametrize("P", [4, 768, 1000])
def test_pair_sim_bwd(ops, P):
    """da = ds_pos·tp + ds_neg·tn, dtp = ds_pos·a, dtn = ds_neg·a: one, three and four (ragged)
    column passes."""
    torch.manual_seed(P)
    B = 3
    a, tp, tn = (torch.randn(B, P) for _ in range(3))
    gp, gn = torch.randn(B), torch.randn(B)
    da, dtp, dtn = (torch.full((B, P), 7.0, device=DEV) for _ in range(3))
    ops.pair_sim_bwd(a.to(DEV), tp.to(DEV), tn.to(DEV), gp.to(DEV), gn.to(DEV), da, dtp, dtn)
    gp, gn = gp.double()[:, None], gn.double()[:, None]
    assert _rel(da, gp * tp.double() + gn * tn.double()) < F32_TOL
    assert _rel(dtp, gp * a.double()) < F32_TOL and _rel(dtn, gn * a.double()) < F32_TOL


@pytest.mark.parametrize("has_gscale", [False, True])
def test_inbatch_ce(ops, has_gscale):
    """NB = 300 global columns (more than the 256 threads), local rows 290..294, padded S and dS:
    loss += weight/B·Σ CE, dS = weight·gscale/B·(softmax - onehot)/tau, padding untouched."""
    torch.manual_seed(17 + has_gscale)
    B, NB, row0, tau, weight = 5, 300, 290, 0.07, 0.7
    ldS, lddS = NB + 4, NB + 8
    S = torch.randn(B, ldS) * 0.3
    gs = 64.0 if has_gscale else 1.0
    tau_, w_ = f32(tau), f32(weight)

    def fn(S):
        ce = F.cross_entropy(S[:, :NB] / tau_, torch.arange(row0, row0 + B), reduction="sum")
        return (w_ / B * ce,)

    (lref,), (dref,) = _grads(fn, (S,), F64, (torch.ones(()),))
    (l32,), (d32,) = _grads(fn, (S,), F32, (torch.ones(()),))
    loss = torch.full((1,), 2.0, device=DEV)
    dS = torch.full((B, lddS), 7.0, device=DEV)
    gscale = torch.tensor([gs], device=DEV) if has_gscale else None
    ops.inbatch_ce(S.to(DEV), B, NB, row0, tau, weight, gscale, loss, dS)
    _margin(abs(float(loss) - 2.0 - float(lref)) / float(lref), abs(float(l32) - float(lref)) / float(lref),
            "inbatch_ce loss")
    _margin(_rel(dS[:, :NB], gs * dref[:, :NB]), _rel(d32[:, :NB], dref[:, :NB]), "inbatch_ce dS")
    assert torch.equal(dS[:, NB:], torch.full((B, lddS - NB), 7.0, device=DEV))


@pytest.mark.parametrize("has_losses", [True, False])
def test_pair_metrics(ops, has_losses):
    """NB = 300 rows and columns: Σ sigmoid(s/τ) on both diagonals, pair accuracy, top-1 hits with
    exact ties in a row (the lowest index wins, as argmax over the first maximum does: a tie won by
    the diagonal within a wave and across waves, one lost to a lower column, one between two other
    columns), the row count and the
    loss term (untouched when losses is NULL); acc accumulates."""
    torch.manual_seed(23)
    NB, tau = 300, 0.1
    off_neg = NB + 4
    S = torch.randn(NB, off_neg + NB) * 0.3
    S[9, 9] = S[9, 200] = 5.0        # hit
    S[11, 5] = S[11, 11] = 5.0       # miss
    S[7, 3] = S[7, 299] = 5.0        # miss
    S[260, 260] = S[260, 299] = 5.0  # hit, past the first thread pass
    S[70, 70] = S[70, 261] = 5.0    # hit: the diagonal in wave 1, its tie in wave 0's second pass
    losses = torch.rand(3) if has_losses else None
    pre = torch.arange(1, 7, dtype=F64)
    acc = pre.to(DEV)
    ops.pair_metrics(S.to(DEV), off_neg, tau, acc, None if losses is None else losses.to(DEV), loss_w=8.0)
    i = torch.arange(NB)
    sp, sn = S[i, i], S[i, off_neg + i]
    got = (acc.cpu() - pre).tolist()
    tau_ = f32(tau)
    for k, s in enumerate((sp, sn)):
        ref = float(torch.sigmoid(s.double() / tau_).sum())
        _margin(abs(got[k] - ref) / ref, abs(float(torch.sigmoid(s / tau_).double().sum()) - ref) / ref,
                f"pair_metrics acc[{k}]")
    assert got[2] == float((sp > sn).sum())
    assert got[3] == float((S[:, :NB].argmax(1) == i).sum())
    assert got[4] == float(NB)
    ref5 = 8.0 * float(losses.double().sum()) if has_losses else 0.0
    assert abs(got[5] - ref5) <= 1e-12 * max(ref5, 1.0)


# ------------------------------------------------------------------ cross-modal attention
def _xattn(q, k, v, mask, B, S, nh, nq, scale, drops):
    """nq single-vector query sets over one K/V -> (out [nq·B, P], probs [nq·B, nh, S])."""
    P = q.shape[1]
    d = P // nh
    kh, vh = (x.reshape(B, S, nh, d).transpose(1, 2) for x in (k, v))
    outs, prs = [], []
    for qi in range(nq):
        a = (q[qi * B:(qi + 1) * B].reshape(B, nh, 1, d) @ kh.transpose(-1, -2)) * scale
        if mask is not None:
            a = a.masked_fill(mask.view(B, 1, 1, S) == 0, -1e9)
        p = a.softmax(-1)
        prs.append(p.reshape(B, nh, S))
        if drops is not None:
            p = p * drops[qi].to(p.dtype).view(B, nh, 1, S)
        outs.append((p @ vh).transpose(1, 2).reshape(B, P))
    return torch.cat(outs), torch.cat(prs)


@pytest.mark.parametrize("S", [1, 5, 257])
@pytest.mark.parametrize("P", [96, 32, 1024])
def test_xattn(ops, P, S):
    """xattn_fwd / _bwd / _bwd_bf16 with 4 heads of 24 / 8 / 256 (42 row groups and 4 idle threads,
    128 row groups, 4 row groups), one key, fewer keys than row groups and more keys than threads;
    one and two query sets, dropout, no mask and a mask with a partly and a fully masked sample
    (uniform weights, no score gradient); K and V are column views of one padded buffer
    (ldkv = 2P + 8) and so are dK, dV (lddkv = 2P + 8, padding untouched); the fp32 dK / dV
    accumulate, the bf16 ones equal the fp32 result rounded and their column sums go to fp64."""
    nh, B = 4, 3
    d, ld = P // nh, 2 * P + 8
    scale = f32(d ** -0.5)
    torch.manual_seed(P + S)
    buf = torch.randn(B * S, ld).bfloat16()
    k, v = buf[:, :P], buf[:, P:2 * P]
    buf_d = buf.to(DEV)
    k_d, v_d = buf_d[:, :P], buf_d[:, P:2 * P]
    for nq, drop_p, masked in ((1, 0.0, False), (2, 0.1, True), (1, 0.1, True), (2, 0.0, False)):
        what = f"xattn P={P} S={S} nq={nq} drop={drop_p} mask={masked}"
        q, dout = torch.randn(nq * B, P), torch.randn(nq * B, P)
        mask = None
        if masked:
            mask = torch.ones(B, S, dtype=I32)
            mask[1] = 0
            if S > 2:
                mask[0, S - 2:] = 0
        seeds = (1234, 777)[:nq]
        drops = None
        if drop_p > 0:
            idx = np.arange(B * nh * S).astype(np.uint64)
            drops = [torch.from_numpy(drop_scale(sd, idx, f32(drop_p))) for sd in seeds]

        def fn(q, k, v):
            return _xattn(q, k, v, mask, B, S, nh, nq, scale, drops)

        (oref, pref), (dqr, dkr, dvr) = _grads(fn, (q, k, v), F64, (dout, None))
        (o32, p32), (dq32, dk32, dv32) = _grads(fn, (q, k, v), F32, (dout, None))
        q_d, do_d = q.to(DEV), dout.to(DEV)
        m_d = None if mask is None else mask.view(-1).to(DEV)
        probs = torch.full((nq * B * nh * S,), 7.0, device=DEV)
        out = torch.full((nq * B, P), 7.0, device=DEV)
        ops.xattn_fwd(q_d, k_d, v_d, m_d, B, S, nh, probs, out, seeds, drop_p=drop_p)
        _margin(_rel(probs, pref.reshape(-1)), _rel(p32, pref), what + " probs")
        _margin(_rel(out, oref), _rel(o32, oref), what + " out")

        def bwd(init, bf16=False):
            dq = torch.full((nq * B, P), 7.0, device=DEV)
            dkv = init.clone()
            cs = torch.zeros(2 * P, device=DEV) if bf16 else None
            ops.xattn_bwd(q_d, k_d, v_d, probs, do_d, B, S, nh, dq, dkv[:, :P], dkv[:, P:2 * P], seeds, drop_p=drop_p,
                          colsum=cs, mask=m_d)
            return dq, dkv, cs

        pre = torch.randn(B * S, ld, device=DEV)
        dq, dkv, _ = bwd(torch.zeros(B * S, ld, device=DEV))
        _margin(_rel(dq, dqr), _rel(dq32, dqr), what + " dq")
        _margin(_rel(dkv[:, :P], dkr), _rel(dk32, dkr), what + " dk")
        _margin(_rel(dkv[:, P:2 * P], dvr), _rel(dv32, dvr), what + " dv")
        assert float(dkv[:, 2 * P:].abs().max()) == 0.0
        dq2, dkv2, _ = bwd(pre)                                     # +=: one fp32 add on top of the prefill
        assert torch.equal(dq2, dq) and torch.equal(dkv2[:, 2 * P:], pre[:, 2 * P:])
        assert _rel(dkv2[:, :2 * P], pre[:, :2 * P].double() + dkv[:, :2 * P].double()) < F32_TOL
        dqb, dkvb, cs = bwd(torch.full((B * S, ld), 7.0, device=DEV, dtype=BF16), bf16=True)
        assert torch.equal(dqb, dq) and torch.equal(dkvb[:, :2 * P], dkv[:, :2 * P].bfloat16())
        assert torch.equal(dkvb[:, 2 * P:], torch.full((B * S, 8), 7.0, device=DEV, dtype=BF16))
        csr = torch.cat([dkr, dvr], 1).sum(0)
        _margin(_rel(cs, csr), _rel(torch.cat([dk32, dv32], 1).sum(0), csr), what + " colsum")


def test_xattn_error_returns(lib):
    """Refused before any launch: dh % 8 != 0, P > 1024, nq·S > 16384, ldkv % 8 != 0, nq = 3, and the
    bf16 backward without colsum_part."""
    t = torch.zeros(1 << 16, device=DEV)
    s = _s(lib)

    def fwd(B, S, P, nh, nq, ldkv):
        return lib.fn("ste_xattn_fwd")(_p(t), _p(t), _p(t), ldkv, None, B, S, P, nh, nq, 0.25, 0.0, 1, 2, _p(t), _p(t), s)

    def bwd(name, B, S, P, nh, nq, ldkv, *tail):
        return lib.fn(name)(_p(t), _p(t), _p(t), ldkv, _p(t), _p(t), None, B, S, P, nh, nq, 0.25, 0.0, 1, 2, _p(t), _p(t),
                            _p(t), P, *tail, s)

    for B, S, P, nh, nq, ldkv in ((2, 4, 48, 4, 1, 48), (1, 2, 1032, 4, 1, 1032), (1, 8193, 32, 4, 2, 32),
                                  (2, 4, 32, 4, 1, 36), (2, 4, 32, 4, 3, 32)):
        assert fwd(B, S, P, nh, nq, ldkv) == ERR_SHAPE, (B, S, P, nh, nq, ldkv)
        assert bwd("ste_xattn_bwd", B, S, P, nh, nq, ldkv) == ERR_SHAPE
        assert bwd("ste_xattn_bwd_bf16", B, S, P, nh, nq, ldkv, _p(t)) == ERR_SHAPE
    assert bwd("ste_xattn_bwd_bf16", 2, 4, 32, 4, 1, 32, None) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ------------------------------------------------------------------ pooling
def _attn_pool(t, w2, b2, h, mask, B, L):
    s = (t @ w2 + b2).view(B, L)
    if mask is not None:
        s = s.masked_fill(mask.view(B, L) == 0, -1e9)
    w = s.softmax(1)
    return (w.unsqueeze(1) @ h.view(B, L, -1)).squeeze(1), w


@pytest.mark.parametrize("f32_states", [False, True])
@pytest.mark.parametrize("B,L,H,Hh", [(1, 1, 4, 4), (2, 17, 8, 1024), (2, 70, 260, 4)])
def test_attn_pool(ops, B, L, H, Hh, f32_states):
    """attn_pool_fwd / _bwd on bf16 and on fp32 states: one row of one quad; Hh = 1024 (one thread
    group in the backward's dz kernel); Hh = 4 (256 groups for 16-row chunks), H = 260 and a ragged
    last chunk.  mask NULL and a ragged mask; the bf16 pooled copy and dt_lo, dw2, db2, db1 each NULL
    in turn; dh, dw2, db2, db1 accumulate; every output is bit-identical between runs."""
    torch.manual_seed(B * L + H + Hh)
    sdt = F32 if f32_states else BF16
    t = torch.tanh(torch.randn(B * L, Hh)).to(sdt)
    h = (torch.randn(B * L, H) + 1.0).to(sdt)
    w2, b2, dp = torch.randn(Hh) * 0.3, torch.randn(1), torch.randn(B, H)
    t_d, h_d, w2_d, b2_d, dp_d = (x.to(DEV) for x in (t, h, w2, b2, dp))
    fwd = ops.attn_pool_fwd_f32 if f32_states else ops.attn_pool_fwd
    for masked in ((False, True) if L > 3 else (False,)):
        what = f"attn_pool B={B} L={L} H={H} Hh={Hh} f32={f32_states} mask={masked}"
        mask = None
        if masked:
            mask = torch.ones(B, L, dtype=I32)
            mask[B - 1, L - 3:] = 0
        m_d = None if mask is None else mask.view(-1).to(DEV)

        def fn(t, w2, b2, h):
            return _attn_pool(t, w2, b2, h, mask, B, L)

        (pref, wref), (gt, gw2, gb2, gh) = _grads(fn, (t, w2, b2, h), F64, (dp, None))
        (p32, w32), (gt32, gw232, gb232, gh32) = _grads(fn, (t, w2, b2, h), F32, (dp, None))
        weights, pooled = torch.full((B * L,), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
        pooledb = torch.full((B, H), 7.0, device=DEV, dtype=BF16)
        fwd(t_d, w2_d, b2_d, h_d, m_d, B, L, weights, pooled, pooledb)
        _margin(_rel(weights, wref.reshape(-1)), _rel(w32, wref), what + " weights")
        _margin(_rel(pooled, pref), _rel(p32, pref), what + " pooled")
        assert torch.equal(pooledb, pooled.bfloat16())
        w_2, p_2 = torch.empty_like(weights), torch.empty_like(pooled)
        fwd(t_d, w2_d, b2_d, h_d, m_d, B, L, w_2, p_2, None)
        assert torch.equal(w_2, weights) and torch.equal(p_2, pooled)

        opt = ("dw2", "db2", "db1") if f32_states else ("dt_lo", "dw2", "db2", "db1")
        zero = dict(dh=torch.zeros(B * L, H, device=DEV), dw2=torch.zeros(Hh, device=DEV),
                    db2=torch.zeros(1, device=DEV), db1=torch.zeros(Hh, device=DEV))
        pre = {n: torch.randn_like(x) for n, x in zero.items()}

        def run(init, has=opt):
            o = {n: (init[n].clone() if n == "dh" or n in has else None) for n in init}
            o["dt"] = torch.full((B * L, Hh), 7.0, device=DEV, dtype=sdt)
            o["dt_lo"] = torch.full((B * L, Hh), 7.0, device=DEV, dtype=BF16) if "dt_lo" in has else None
            if f32_states:
                ops.attn_pool_bwd_f32(t_d, w2_d, h_d, weights, dp_d, B, L, o["dh"], o["dt"], o["dw2"], o["db2"],
                                      db1=o["db1"], mask=m_d)
            else:
                ops.attn_pool_bwd(t_d, w2_d, h_d, weights, dp_d, B, L, o["dh"], o["dt"], o["dw2"], o["db2"],
                                  db1=o["db1"], dz_lo=o["dt_lo"], mask=m_d)
            return o

        o1 = run(zero)
        dzr, dz32 = gt * (1 - t.double() ** 2), gt32 * (1 - t.float() ** 2)
        _margin(_rel(o1["dh"], gh), _rel(gh32, gh), what + " dh")
        if f32_states:
            _margin(_rel(o1["dt"], dzr), _rel(dz32, dzr), what + " dt")
        else:
            _assert_bf16_close(o1["dt"], dzr, what + " dt")
            # hi = bf16(dz) is off by <= 2^-9·|dz| and lo = bf16(dz - hi) by <= 2^-9·|dz - hi|, so hi + lo
            # is the kernel's fp32 dz to 2^-18 relative, on top of that fp32 value's own margin
            err, e32 = _rel(o1["dt"].double() + o1["dt_lo"].double(), dzr), _rel(dz32, dzr)
            print(f"{what} dt + dt_lo: kernel {err:.3e}, fp32 torch {e32:.3e}")
            assert err <= max(1e-6, 10 * e32) + 2.0 ** -18, (what, err, e32)
        _margin(_rel(o1["dw2"], gw2), _rel(gw232, gw2), what + " dw2")
        _margin(_rel(o1["db1"], dzr.sum(0)), _rel(dz32.sum(0), dzr.sum(0)), what + " db1")
        kmax = int(w2.abs().argmax())                     # dscore = d(t·w2 + b2), read off the t gradient
        den = max(float((gt[:, kmax] / w2[kmax].double()).abs().sum()), 1e-300)
        _margin(abs(float(o1["db2"]) - float(gb2)) / den, abs(float(gb232) - float(gb2)) / den, what + " db2 / Σ|dscore|")
        o2 = run(pre)                                     # +=: one fp32 add on top of the prefill
        for n in zero:
            assert _rel(o2[n], pre[n].double() + o1[n].double()) < F32_TOL, n
        for skip in (None,) + opt:                        # each optional output NULL in turn; None: a plain rerun
            o = run(zero, tuple(n for n in opt if n != skip))
            for n, x in o.items():
                assert x is None or torch.equal(x, o1[n]), (skip, n)


@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("B,L,H", [(1, 1, 4), (2, 300, 260)])
def test_mean_pool(ops, B, L, H, cls):
    """mean_pool_fwd on bf16 and fp32 states, CLS row and (masked) mean, mask NULL and a ragged mask;
    L = 300 > 256 threads, H = 260 the 65th quad; weighted_pool_bwd accumulates weight·dpooled into a
    prefilled dh and leaves rows of weight 0 untouched."""
    torch.manual_seed(B * L + H + cls)
    dp = torch.randn(B, H)
    for sdt in (BF16, F32):
        for masked in ((False, True) if L > 1 else (False,)):
            what = f"mean_pool B={B} L={L} H={H} cls={cls} {sdt} mask={masked}"
            h = (torch.randn(B * L, H) + 1.0).to(sdt)
            mask = None
            if masked:
                mask = torch.ones(B, L, dtype=I32)
                mask[B - 1, L // 2:] = 0
            m = torch.ones(B, L, dtype=F64) if mask is None else mask.double()
            wref = F.one_hot(torch.zeros(B, dtype=I64), L).double() if cls else m / m.sum(1, keepdim=True).clamp_min(1e-9)
            pref = (wref[:, :, None] * h.double().view(B, L, H)).sum(1)
            p32 = (wref.float()[:, :, None] * h.float().view(B, L, H)).sum(1)
            weights, pooled = torch.full((B * L,), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
            pooledb = torch.full((B, H), 7.0, device=DEV, dtype=BF16)
            ops.mean_pool_fwd(h.to(DEV), None if mask is None else mask.view(-1).to(DEV), B, L, cls, weights, pooled, pooledb)
            assert _rel(weights, wref.reshape(-1)) < F32_TOL
            _margin(_rel(pooled, pref), _rel(p32, pref), what)
            assert torch.equal(pooledb, pooled.bfloat16())
            pre = torch.randn(B * L, H, device=DEV)
            dh = pre.clone()
            ops.weighted_pool_bwd(weights, dp.to(DEV), B, L, dh)
            ref = pre.double().cpu() + weights.double().cpu()[:, None] * dp.double().repeat_interleave(L, 0)
            assert _rel(dh, ref) < F32_TOL
            untouched = (weights == 0)
            assert torch.equal(dh[untouched], pre[untouched])


# ------------------------------------------------------------------ alignment attention
def _align(q, kv, kmask, B, L, T, P, nh, scale, drop):
    """nn.MultiheadAttention core on kv = [K | V] -> (out [B·L, P], probs [B, nh, L, T])."""
    d = P // nh
    qh = q.reshape(B, L, nh, d).transpose(1, 2)
    kh, vh = (x.reshape(B, T, nh, d).transpose(1, 2) for x in (kv[:, :P], kv[:, P:2 * P]))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if kmask is not None:
        s = s.masked_fill(kmask.view(B, 1, 1, T) == 0, float("-inf"))
    p = s.softmax(-1)
    pd = p if drop is None else p * drop.to(p.dtype).view(B, nh, L, T)
    return (pd @ vh).transpose(1, 2).reshape(B * L, P), p


def _align_check(ops, B, L, T, P, nh, drop_p, masked):
    """Forward and backward on padded row strides (q, kv, out, dout, dq, dkv each a column view of a
    wider buffer whose padding stays untouched) against fp64."""
    what = f"align_attn B={B} L={L} T={T} P={P} drop={drop_p} mask={masked}"
    torch.manual_seed(L * 1000 + T + P)
    d = P // nh
    scale = float(np.float32(1.0) / np.sqrt(np.float32(d)))
    seed = 7
    qb, kvb, dob = (torch.randn(r, c).bfloat16() for r, c in ((B * L, P + 8), (B * T, 2 * P + 8), (B * L, P + 8)))
    q, kv, do = qb[:, :P], kvb[:, :2 * P], dob[:, :P]
    kmask = None
    if masked:                                       # the last clip's tail; never a whole clip (NaN in the reference too)
        kmask = torch.ones(B, T, dtype=I32)
        kmask[B - 1, T - max(1, T // 3):] = 0
    drop = None
    if drop_p > 0:
        drop = torch.from_numpy(drop_scale(seed, np.arange(B * nh * L * T).astype(np.uint64), f32(drop_p)))

    def fn(q, kv):
        return _align(q, kv, kmask, B, L, T, P, nh, scale, drop)

    (oref, pref), (dqr, dkvr) = _grads(fn, (q, kv), F64, (do, None))
    (o32, p32), (dq32, dkv32) = _grads(fn, (q, kv), F32, (do, None))
    qb_d, kvb_d, dob_d = qb.to(DEV), kvb.to(DEV), dob.to(DEV)
    m_d = None if kmask is None else kmask.view(-1).to(DEV)
    probs = torch.full((B * nh * L * T,), 7.0, device=DEV)
    outb = torch.full((B * L, P + 16), 7.0, device=DEV, dtype=BF16)
    ops.align_attn_fwd(qb_d[:, :P], kvb_d[:, :2 * P], m_d, B, L, T, nh, probs, outb[:, :P], drop_p=drop_p, seed=seed)
    _margin(_rel(probs, pref.reshape(-1)), _rel(p32, pref), what + " probs")
    _assert_bf16_close(outb[:, :P], oref, what + " out")
    assert float((outb[:, P:].float() - 7.0).abs().max()) == 0.0
    dqb = torch.full((B * L, P + 24), 7.0, device=DEV, dtype=BF16)
    dkvb = torch.full((B * T, 2 * P + 4), 7.0, device=DEV)
    dsbuf = torch.empty(B * nh * L * T, device=DEV)
    ops.align_attn_bwd(qb_d[:, :P], kvb_d[:, :2 * P], probs, dob_d[:, :P], B, L, T, nh, dsbuf, dqb[:, :P], dkvb[:, :2 * P],
                       drop_p=drop_p, seed=seed)
    _assert_bf16_close(dqb[:, :P], dqr, what + " dq")
    _margin(_rel(dkvb[:, :2 * P], dkvr), _rel(dkv32, dkvr), what + " dkv")
    assert float((dqb[:, P:].float() - 7.0).abs().max()) == 0.0 and float((dkvb[:, 2 * P:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("drop_p,masked", [(0.0, False), (0.1, True)])
@pytest.mark.parametrize("B,L,T,P", [(1, 1, 1, 32), (2, 9, 300, 32), (1, 70, 17, 768)])
def test_align_attn(ops, B, L, T, P, drop_p, masked):
    """One query, one key; L = 9 ragged against 8 queries per block with T = 300 > 256; d = 192 (the
    backward's limit) with L = 70 (two 64-query chunks in the kv kernel) and T = 17 ragged against
    its 16-key blocks.  kmask NULL, or a mask on the last clip's tail (T = 1 has no tail to mask
    short of the whole clip: it runs unmasked with dropout)."""
    _align_check(ops, B, L, T, P, 4, drop_p, masked and T > 1)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU_BWD, ACT_TANH_BWD_OUT])
@pytest.mark.parametrize("M,K", [(1, 1), (5, 300)])
def test_rank1_bwd(ops, M, K, act):
    """out = a ⊗ w ⊙ act'(z) (bf16), dw += aᵀz, db += Σ a for each activation code; K = 300: two
    blocks, the second partly idle; dw / db NULL."""
    torch.manual_seed(M * K + act)
    a, w, z = torch.randn(M), torch.randn(K), torch.randn(M, K)
    z = (z.relu() if act == ACT_RELU_BWD else z.tanh() if act == ACT_TANH_BWD_OUT else z).bfloat16()
    zd = z.double()
    g = (zd > 0).double() if act == ACT_RELU_BWD else 1 - zd * zd if act == ACT_TANH_BWD_OUT else torch.ones_like(zd)
    a_d, w_d, z_d = a.to(DEV), w.to(DEV), z.to(DEV)
    out = torch.full((M, K), 7.0, device=DEV, dtype=BF16)
    dw, db = torch.zeros(K, device=DEV), torch.zeros(1, device=DEV)
    ops.rank1_bwd(a_d, w_d, z_d, act, out, dw, db)
    _assert_bf16_close(out, a.double()[:, None] * w.double()[None] * g, "out")
    assert _rel(dw, a.double() @ zd) < F32_TOL
    assert abs(float(db) - float(a.double().sum())) <= F32_TOL * float(a.double().abs().sum())
    pre_w, pre_b = torch.randn(K, device=DEV), torch.randn(1, device=DEV)
    dw2, db2, out2 = pre_w.clone(), pre_b.clone(), torch.empty_like(out)
    ops.rank1_bwd(a_d, w_d, z_d, act, out2, dw2, db2)
    assert _rel(dw2, pre_w.double() + dw.double()) < F32_TOL and _rel(db2, pre_b.double() + db.double()) < F32_TOL
    out3 = torch.empty_like(out)
    ops.rank1_bwd(a_d, w_d, z_d, act, out3, None, None)
    assert torch.equal(out2, out) and torch.equal(out3, out)


# ------------------------------------------------------------------ documented limits
def test_align_attn_limit(ops, lib):
    """T = 2048, the largest accepted: 8·T·4 B of dynamic LDS on top of 8 KiB static must fit the
    per-block limit the runtime reports; T = 2049 is refused by both entry points."""
    T = 2048
    assert _lds_limit() >= 8 * T * 4 + 8 * 1024, _lds_limit()
    _align_check(ops, 1, 9, T, 32, 4, 0.0, False)
    t = torch.zeros(1 << 16, device=DEV)
    s = _s(lib)
    assert lib.fn("ste_align_attn_fwd")(_p(t), 32, _p(t), 64, None, 1, 9, T + 1, 32, 4, 0.0, 1, _p(t), _p(t), 32, s) == ERR_SHAPE
    assert lib.fn("ste_align_attn_bwd")(_p(t), 32, _p(t), 64, _p(t), _p(t), 32, 1, 9, T + 1, 32, 4, 0.0, 1, _p(t), _p(t), 32,
                                        _p(t), 64, s) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_mean_pool_limit(ops, lib):
    """L = 16384, the largest accepted: L·4 B of dynamic LDS + 32 B static; L = 16385 is refused."""
    B, L, H = 1, 16384, 4
    assert _lds_limit() >= L * 4 + 32, _lds_limit()
    torch.manual_seed(5)
    mask = torch.ones(B, L, dtype=I32)
    mask[0, L - 100:] = 0
    for sdt in (BF16, F32):
        h = (torch.randn(B * L, H) + 1.0).to(sdt)
        wref = mask.double() / mask.sum()
        pref = (wref[:, :, None] * h.double().view(B, L, H)).sum(1)
        p32 = (wref.float()[:, :, None] * h.float().view(B, L, H)).sum(1)
        weights, pooled = torch.full((B * L,), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
        ops.mean_pool_fwd(h.to(DEV), mask.view(-1).to(DEV), B, L, 0, weights, pooled)
        assert _rel(weights, wref.reshape(-1)) < F32_TOL
        _margin(_rel(pooled, pref), _rel(p32, pref), f"mean_pool L={L} {sdt}")
    t = torch.zeros(1 << 17, device=DEV)
    for name in ("ste_mean_pool_fwd", "ste_mean_pool_fwd_f32"):
        assert lib.fn(name)(_p(t), None, 1, L + 1, 4, 0, _p(t), _p(t), None, _s(lib)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_attn_pool_limit(ops, lib):
    """L = 8192, the largest the forward accepts: L·4 B of dynamic LDS + 8 KiB static in the
    weighted-sum kernel; L = 8193 is refused."""
    B, L, H, Hh = 1, 8192, 4, 4
    assert _lds_limit() >= L * 4 + 8 * 1024, _lds_limit()
    torch.manual_seed(6)
    w2, b2 = torch.randn(Hh) * 0.3, torch.randn(1)
    for sdt, fwd in ((BF16, ops.attn_pool_fwd), (F32, ops.attn_pool_fwd_f32)):
        t, h = torch.tanh(torch.randn(B * L, Hh)).to(sdt), (torch.randn(B * L, H) + 1.0).to(sdt)
        pref, wref = _attn_pool(t.double(), w2.double(), b2.double(), h.double(), None, B, L)
        p32, w32 = _attn_pool(t.float(), w2, b2, h.float(), None, B, L)
        weights, pooled = torch.full((B * L,), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
        fwd(t.to(DEV), w2.to(DEV), b2.to(DEV), h.to(DEV), None, B, L, weights, pooled)
        _margin(_rel(weights, wref.reshape(-1)), _rel(w32, wref), f"attn_pool L={L} {sdt} weights")
        _margin(_rel(pooled, pref), _rel(p32, pref), f"attn_pool L={L} {sdt} pooled")
    z = torch.zeros(1 << 16, device=DEV)
    for name in ("ste_attn_pool_fwd", "ste_attn_pool_fwd_f32"):
        assert lib.fn(name)(_p(z), _p(z), _p(z), _p(z), None, 1, L + 1, 4, 4, _p(z), _p(z), None, _s(lib)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0


def test_heads_error_returns(lib):
    """Refused before any launch: align d % 8 != 0 (both entries) and backward d = 200 (16·200 > 12·256
    accumulator slots; the forward accepts it), attn_pool_bwd Hh = 1028."""
    t = torch.zeros(1 << 16, device=DEV)
    s = _s(lib)

    def afwd(P):
        return lib.fn("ste_align_attn_fwd")(_p(t), P, _p(t), 2 * P, None, 1, 2, 3, P, 4, 0.0, 1, _p(t), _p(t), P, s)

    def abwd(P):
        return lib.fn("ste_align_attn_bwd")(_p(t), P, _p(t), 2 * P, _p(t), _p(t), P, 1, 2, 3, P, 4, 0.0, 1, _p(t), _p(t), P,
                                            _p(t), 2 * P, s)

    assert afwd(48) == ERR_SHAPE and abwd(48) == ERR_SHAPE
    assert abwd(800) == ERR_SHAPE
    for name, lo in (("ste_attn_pool_bwd", (_p(t),)), ("ste_attn_pool_bwd_f32", ())):
        assert lib.fn(name)(_p(t), _p(t), _p(t), _p(t), _p(t), None, 1, 2, 1028, 4, _p(t), _p(t), *lo, _p(t), _p(t), _p(t),
                            _p(t), s) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
