"""The hot path as an explicit HIP schedule: forward and backward of the whole
contrastive step (two encoders + heads), every op a libste.so kernel.

Reference call stack being replaced (ref = /root/reference/training/trainer_unfreeze.py):
  EnhancedAudioTextModel.compute_pos_neg_embeddings  ref:502-565
    encode_text x2 (pos, neg)                        ref:567-585  -> XLM-R (batched pos+neg here)
    encode_audio                                     ref:587-641  -> Wav2Vec2Bert (Conformer)
    apply_cross_modal_attention x2                   ref:643-682
    word_level_alignment (optional)                  ref:550-558
    F.normalize x3                                   ref:561-563
and the autograd backward of all of it.

Data layout in HBM: activations are row-major [rows, features]; rows = batch*time
(audio) or 2*batch*tokens (text, pos rows then neg rows).  Residual streams and
LayerNorm inputs are fp32; every GEMM operand is bf16 (MFMA), accumulation fp32.
Backward writes parameter gradients straight into the flat gradient buffer of
store.py (beta=1 accumulation), so micro-batch accumulation needs no extra pass.
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops
from ._lib import (ACT_GELU, ACT_GELU_BWD, ACT_NONE, ACT_RELU, ACT_RELU_BWD, ACT_SWISH, ACT_SWISH_BWD,
                   ACT_TANH)

BF16, F32 = torch.bfloat16, torch.float32
_GOLD = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def _site_seed(base: int, site: int) -> int:
    x = (base + (site + 1) * _GOLD) & _M64
    x ^= x >> 31
    return (x * 0xBF58476D1CE4E5B9) & _M64


# parameter names of the post-LN layer (Engine._postln_fwd / _postln_bwd)
XLMR_NAMES = dict(layer="text_encoder.encoder.layer.{i}.", q="attention.self.query", o="attention.output.dense",
                  ln1="attention.output.LayerNorm", fi="intermediate.dense", fo="output.dense", ln2="output.LayerNorm")
W2V2_NAMES = dict(layer="audio_encoder.encoder.layers.{i}.", q="attention.q_proj", o="attention.out_proj",
                  ln1="layer_norm", fi="feed_forward.intermediate_dense", fo="feed_forward.output_dense",
                  ln2="final_layer_norm")


class Ctx(dict):
    """Saved activations of one forward (freed when backward finishes)."""


class Engine:
    def __init__(self, model):
        self.m = model
        self.s = model.store
        self.acfg = model.audio_cfg
        self.tcfg = model.text_cfg
        self._ws = {}
        self._side = None
        # the text encoder (forward and backward) runs on a second HIP stream, concurrently with
        # the audio encoder: its GEMMs are too small to fill 256 CUs (8,192 rows) and overlap the
        # audio side's bandwidth-bound kernels.  STE_TEXT_STREAM=0: one stream (A/B runs).
        self.overlap = _lib.ab_env("STE_TEXT_STREAM", "1") != "0"
        # layerdrop draws (tf:…wav2vec2_bert…:519-522): the global torch RNG unless a trainer sets a
        # generator (TrainStep broadcasts one seed so every data-parallel rank drops the same layers)
        self.layerdrop_gen = None
        # a Conformer layer's final LN and the next layer's FFN1 LN as one fused pass (forward and
        # backward, ste_layernorm_*_pair); STE_LN_PAIR=0: separate launches (A/B runs)
        self.ln_pair = _lib.ab_env("STE_LN_PAIR", "1") != "0"
        # with the text stream: enqueue the text forward after the audio encoder's first layer instead
        # of before it (Engine.forward); STE_TEXT_AFTER_LAYER=0: before (A/B runs)
        self.text_after_first_layer = _lib.ab_env("STE_TEXT_AFTER_LAYER", "1") != "0"
        # the text encoder's forward to ~fp32 accuracy (split-bf16 GEMMs, fp32 attention): the loss
        # gradient differences the positive and corrupted transcripts' embeddings, so their bf16
        # forward rounding reappeared in every gradient downstream.  STE_TEXT_PRECISE=0:
        # the plain bf16 forward (A/B runs only)
        self.precise_text = _lib.ab_env("STE_TEXT_PRECISE", "1") != "0"
        # with precise_text: the text backward to ~fp32 accuracy as well (_postln_bwd_x2: fp32 text
        # attention backward, split-bf16 dY and dW operands).  Opt-in: it halves the loss-derived
        # error of the text weights (tests/test_model_gpu.py, tests/precision_probe_text.py) for
        # 2.9 % of the c2 step (its extra side-stream work competes with the audio chain:
        # profiles/r5e_text_bwd_ab.txt); off, the backward reads bf16 copies of the precise forward's
        # activations (_postln_bwd).  Set the attribute before the first forward.
        self.precise_text_bwd = _lib.ab_env("STE_TEXT_PRECISE_BWD", "0") == "1"

    @property
    def fp8(self):
        """MX-fp8 forward GEMMs in the Conformer layers (model fp8_gemm=True, BASELINE config 5)."""
        return bool(getattr(self.m, "fp8_gemm", False))

    @property
    def fp8_bwd(self):
        """Also the Conformer layers' input-gradient GEMMs (dX = dY·W) on MX-fp8 (opt-in A/B of
        config 5: model.fp8_bwd = True together with fp8_gemm; weight gradients stay bf16)."""
        return self.fp8 and bool(getattr(self.m, "fp8_bwd", False))

    WS_BYTES = 80 << 20   # split-K slabs of the weight-gradient GEMMs (largest: 7 x 3072 x 768 fp32)

    @property
    def ws(self):
        """Split-K workspace of the CURRENT stream (the text and audio backward run concurrently)."""
        return ops.stream_ws(self.s.device, self.WS_BYTES // 4, cache=self._ws)

    def _await_params(self, *names):
        """Order the current stream after the overlapped optimizer's update of these parameter
        blocks (TrainStep(overlap_optimizer=True) sets param_events; waiting on a finished event
        costs nothing)."""
        evs = getattr(self, "param_events", None)
        if evs:
            cur = torch.cuda.current_stream(self.s.device)
            for n in names:
                ev = evs.get(n)
                if ev is not None:
                    cur.wait_event(ev)

    def _side_stream(self):
        if not (self.overlap and self.s.device.type == "cuda"):
            return None
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.s.device)
        return self._side

    # ------------------------------------------------------------- helpers
    def _e(self, *shape, dtype=F32):
        return torch.empty(shape, device=self.s.device, dtype=dtype)

    def _z(self, *shape, dtype=F32):
        return torch.zeros(shape, device=self.s.device, dtype=dtype)

    def _dw(self, dy_b, x_b, wname, fused=1):
        """dW[N,K] += dyᵀ·x into the flat gradient buffer (if the weight receives gradients)."""
        g = self.s.fused(wname, fused, "g")
        if g is None:
            return
        g2 = g.view(g.shape[0], -1)
        ops.linear_dw(dy_b, x_b, out=g2, beta=1.0, ws=self.ws)

    def _dx(self, dy, wname, fused=1, **kw):
        """dX = dY·W of an encoder Linear on the KC-KC GEMM with the cached k-contiguous Wᵀ
        (ParamStore.wt): 15-20 % faster than reading W k-major through transposing LDS reads,
        and bit-identical to it (same reduction order).  Outputs too narrow to fill the CUs with
        256x256 tiles (the text encoder's N = 768) take ste_gemm's few-tile split-K plan; the
        workspace is always passed and the library decides (ste_gemm_kernel)."""
        kw.setdefault("ws", self.ws)
        return ops.linear(dy, self.s.wt(wname, fused), **kw)

    def _dx_mx8(self, dy, wname, fused=1, **kw):
        """dX = dY·W on the MX-fp8 GEMM (opt-in engine.fp8_bwd, config 5): dY block-quantised along
        its row (the reduction axis: 32 outputs per E8M0 scale) by ste_mx8_quant, W from
        ParamStore.wtq (Wᵀ quantised along `out`).  Same epilogues as _dx, except that a bias
        gradient is the ordered column sum of the bf16 output (run-to-run deterministic; the MX
        kernel has no partial-sum workspace)."""
        kw.pop("ws", None)
        cs = kw.pop("colsum", None)
        out = ops.linear_mx8(ops.mx8_quant(dy), self.s.wtq(wname, fused), **kw)
        if cs is not None:
            ops.colsum(out, cs)
        return out

    def _db(self, x, bname, fused=1):
        g = self.s.fused(bname, fused, "g")
        if g is not None:
            ops.colsum(x, g)

    def _ln(self, x, name, eps, **kw):
        return ops.layernorm_fwd(x, self.s.p(name + ".weight"), self.s.p(name + ".bias"), eps, **kw)

    def _ln_bwd(self, dy, x, stats, name, **kw):
        g = self.s.g(name + ".weight")
        return ops.layernorm_bwd(dy, x, stats[0], stats[1], self.s.p(name + ".weight"), beta=self.s.p(name + ".bias"),
                                 dgamma=g, dbeta=self.s.g(name + ".bias"), **kw)

    # ================================================================ audio
    @property
    def raw_audio(self):
        """wav2vec2 raw-waveform encoder (wav2vec2.py) instead of w2v-bert's fbank Conformer."""
        from .modules import W2V2Config
        return isinstance(self.acfg, W2V2Config)

    def audio_forward(self, feats, mask_i64, train, base_seed, ctx, save=True, lengths=None):
        """lengths: host list of each clip's valid frames (None: read from mask_i64 when
        SpecAugment needs them, one device->host sync)."""
        if self.raw_audio:
            from . import wav2vec2
            self._await_params("audio", "late")
            return wav2vec2.forward(self, feats, mask_i64, train, base_seed, ctx, save, lengths=lengths)
        self._await_params("audio")   # feature projection (and SpecAugment's embedding)
        c = self.acfg
        b, T, fin = feats.shape
        M = b * T
        D = c.hidden_size
        maskf = self._e(M)
        mask32 = self._e(M, dtype=torch.int32)
        _lib.call("ste_mask_i64_to_f32", mask_i64.data_ptr(), maskf.data_ptr(), mask32.data_ptr(), M,
                  _lib.stream_ptr())
        xin = feats.reshape(M, fin)
        a0 = self._e(M, fin, dtype=BF16)
        st0 = self._ln(xin, "audio_encoder.feature_projection.layer_norm", c.layer_norm_eps, yb=a0)
        x = ops.linear(a0, self.s.w("audio_encoder.feature_projection.projection.weight"),
                       self.s.p("audio_encoder.feature_projection.projection.bias"), row_scale=maskf)
        spec = None
        if train and getattr(self.m, "spec_augment", False) and c.mask_time_prob > 0:
            # SpecAugment (w2v:944-988): spans drawn on the host with numpy's global RNG exactly as
            # transformers does, from the host-known clip lengths (TrainStep / to_model_batch pass
            # them); only a caller with nothing but a device mask pays a device->host sync here
            from .specaug import compute_mask_indices, upload_mask
            if lengths is None:
                lengths = mask_i64.sum(-1).tolist() if mask_i64 is not None else [T] * b
            sm = compute_mask_indices((b, T), c.mask_time_prob, c.mask_time_length, lengths, c.mask_time_min_masks)
            spec = upload_mask(sm, self.s.device)
            ops.spec_mask_fwd(x, spec, maskf, self.s.p("audio_encoder.masked_spec_embed"))
        ctx.update(a_b=b, a_T=T, a_maskf=maskf, a_mask32=mask32, a_xin=xin, a_a0=a0, a_st0=st0, a_spec=spec)
        xb = None
        nl = c.num_hidden_layers
        # layerdrop draws (one per layer, in layer order, as transformers does) made up front so
        # each layer knows the next one that runs (its FFN1 LN fuses with this layer's final LN)
        run = [not (train and c.layerdrop > 0 and float(torch.rand([], generator=self.layerdrop_gen)) < c.layerdrop)
               for _ in range(nl)]
        order = [i for i in range(nl) if run[i]]
        layers = [None] * nl
        pre1 = None
        lo = next((i for i in range(nl)
                   if self.s.trainable_layer(f"audio_encoder.encoder.layers.{i}.ffn1_layer_norm.weight")), nl)
        for k, i in enumerate(order):
            last = i == nl - 1
            nxt = order[k + 1] if (self.ln_pair and k + 1 < len(order)) else None
            if i >= lo or (nxt is not None and nxt >= lo):
                self._await_params("late")   # the trainable layers (this one, or the next one's LN)
            x, xb, sv, pre1 = self._conformer_fwd(i, x, b, T, maskf, mask32, train, _site_seed(base_seed, 100 + i),
                                                  last, save, pre1=pre1, nxt=nxt)
            layers[i] = sv if save else None
            if k == 0 and "_text_enqueue" in ctx:   # Engine.forward: the side stream's text forward, now
                ctx.pop("_text_enqueue")()          # that the main stream holds a layer of work
        if xb is None:  # the last layer was dropped (only the last layer writes the split image)
            xb = ops.split_bf16(x, 2, 2)
        ctx["a_layers"] = layers
        ctx["a_hs"] = xb    # [hi | lo] split image of the encoder output (audio pooling scorer)
        return x, xb[:, :D]

    def _conformer_fwd(self, i, x, b, T, maskf, mask32, train, seed, want_bf16, save=True, pre1=None, nxt=None):
        """One Conformer layer.  pre1 = (a1, a1in, stats): this layer's FFN1 LN, already computed
        by the previous layer's fused final-LN pair; nxt = index of the next layer that runs
        (None: none, or no fusion): its FFN1 LN is computed here, fused with this final LN.
        -> (x5, x5 bf16 or None, saved activations, pre1 of layer nxt)."""
        c = self.acfg
        s = self.s
        pre = f"audio_encoder.encoder.layers.{i}."
        M, D, F_ = x.shape[0], c.hidden_size, c.intermediate_size
        H = c.num_attention_heads
        eps = c.layer_norm_eps
        tr = s.trainable_layer(pre + "ffn1_layer_norm.weight")
        sv = {"tr": tr, "seed": seed}
        fp8 = self.fp8

        def lin(xb, wname, bias, count=1, **kw):
            """Forward nn.Linear: bf16 MFMA, or MX-fp8 (fp8_gemm: x block-quantised here unless it
            arrives quantised as an (e4m3, scales) pair, W from ParamStore.wq)."""
            if fp8:
                xq = xb if isinstance(xb, tuple) else ops.mx8_quant(xb)
                return ops.linear_mx8(xq, s.wq(wname, count), bias, **kw)
            return ops.linear(xb, s.fused(wname, count, "w"), bias, **kw)

        def ffn_in(a, wname, bname, z):
            """FFN intermediate (swish): bf16 output, and under fp8_gemm the MX-fp8 copy the output
            GEMM reads; the bf16 copy is kept only for the trained layers' weight gradients."""
            if not fp8:
                h = lin(a, wname, s.p(bname), act=ACT_SWISH, pre_out=z, out_bf16=True)
                return h, h
            q = (self._e(M, F_, dtype=torch.uint8), self._e(M, F_ // 32, dtype=torch.uint8))
            h = self._e(M, F_, dtype=BF16) if (tr and save) else False
            lin(a, wname, s.p(bname), act=ACT_SWISH, pre_out=z, out=h, out_bf16=True, q_out=q)
            return (h if h is not False else None), q

        def ln_in(xin, name, st, **kw):
            """LayerNorm feeding a Linear: bf16 output, or under fp8_gemm the MX-fp8 copy written by
            the LN kernel itself (bf16 kept only for the trained layers' weight gradients)."""
            if not fp8:
                y = self._e(M, D, dtype=BF16)
                sv[st] = self._ln(xin, name, eps, yb=y, **kw)
                return y, y
            y = self._e(M, D, dtype=BF16) if (tr and save) else None
            q = (self._e(M, D, dtype=torch.uint8), self._e(M, D // 32, dtype=torch.uint8))
            sv[st] = self._ln(xin, name, eps, yb=y, q8=q, **kw)
            return y, q

        def ln_in_out(name, tr_, **kw):
            """ln_in's outputs for a LayerNorm computed by a fused pair: (keyword set, a, ain)."""
            if not fp8:
                y = self._e(M, D, dtype=BF16)
                return dict(yb=y, **kw), y, y
            y = self._e(M, D, dtype=BF16) if (tr_ and save) else None
            q = (self._e(M, D, dtype=torch.uint8), self._e(M, D // 32, dtype=torch.uint8))
            return dict(yb=y, q8=q, **kw), y, q

        # -- FFN1 (half-step)
        if pre1 is not None:
            a1, a1in, sv["st1"] = pre1
        else:
            a1, a1in = ln_in(x, pre + "ffn1_layer_norm", "st1")
        z1 = self._e(M, F_, dtype=BF16) if save else None  # swish pre-activation, for backward only
        h1, h1in = ffn_in(a1in, pre + "ffn1.intermediate_dense.weight", pre + "ffn1.intermediate_dense.bias", z1)
        x1 = lin(h1in, pre + "ffn1.output_dense.weight", s.p(pre + "ffn1.output_dense.bias"), alpha=0.5,
                 residual=x)
        # -- relative-key MHSA
        a2, a2in = ln_in(x1, pre + "self_attn_layer_norm", "st2")
        qkv = lin(a2in, pre + "self_attn.linear_q.weight", s.fused(pre + "self_attn.linear_q.bias", 3, "p"), count=3,
                  out_bf16=True)
        o = self._e(M, D, dtype=BF16)
        o_lo = self._e(M, D, dtype=BF16) if save else None   # low half of O for the backward's delta
        lse = self._e(b * H * T)
        ops.attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B=b, T=T, H=H, o=o, lse=lse, key_mask=mask32,
                          rel_E=s.w(pre + "self_attn.distance_embedding.weight"),
                          rel_left=c.left_max_position_embeddings, rel_right=c.right_max_position_embeddings,
                          scale=1.0 / math.sqrt(D // H), o_lo=o_lo)
        x2 = lin(o, pre + "self_attn.linear_out.weight", s.p(pre + "self_attn.linear_out.bias"), residual=x1)
        # -- convolution module
        a3, a3in = ln_in(x2, pre + "conv_module.layer_norm", "st3", row_scale=maskf)
        pw1 = lin(a3in, pre + "conv_module.pointwise_conv1.weight", None, out_bf16=True)
        cv = self._e(M, D, dtype=BF16)
        ops.glu_dwconv_fwd(pw1, s.p(pre + "conv_module.depthwise_conv.weight").view(D, -1), cv, b, T)
        sw, swin = ln_in(cv, pre + "conv_module.depthwise_layer_norm", "st4", act=ACT_SWISH)
        p_conv = c.conformer_conv_dropout if train else 0.0
        x3 = lin(swin, pre + "conv_module.pointwise_conv2.weight", None, residual=x2, drop_p=p_conv,
                 seed=_site_seed(seed, 1))
        # -- FFN2 (half-step) + final LN
        a5, a5in = ln_in(x3, pre + "ffn2_layer_norm", "st5")
        z2 = self._e(M, F_, dtype=BF16) if save else None
        h2, h2in = ffn_in(a5in, pre + "ffn2.intermediate_dense.weight", pre + "ffn2.intermediate_dense.bias", z2)
        x4 = lin(h2in, pre + "ffn2.output_dense.weight", s.p(pre + "ffn2.output_dense.bias"), alpha=0.5,
                 residual=x3)
        x5 = self._e(M, D)
        # the encoder output's bf16 copy as the [hi | lo] split image [M, 2D] (the audio pooling
        # scorer reads it to ~fp32 accuracy; the hi half is the heads' bf16 operand)
        x5s = self._e(M, 2 * D, dtype=BF16) if want_bf16 else None
        x5b = x5s[:, :D] if want_bf16 else None
        x5lo = x5s[:, D:] if want_bf16 else None
        pre_next = None
        if nxt is None:
            sv["st6"] = self._ln(x4, pre + "final_layer_norm", eps, y=x5, yb=x5b, ylo=x5lo)
        else:
            # this final LN fused with layer nxt's FFN1 LN (x5 stays in registers for the second)
            prej = f"audio_encoder.encoder.layers.{nxt}.ffn1_layer_norm"
            trj = s.trainable_layer(f"audio_encoder.encoder.layers.{nxt}.ffn1_layer_norm.weight")
            second, a1j, a1inj = ln_in_out(prej, trj, gamma=s.p(prej + ".weight"), beta=s.p(prej + ".bias"), eps=eps)
            sv["st6"], st1j = ops.layernorm_fwd_pair(
                dict(x=x4, gamma=s.p(pre + "final_layer_norm.weight"), beta=s.p(pre + "final_layer_norm.bias"), eps=eps,
                     y=x5, yb=x5b, ylo=x5lo), second)
            pre_next = (a1j, a1inj, st1j)
        sv.update(x=x, z1=z1, x1=x1, qkv=qkv, o=o, o_lo=o_lo, lse=lse, x2=x2, pw1=pw1, cv=cv, x3=x3, z2=z2, x4=x4, p_conv=p_conv)
        if tr:
            sv.update(a1=a1, h1=h1, a2=a2, a3=a3, sw=sw, a5=a5, h2=h2)
        return x5, x5s, sv, pre_next

    def _ln_bwd_kw(self, x, stats, name, **kw):
        """layernorm_bwd keyword set of the named LN (the pair kernels' argument form)."""
        return dict(x=x, mean=stats[0], rstd=stats[1], gamma=self.s.p(name + ".weight"), beta=self.s.p(name + ".bias"),
                    dgamma=self.s.g(name + ".weight"), dbeta=self.s.g(name + ".bias"), **kw)

    def _conformer_bwd(self, i, sv, dx5, b, T, maskf, mask32, pending=None):
        """Backward of one Conformer layer.  pending: the FFN1-LN backward of the layer above
        (keyword set, dy included), fused here with this layer's final-LN backward; dx5 is then
        None.  -> (d input or None, this layer's own FFN1-LN backward as a pending keyword set
        when fusion is on, else None)."""
        c = self.acfg
        s = self.s
        pre = f"audio_encoder.encoder.layers.{i}."
        M, D, F_ = sv["x4"].shape[0], c.hidden_size, c.intermediate_size
        H = c.num_attention_heads
        tr = sv["tr"]
        _dx = self._dx_mx8 if self.fp8_bwd else self._dx
        # final LN
        dx4 = self._e(M, D)
        dx4b = self._e(M, D, dtype=BF16)
        if pending is None:
            self._ln_bwd(dx5, sv["x4"], sv["st6"], pre + "final_layer_norm", dx=dx4, dxb=dx4b, out_scale=0.5,
                         dsum=s.g(pre + "ffn2.output_dense.bias"))
        else:
            ops.layernorm_bwd_pair(self._ln_bwd_kw(sv["x4"], sv["st6"], pre + "final_layer_norm", dx=dx4, dxb=dx4b,
                                                   out_scale=0.5, dsum=s.g(pre + "ffn2.output_dense.bias")), pending)
        # FFN2
        dz2 = _dx(dx4b, pre + "ffn2.output_dense.weight", act=ACT_SWISH_BWD, z=sv["z2"],
                            out_bf16=True, colsum=s.g(pre + "ffn2.intermediate_dense.bias"))
        if tr:
            self._dw(dx4b, sv["h2"], pre + "ffn2.output_dense.weight")
        # dX GEMMs feeding an LN backward leave bf16 (as under the reference's bf16 autocast, whose
        # Linear backward returns a bf16 input gradient); the residual-stream gradient stays fp32
        da5 = _dx(dz2, pre + "ffn2.intermediate_dense.weight", out_bf16=True)
        if tr:
            self._dw(dz2, sv["a5"], pre + "ffn2.intermediate_dense.weight")
        del dz2
        dx3 = self._e(M, D)
        dx3b = self._e(M, D, dtype=BF16)
        self._ln_bwd(da5, sv["x3"], sv["st5"], pre + "ffn2_layer_norm", dres=dx4, dx=dx3, dxb=dx3b,
                     drop_p=sv["p_conv"], seed=_site_seed(sv["seed"], 1))
        del da5, dx4, dx4b
        # conv module
        dsw = _dx(dx3b, pre + "conv_module.pointwise_conv2.weight", out_bf16=True)
        if tr:
            self._dw(dx3b, sv["sw"], pre + "conv_module.pointwise_conv2.weight")
        dcv = self._e(M, D, dtype=BF16)
        self._ln_bwd(dsw, sv["cv"], sv["st4"], pre + "conv_module.depthwise_layer_norm", act=ACT_SWISH, dxb=dcv)
        del dsw
        dpw1 = self._e(M, 2 * D, dtype=BF16)
        gdw = s.g(pre + "conv_module.depthwise_conv.weight")
        ops.glu_dwconv_bwd(sv["pw1"], s.p(pre + "conv_module.depthwise_conv.weight").view(D, -1), dcv, dpw1,
                           None if gdw is None else gdw.view(D, -1), b, T)
        del dcv
        da3 = _dx(dpw1, pre + "conv_module.pointwise_conv1.weight", out_bf16=True)
        if tr:
            self._dw(dpw1, sv["a3"], pre + "conv_module.pointwise_conv1.weight")
        del dpw1
        dx2 = self._e(M, D)
        dx2b = self._e(M, D, dtype=BF16)
        self._ln_bwd(da3, sv["x2"], sv["st3"], pre + "conv_module.layer_norm", row_scale=maskf, dres=dx3, dx=dx2,
                     dxb=dx2b, dsum=s.g(pre + "self_attn.linear_out.bias"))
        del da3, dx3, dx3b
        # attention
        do = _dx(dx2b, pre + "self_attn.linear_out.weight", out_bf16=True)
        if tr:
            self._dw(dx2b, sv["o"], pre + "self_attn.linear_out.weight")
        del dx2b
        qkv = sv["qkv"]
        dqkv = self._e(M, 3 * D, dtype=BF16)
        delta = self._e(b * H * T)
        gE = s.g(pre + "self_attn.distance_embedding.weight")
        gwork = self._e(b * H * T * 80) if gE is not None else None
        ops.attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], sv["o"], sv["lse"], do, dqkv[:, :D],
                          dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=b, T=T, H=H, delta=delta, key_mask=mask32,
                          rel_E=s.w(pre + "self_attn.distance_embedding.weight"),
                          rel_left=c.left_max_position_embeddings, rel_right=c.right_max_position_embeddings,
                          scale=1.0 / math.sqrt(D // H), dE=gE, gwork=gwork, o_lo=sv["o_lo"])
        del do, delta, gwork
        da2 = _dx(dqkv, pre + "self_attn.linear_q.weight", 3, out_bf16=True)
        if tr:
            self._dw(dqkv, sv["a2"], pre + "self_attn.linear_q.weight", fused=3)
            self._db(dqkv, pre + "self_attn.linear_q.bias", fused=3)
        del dqkv
        dx1 = self._e(M, D)
        dx1b = self._e(M, D, dtype=BF16)
        self._ln_bwd(da2, sv["x1"], sv["st2"], pre + "self_attn_layer_norm", dres=dx2, dx=dx1, dxb=dx1b,
                     out_scale=0.5, dsum=s.g(pre + "ffn1.output_dense.bias"))
        del da2, dx2
        # FFN1
        dz1 = _dx(dx1b, pre + "ffn1.output_dense.weight", act=ACT_SWISH_BWD, z=sv["z1"],
                            out_bf16=True, colsum=s.g(pre + "ffn1.intermediate_dense.bias"))
        if tr:
            self._dw(dx1b, sv["h1"], pre + "ffn1.output_dense.weight")
        da1 = _dx(dz1, pre + "ffn1.intermediate_dense.weight", out_bf16=True)
        if tr:
            self._dw(dz1, sv["a1"], pre + "ffn1.intermediate_dense.weight")
        del dz1
        kw = self._ln_bwd_kw(sv["x"], sv["st1"], pre + "ffn1_layer_norm", dy=da1, dres=dx1)
        if self.ln_pair:
            return None, kw
        dx0 = self._e(M, D)
        ops.layernorm_bwd(dx=dx0, **kw)
        return dx0, None

    def _flush_ln(self, pending):
        """Run a pending FFN1-LN backward on its own -> its input gradient."""
        dx0 = self._e(*pending["x"].shape)
        ops.layernorm_bwd(dx=dx0, **pending)
        return dx0

    def audio_backward(self, dh, ctx, layers_done=None):
        """layers_done() is called once every trainable Conformer layer's gradients are final
        (after the lowest trainable layer), so their all-reduce overlaps the frozen layers."""
        if self.raw_audio:
            from . import wav2vec2
            return wav2vec2.backward(self, dh, ctx, layers_done)
        c = self.acfg
        b, T = ctx["a_b"], ctx["a_T"]
        maskf, mask32 = ctx["a_maskf"], ctx["a_mask32"]
        lo = next((i for i in range(c.num_hidden_layers)
                   if self.s.trainable_layer(f"audio_encoder.encoder.layers.{i}.ffn1_layer_norm.weight")), None)
        dx = dh
        pending = None
        for i in reversed(range(c.num_hidden_layers)):
            sv = ctx["a_layers"][i]
            if sv is not None:
                dx, pending = self._conformer_bwd(i, sv, dx, b, T, maskf, mask32, pending)
                ctx["a_layers"][i] = None
            if i == lo:
                # the lowest trainable layer's FFN1-LN gradients must be final before its sync;
                # flushed on every micro-batch (not only the one that syncs), so a micro-batch's
                # gradients never depend on its place in the accumulation window (the single and
                # pair LN kernels agree only to fp32 rounding)
                if pending is not None:
                    dx, pending = self._flush_ln(pending), None
                if layers_done is not None:
                    layers_done()
        if pending is not None:
            dx = self._flush_ln(pending)
        s = self.s
        if ctx.get("a_spec") is not None:  # SpecAugment rows: gradient to masked_spec_embed, not the projection
            ops.spec_mask_bwd(dx, ctx["a_spec"], maskf, s.g("audio_encoder.masked_spec_embed"))
        # feature projection: x = mask * (LN(feats) W^T + b)
        gW = s.g("audio_encoder.feature_projection.projection.weight")
        if gW is not None:
            M = dx.shape[0]
            # the forward's masked_fill (row_scale) multiplies dY row-wise
            _lib.call("ste_scale_rows", dx.data_ptr(), maskf.data_ptr(), M, c.hidden_size, dx.stride(0),
                      _lib.stream_ptr())
            dxb = ops.cast_bf16(dx, self._e(M, c.hidden_size, dtype=BF16))
            self._dw(dxb, ctx["a_a0"], "audio_encoder.feature_projection.projection.weight")
            self._db(dxb, "audio_encoder.feature_projection.projection.bias")
            if s.g("audio_encoder.feature_projection.layer_norm.weight") is not None:
                da0 = ops.linear_dx(dxb, s.w("audio_encoder.feature_projection.projection.weight"))
                self._ln_bwd(da0, ctx["a_xin"], ctx["a_st0"], "audio_encoder.feature_projection.layer_norm")

    # ================================================================= text
    def text_forward(self, ids, mask_i64, train, base_seed, ctx, save=True):
        self._await_params("text")
        c = self.tcfg
        s = self.s
        nb, L = ids.shape
        M, D = nb * L, c.hidden_size
        mask32 = self._e(M, dtype=torch.int32)
        _lib.call("ste_mask_i64_to_f32", mask_i64.data_ptr(), None, mask32.data_ptr(), M, _lib.stream_ptr())
        emb = self._e(M, D)
        pos_ids = self._e(M, dtype=torch.int32)
        ops.text_embed_fwd(ids, c.pad_token_id, s.p("text_encoder.embeddings.word_embeddings.weight"),
                           s.p("text_encoder.embeddings.position_embeddings.weight"),
                           s.p("text_encoder.embeddings.token_type_embeddings.weight"), emb, pos_ids)
        hp = c.hidden_dropout_prob if train else 0.0
        ap = c.attention_probs_dropout_prob if train else 0.0
        x = self._e(M, D)
        if self.precise_text:   # xb: the [hi | lo] split image [M, 2D] the precise forward's GEMMs read
            xb = self._e(M, 2 * D, dtype=BF16)
            st = self._ln(emb, "text_encoder.embeddings.LayerNorm", c.layer_norm_eps, y=x, yb=xb[:, :D], ylo=xb[:, D:],
                          drop_p=hp, seed=_site_seed(base_seed, 1))
        else:
            xb = self._e(M, D, dtype=BF16)
            st = self._ln(emb, "text_encoder.embeddings.LayerNorm", c.layer_norm_eps, y=x, yb=xb, drop_p=hp,
                          seed=_site_seed(base_seed, 1))
        ctx.update(t_nb=nb, t_L=L, t_mask32=mask32, t_ids=ids, t_emb=emb, t_pos=pos_ids, t_st=st, t_hp=hp, t_ap=ap,
                   t_seed=base_seed)
        layers = []
        for i in range(c.num_hidden_layers):
            x, xb, sv = self._xlmr_fwd(i, x, xb, nb, L, mask32, hp, ap, _site_seed(base_seed, 10 + i), save)
            layers.append(sv if save else None)
        ctx["t_layers"] = layers
        return x, (xb[:, :D] if self.precise_text else xb)

    def _xlmr_fwd(self, i, x, xb, nb, L, mask32, hp, ap, seed, save=True):
        if self.precise_text:
            return self._postln_fwd_x2(self.tcfg, XLMR_NAMES, i, x, xb, nb, L, mask32, hp, ap, seed, save)
        return self._postln_fwd(self.tcfg, XLMR_NAMES, i, x, xb, nb, L, mask32, hp, ap, seed, save)

    def _xlmr_bwd(self, i, sv, dx2, nb, L, mask32, hp, ap):
        if self.precise_text and self.precise_text_bwd:
            return self._postln_bwd_x2(self.tcfg, XLMR_NAMES, i, sv, dx2, nb, L, mask32, hp, ap)
        return self._postln_bwd(self.tcfg, XLMR_NAMES, i, sv, dx2, nb, L, mask32, hp, ap)

    def _postln_fwd(self, c, nm, i, x, xb, nb, L, mask32, hp, ap, seed, save=True, act_p=0.0):
        """One post-LN transformer layer: XLM-R (tf:…xlm_roberta…:186-398) and wav2vec2
        (tf:models/wav2vec2/modeling_wav2vec2.py:466-608) share the math
        LN(x + drop(O(attn(QKV x)))) -> LN(x1 + drop(W2·drop_act(gelu(W1 x1)))); `nm` maps the
        parameter names (XLMR_NAMES / W2V2_NAMES).  Both run on SDPA in the reference's
        transformers, so a query whose keys are all masked gets zero attention (zero_masked_rows)."""
        s = self.s
        pre = nm["layer"].format(i=i)
        M, D, F_ = x.shape[0], c.hidden_size, c.intermediate_size
        H = c.num_attention_heads
        eps = c.layer_norm_eps
        tr = s.trainable_layer(pre + nm["q"] + ".weight")
        sv = {"tr": tr, "seed": seed, "act_p": act_p}
        qkv = ops.linear(xb, s.fused(pre + nm["q"] + ".weight", 3, "w"), s.fused(pre + nm["q"] + ".bias", 3, "p"),
                         out_bf16=True)
        o = self._e(M, D, dtype=BF16)
        o_lo = self._e(M, D, dtype=BF16) if save else None
        lse = self._e(nb * H * L)
        ops.attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B=nb, T=L, H=H, o=o, lse=lse,
                          key_mask=mask32, scale=1.0 / math.sqrt(D // H), drop_p=ap, seed=_site_seed(seed, 1),
                          o_lo=o_lo, zero_masked_rows=True)
        y1 = ops.linear(o, s.w(pre + nm["o"] + ".weight"), s.p(pre + nm["o"] + ".bias"),
                        residual=x, drop_p=hp, seed=_site_seed(seed, 2))
        x1 = self._e(M, D)
        x1b = self._e(M, D, dtype=BF16)
        sv["st1"] = self._ln(y1, pre + nm["ln1"], eps, y=x1, yb=x1b)
        zt = self._e(M, F_, dtype=BF16) if save else None  # GELU pre-activation, for backward only
        h = ops.linear(x1b, s.w(pre + nm["fi"] + ".weight"), s.p(pre + nm["fi"] + ".bias"),
                       act=ACT_GELU, pre_out=zt, out_bf16=True, drop_p=act_p, seed=_site_seed(seed, 4))
        y2 = ops.linear(h, s.w(pre + nm["fo"] + ".weight"), s.p(pre + nm["fo"] + ".bias"), residual=x1, drop_p=hp,
                        seed=_site_seed(seed, 3))
        x2 = self._e(M, D)
        x2b = self._e(M, D, dtype=BF16)
        sv["st2"] = self._ln(y2, pre + nm["ln2"], eps, y=x2, yb=x2b)
        sv.update(qkv=qkv, o=o, o_lo=o_lo, lse=lse, y1=y1, zt=zt, y2=y2)
        if tr:
            sv.update(xb=xb, x1b=x1b, h=h)
        return x2, x2b, sv

    def _postln_fwd_x2(self, c, nm, i, x, xs, nb, L, mask32, hp, ap, seed, save=True, act_p=0.0):
        """_postln_fwd with the activations to ~fp32 accuracy.  Every Linear reads its input as the
        [hi | lo] split image ([M, 2·in] bf16, hi = bf16(v), lo = bf16(v − hi)) against [W | W]
        (ParamStore.w2): one bf16 MFMA GEMM over K' = 2·in computes the fp32 activations times the
        bf16 weight — the weight's rounding is common to both transcripts, the activations' is what
        the loss gradient differences.  The producers write the split images themselves (LayerNorm
        hi + lo outputs, the FFN GEMM's bf16 output + low-half copy, the fp32 attention kernel's O +
        O_lo), so no extra pass runs.  It saves what _postln_bwd reads, in the same dtypes (bf16
        q/k/v, O + O_lo, pre-activation, the bf16 hi halves as the trained layers' dW operands), so
        the backward is unchanged.  xs / the returned x2s: split images of x / x2."""
        s = self.s
        pre = nm["layer"].format(i=i)
        M, D, F_ = x.shape[0], c.hidden_size, c.intermediate_size
        H = c.num_attention_heads
        eps = c.layer_norm_eps
        tr = s.trainable_layer(pre + nm["q"] + ".weight")
        sv = {"tr": tr, "seed": seed, "act_p": act_p}
        qkvb = self._e(M, 3 * D, dtype=BF16) if (save and not self.precise_text_bwd) else None
        qkv = ops.linear(xs, s.w2(pre + nm["q"] + ".weight", 3), s.fused(pre + nm["q"] + ".bias", 3, "p"),
                         out_bf16_copy=qkvb)
        os_ = self._e(M, 2 * D, dtype=BF16)   # [O | O_lo]: the O-proj input and the backward's O, O_lo
        lse = self._e(nb * H * L)
        ops.attention_fwd_f32(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B=nb, T=L, H=H, o32=None, lse=lse,
                              o=os_[:, :D], o_lo=os_[:, D:], key_mask=mask32, scale=1.0 / math.sqrt(D // H),
                              drop_p=ap, seed=_site_seed(seed, 1), zero_masked_rows=True)
        y1 = ops.linear(os_, s.w2(pre + nm["o"] + ".weight"), s.p(pre + nm["o"] + ".bias"), residual=x, drop_p=hp,
                        seed=_site_seed(seed, 2))
        x1 = self._e(M, D)
        x1s = self._e(M, 2 * D, dtype=BF16)
        sv["st1"] = self._ln(y1, pre + nm["ln1"], eps, y=x1, yb=x1s[:, :D], ylo=x1s[:, D:])
        zt = self._e(M, F_, dtype=BF16) if save else None  # GELU pre-activation, for backward only
        hs_ = self._e(M, 2 * F_, dtype=BF16)              # [h | h_lo]
        ops.linear(x1s, s.w2(pre + nm["fi"] + ".weight"), s.p(pre + nm["fi"] + ".bias"), act=ACT_GELU, pre_out=zt,
                   drop_p=act_p, seed=_site_seed(seed, 4), out=hs_[:, :F_], out_bf16_copy=hs_[:, F_:], copy_lo=True)
        y2 = ops.linear(hs_, s.w2(pre + nm["fo"] + ".weight"), s.p(pre + nm["fo"] + ".bias"), residual=x1, drop_p=hp,
                        seed=_site_seed(seed, 3), ws=self.ws)   # 96 output tiles: few-tile split-K
        x2 = self._e(M, D)
        x2s = self._e(M, 2 * D, dtype=BF16)
        sv["st2"] = self._ln(y2, pre + nm["ln2"], eps, y=x2, yb=x2s[:, :D], ylo=x2s[:, D:])
        if save and self.precise_text_bwd:   # what _postln_bwd_x2 reads: fp32 q/k/v, the O image, LSE,
            sv.update(qkv=qkv, os=os_, lse=lse, y1=y1, zt=zt, y2=y2)   # LN inputs, GELU input
            if tr:                             # the trained layers' dW operands as [hi | lo] images
                sv.update(xs=xs, x1s=x1s, hs=hs_)
        elif save:                             # what _postln_bwd reads: bf16 copies, the hi halves
            sv.update(qkv=qkvb, o=os_[:, :D], o_lo=os_[:, D:], lse=lse, y1=y1, zt=zt, y2=y2)
            if tr:
                sv.update(xb=xs[:, :D], x1b=x1s[:, :D], h=hs_[:, :F_])
        return x2, x2s, sv

    def _dw2(self, dys, xs, wname, fused=1):
        """dW += dYᵀ·X of a text Linear from [hi | lo] split images of both operands, to ~fp32:
        dY_hiᵀX_hi + dY_loᵀX_hi + dY_hiᵀX_lo (the lo·lo term is below fp32 rounding), three
        k-major GEMMs accumulating into the flat gradient buffer."""
        g = self.s.fused(wname, fused, "g")
        if g is None:
            return
        g2 = g.view(g.shape[0], -1)
        n, k = dys.shape[1] // 2, xs.shape[1] // 2
        for dy, x in ((dys[:, :n], xs[:, :k]), (dys[:, n:], xs[:, :k]), (dys[:, :n], xs[:, k:])):
            ops.linear_dw(dy, x, out=g2, beta=1.0, ws=self.ws)

    def _postln_bwd_x2(self, c, nm, i, sv, dx2, nb, L, mask32, hp, ap):
        """Backward of _postln_fwd_x2 to ~fp32 accuracy.  The loss gradient reaching the text
        encoder is the difference of the clean and the corrupted transcript's nearly equal
        backward passes (80 % shared tokens), which every text weight and bias gradient sums over
        rows: bf16 rounding of the backward's dY operands, of dO and of the attention backward
        reappeared there as 1.2-2 % errors (tests/precision_probe_text.py).  So every dX GEMM reads
        its dY as a [hi | lo] split image against [Wᵀ | Wᵀ] (ParamStore.wt2, K' = 2·out), the
        GELU-backward GEMM writes its output as a split image, the O-proj input gradient dO stays
        fp32, the attention backward runs in fp32 on the fp32 q/k/v (ste_attention_bwd_f32), the
        bias gradients are column sums of fp32 values, and the trained layers' dW read split
        images of both operands (_dw2)."""
        s = self.s
        pre = nm["layer"].format(i=i)
        M, D, F_ = dx2.shape[0], c.hidden_size, c.intermediate_size
        H = c.num_attention_heads
        tr = sv["tr"]
        seed = sv["seed"]
        dy2 = self._e(M, D)
        self._ln_bwd(dx2, sv["y2"], sv["st2"], pre + nm["ln2"], dx=dy2, drop_p=hp, seed=_site_seed(seed, 3),
                     dsum=s.g(pre + nm["fo"] + ".bias"))
        dy2s = ops.split_bf16(dy2, 2, 2)
        dzs = self._e(M, 2 * F_, dtype=BF16)     # [dz | dz_lo]
        ops.linear(dy2s, s.wt2(pre + nm["fo"] + ".weight"), act=ACT_GELU_BWD, z=sv["zt"], out=dzs[:, :F_],
                   out_bf16_copy=dzs[:, F_:], copy_lo=True, colsum=s.g(pre + nm["fi"] + ".bias"),
                   drop_p=sv["act_p"], seed=_site_seed(seed, 4), ws=self.ws)
        if tr:
            self._dw2(dy2s, sv["hs"], pre + nm["fo"] + ".weight")
        del dy2s
        dx1 = ops.linear(dzs, s.wt2(pre + nm["fi"] + ".weight"), residual=dy2, ws=self.ws)
        if tr:
            self._dw2(dzs, sv["x1s"], pre + nm["fi"] + ".weight")
        del dzs, dy2
        dy1 = self._e(M, D)
        self._ln_bwd(dx1, sv["y1"], sv["st1"], pre + nm["ln1"], dx=dy1, drop_p=hp, seed=_site_seed(seed, 2),
                     dsum=s.g(pre + nm["o"] + ".bias"))
        del dx1
        dy1s = ops.split_bf16(dy1, 2, 2)
        do = ops.linear(dy1s, s.wt2(pre + nm["o"] + ".weight"), ws=self.ws)   # fp32 dO
        if tr:
            self._dw2(dy1s, sv["os"], pre + nm["o"] + ".weight")
        del dy1s
        qkv, os_ = sv["qkv"], sv["os"]
        dqkv = self._e(M, 3 * D)
        ops.attention_bwd_f32(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], os_[:, :D], os_[:, D:], sv["lse"], do,
                              dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=nb, T=L, H=H, key_mask=mask32,
                              scale=1.0 / math.sqrt(D // H), drop_p=ap, seed=_site_seed(seed, 1),
                              zero_masked_rows=True)
        del do
        if tr:
            self._db(dqkv, pre + nm["q"] + ".bias", fused=3)
        dqkvs = ops.split_bf16(dqkv, 2, 2)
        del dqkv
        dx0 = ops.linear(dqkvs, s.wt2(pre + nm["q"] + ".weight", 3), residual=dy1, ws=self.ws)
        if tr:
            self._dw2(dqkvs, sv["xs"], pre + nm["q"] + ".weight", fused=3)
        return dx0

    def _postln_bwd(self, c, nm, i, sv, dx2, nb, L, mask32, hp, ap):
        s = self.s
        pre = nm["layer"].format(i=i)
        M, D = dx2.shape[0], c.hidden_size
        H = c.num_attention_heads
        tr = sv["tr"]
        seed = sv["seed"]
        dy2 = self._e(M, D)
        dy2b = self._e(M, D, dtype=BF16)
        self._ln_bwd(dx2, sv["y2"], sv["st2"], pre + nm["ln2"], dx=dy2, dxb=dy2b, drop_p=hp,
                     seed=_site_seed(seed, 3), dsum=s.g(pre + nm["fo"] + ".bias"))
        dzt = self._dx(dy2b, pre + nm["fo"] + ".weight", act=ACT_GELU_BWD, z=sv["zt"], out_bf16=True,
                       colsum=s.g(pre + nm["fi"] + ".bias"), drop_p=sv["act_p"], seed=_site_seed(seed, 4))
        if tr:
            self._dw(dy2b, sv["h"], pre + nm["fo"] + ".weight")
        del dy2b
        dx1 = self._dx(dzt, pre + nm["fi"] + ".weight", residual=dy2)
        if tr:
            self._dw(dzt, sv["x1b"], pre + nm["fi"] + ".weight")
        del dzt, dy2
        dy1 = self._e(M, D)
        dy1b = self._e(M, D, dtype=BF16)
        self._ln_bwd(dx1, sv["y1"], sv["st1"], pre + nm["ln1"], dx=dy1, dxb=dy1b, drop_p=hp,
                     seed=_site_seed(seed, 2), dsum=s.g(pre + nm["o"] + ".bias"))
        del dx1
        do = self._dx(dy1b, pre + nm["o"] + ".weight", out_bf16=True)
        if tr:
            self._dw(dy1b, sv["o"], pre + nm["o"] + ".weight")
        del dy1b
        qkv = sv["qkv"]
        dqkv = self._e(M, 3 * D, dtype=BF16)
        delta = self._e(nb * H * L)
        ops.attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], sv["o"], sv["lse"], do, dqkv[:, :D],
                          dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=nb, T=L, H=H, delta=delta, key_mask=mask32,
                          scale=1.0 / math.sqrt(D // H), drop_p=ap, seed=_site_seed(seed, 1), o_lo=sv["o_lo"])
        del do, delta
        dx0 = self._dx(dqkv, pre + nm["q"] + ".weight", 3, residual=dy1)
        if tr:
            self._dw(dqkv, sv["xb"], pre + nm["q"] + ".weight", fused=3)
            self._db(dqkv, pre + nm["q"] + ".bias", fused=3)
        return dx0

    def _preln_fwd(self, c, nm, i, x, nb, L, mask32, hp, ap, seed, save=True, act_p=0.0):
        """One pre-LN transformer layer (Wav2Vec2EncoderLayerStableLayerNorm, tf:models/wav2vec2/
        modeling_wav2vec2.py:611-654): x1 = x + drop(O(attn(QKV·LN1(x)))),
        x2 = x1 + drop(W2·drop_act(gelu(W1·LN2(x1)))).  The residual stream x stays fp32; the
        LayerNorms write the bf16 GEMM operands.  Same kernels, dropout-site seeds and saved-tensor
        conventions as _postln_fwd."""
        s = self.s
        pre = nm["layer"].format(i=i)
        M, D, F_ = x.shape[0], c.hidden_size, c.intermediate_size
        H = c.num_attention_heads
        eps = c.layer_norm_eps
        tr = s.trainable_layer(pre + nm["q"] + ".weight")
        sv = {"tr": tr, "seed": seed, "act_p": act_p}
        a1 = self._e(M, D, dtype=BF16)
        sv["st1"] = self._ln(x, pre + nm["ln1"], eps, yb=a1)
        qkv = ops.linear(a1, s.fused(pre + nm["q"] + ".weight", 3, "w"), s.fused(pre + nm["q"] + ".bias", 3, "p"),
                         out_bf16=True)
        o = self._e(M, D, dtype=BF16)
        o_lo = self._e(M, D, dtype=BF16) if save else None
        lse = self._e(nb * H * L)
        ops.attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B=nb, T=L, H=H, o=o, lse=lse,
                          key_mask=mask32, scale=1.0 / math.sqrt(D // H), drop_p=ap, seed=_site_seed(seed, 1),
                          o_lo=o_lo, zero_masked_rows=True)
        x1 = ops.linear(o, s.w(pre + nm["o"] + ".weight"), s.p(pre + nm["o"] + ".bias"),
                        residual=x, drop_p=hp, seed=_site_seed(seed, 2))
        a2 = self._e(M, D, dtype=BF16)
        sv["st2"] = self._ln(x1, pre + nm["ln2"], eps, yb=a2)
        zt = self._e(M, F_, dtype=BF16) if save else None  # GELU pre-activation, for backward only
        h = ops.linear(a2, s.w(pre + nm["fi"] + ".weight"), s.p(pre + nm["fi"] + ".bias"),
                       act=ACT_GELU, pre_out=zt, out_bf16=True, drop_p=act_p, seed=_site_seed(seed, 4))
        x2 = ops.linear(h, s.w(pre + nm["fo"] + ".weight"), s.p(pre + nm["fo"] + ".bias"), residual=x1, drop_p=hp,
                        seed=_site_seed(seed, 3))
        sv.update(qkv=qkv, o=o, o_lo=o_lo, lse=lse, x=x, x1=x1, zt=zt)
        if tr:
            sv.update(a1=a1, a2=a2, h=h)
        return x2, sv

    def _preln_out_grad(self, c, nm, i, sv, hp):
        """_ln_bwd keywords with which the LayerNorm backward ABOVE layer i (the next layer's LN1, or
        the encoder's trailing LayerNorm) also emits what _preln_bwd(i) starts from: the bf16 copy of
        the residual-stream gradient through the FFN output dropout, and its column sum, the
        output_dense bias gradient."""
        pre = nm["layer"].format(i=i)
        M, D = sv["x"].shape
        return dict(dxb=self._e(M, D, dtype=BF16), drop_p=hp, seed=_site_seed(sv["seed"], 3),
                    dsum=self.s.g(pre + nm["fo"] + ".bias"))

    def _preln_bwd(self, c, nm, i, sv, dx2, dx2b, nb, L, mask32, hp, ap, below=None):
        """Backward of _preln_fwd.  dx2 fp32: gradient of the layer's output; dx2b: its bf16 copy
        through the FFN output dropout (_preln_out_grad, written by the LayerNorm backward above).
        below: the _preln_out_grad keywords of the next layer down that ran, so that this layer's
        LN1 backward writes that layer's dx2b.  -> d input (fp32; below["dxb"] is filled)."""
        s = self.s
        pre = nm["layer"].format(i=i)
        M, D = dx2.shape[0], c.hidden_size
        H = c.num_attention_heads
        tr = sv["tr"]
        seed = sv["seed"]
        dzt = self._dx(dx2b, pre + nm["fo"] + ".weight", act=ACT_GELU_BWD, z=sv["zt"], out_bf16=True,
                       colsum=s.g(pre + nm["fi"] + ".bias"), drop_p=sv["act_p"], seed=_site_seed(seed, 4))
        if tr:
            self._dw(dx2b, sv["h"], pre + nm["fo"] + ".weight")
        # dX GEMMs feeding an LN backward leave bf16 (as in _conformer_bwd); the stream stays fp32
        da2 = self._dx(dzt, pre + nm["fi"] + ".weight", out_bf16=True)
        if tr:
            self._dw(dzt, sv["a2"], pre + nm["fi"] + ".weight")
        del dzt
        dx1 = self._e(M, D)
        dx1b = self._e(M, D, dtype=BF16)
        self._ln_bwd(da2, sv["x1"], sv["st2"], pre + nm["ln2"], dres=dx2, dx=dx1, dxb=dx1b, drop_p=hp,
                     seed=_site_seed(seed, 2), dsum=s.g(pre + nm["o"] + ".bias"))
        del da2
        do = self._dx(dx1b, pre + nm["o"] + ".weight", out_bf16=True)
        if tr:
            self._dw(dx1b, sv["o"], pre + nm["o"] + ".weight")
        del dx1b
        qkv = sv["qkv"]
        dqkv = self._e(M, 3 * D, dtype=BF16)
        delta = self._e(nb * H * L)
        ops.attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], sv["o"], sv["lse"], do, dqkv[:, :D],
                          dqkv[:, D:2 * D], dqkv[:, 2 * D:], B=nb, T=L, H=H, delta=delta, key_mask=mask32,
                          scale=1.0 / math.sqrt(D // H), drop_p=ap, seed=_site_seed(seed, 1), o_lo=sv["o_lo"])
        del do, delta
        da1 = self._dx(dqkv, pre + nm["q"] + ".weight", 3, out_bf16=True)
        if tr:
            self._dw(dqkv, sv["a1"], pre + nm["q"] + ".weight", fused=3)
            self._db(dqkv, pre + nm["q"] + ".bias", fused=3)
        del dqkv
        dx0 = self._e(M, D)
        self._ln_bwd(da1, sv["x"], sv["st1"], pre + nm["ln1"], dres=dx1, dx=dx0, **(below or {}))
        return dx0

    def text_backward(self, dh, ctx, layers_done=None):
        """layers_done() is called once every trainable XLM-R layer's gradients are final (after
        the lowest trainable layer), so their all-reduce overlaps the frozen text layers' passes."""
        c = self.tcfg
        s = self.s
        nb, L = ctx["t_nb"], ctx["t_L"]
        lo = next((i for i in range(c.num_hidden_layers)
                   if s.trainable_layer(XLMR_NAMES["layer"].format(i=i) + XLMR_NAMES["q"] + ".weight")), None)
        if lo is None and layers_done is not None:
            layers_done()
        dx = dh
        for i in reversed(range(c.num_hidden_layers)):
            dx = self._xlmr_bwd(i, ctx["t_layers"][i], dx, nb, L, ctx["t_mask32"], ctx["t_hp"], ctx["t_ap"])
            ctx["t_layers"][i] = None
            if i == lo and layers_done is not None:
                layers_done()
        gw = s.g("text_encoder.embeddings.word_embeddings.weight")
        gp = s.g("text_encoder.embeddings.position_embeddings.weight")
        gt = s.g("text_encoder.embeddings.token_type_embeddings.weight")
        ln_needed = any(g is not None for g in (gw, gp, gt, s.g("text_encoder.embeddings.LayerNorm.weight")))
        if not ln_needed:
            return
        demb = self._e(dx.shape[0], c.hidden_size)
        self._ln_bwd(dx, ctx["t_emb"], ctx["t_st"], "text_encoder.embeddings.LayerNorm", dx=demb,
                     in_drop_p=ctx["t_hp"], in_seed=_site_seed(ctx["t_seed"], 1))
        if gw is not None or gp is not None or gt is not None:
            ops.text_embed_bwd(ctx["t_ids"], ctx["t_pos"], demb, c.pad_token_id, gw, gp, gt)

    # ================================================================ heads
    # The heads run in fp32 (ste_gemm_f32, the fp32 pooling kernels) wherever the loss gradient
    # differences their values: the text pooling, both projections, the cross-modal queries and
    # outputs, and the fusion Linears.  The loss gradient w.r.t. the audio embedding is
    # ds·(t_neg − t_pos) and every head gradient is a sum of nearly cancelling terms of the
    # positive and the corrupted transcript (80 % shared tokens), so 2^-9 bf16 operand rounding
    # there reappeared as 4–18 % gradient errors.  These GEMMs have M = batch rows
    # (text pooling scorer: 2·b·L), so fp32 costs little.  The large audio-side GEMMs
    # (audio_seq_to_projection, the text→audio K/V, the audio pooling scorer) stay bf16: the two
    # transcripts attend to the same K/V, and the cross-attention backward sums both query sets'
    # dK/dV in fp32 before its single rounding.
    def _w32(self, name):
        """fp32 master weight as a 2-D [out, in] matrix (the ste_gemm_f32 B operand)."""
        w = self.s.p(name)
        return w.view(w.shape[0], -1)

    def _dw32(self, dy, x, wname):
        """dW[N,K] += dyᵀ·x in fp32 (ste_gemm_f32) into the flat gradient buffer."""
        g = self.s.g(wname)
        if g is not None:
            ops.linear_dw(dy, x, out=g.view(g.shape[0], -1), beta=1.0, ws=self.ws)

    def _db32(self, dy, bname):
        g = self.s.g(bname)
        if g is not None:
            ops.colsum(dy, g)

    def _proj_fwd(self, name, x, rows, train, seed, sv):
        """EnhancedProjection ref:66-99 in fp32: x [rows, H] -> [rows, P]."""
        s = self.s
        p_drop = self.m.dropout if train else 0.0
        zp = self._e(rows, s.slots[name + ".projection.0.weight"].shape[0])
        h = ops.linear(x, self._w32(name + ".projection.0.weight"), s.p(name + ".projection.0.bias"), act=ACT_GELU,
                       pre_out=zp, drop_p=p_drop, seed=seed)
        y = ops.linear(h, self._w32(name + ".projection.3.weight"), s.p(name + ".projection.3.bias"))
        out = self._e(rows, y.shape[1])
        st = self._ln(y, name + ".projection.4", 1e-5, y=out)
        sv.update(x=x, zp=zp, h=h, y=y, st=st, p=p_drop, seed=seed)
        return out

    def _proj_bwd(self, name, sv, dout, dx_out):
        """writes d(input) into dx_out (fp32, +=)."""
        s = self.s
        dy = self._e(*dout.shape)
        self._ln_bwd(dout, sv["y"], sv["st"], name + ".projection.4", dx=dy, dsum=s.g(name + ".projection.3.bias"))
        dz = ops.linear_dx(dy, self._w32(name + ".projection.3.weight"), act=ACT_GELU_BWD, z=sv["zp"], drop_p=sv["p"],
                           seed=sv["seed"], colsum=s.g(name + ".projection.0.bias"))
        self._dw32(dy, sv["h"], name + ".projection.3.weight")
        ops.linear_dx(dz, self._w32(name + ".projection.0.weight"), out=dx_out, beta=1.0)
        self._dw32(dz, sv["x"], name + ".projection.0.weight")

    def _pool_fwd(self, name, h, hb, mask32, nb, L, sv, hs=None):
        """AttentivePooling ref:171-211 -> pooled fp32 [nb, H] on the fp32 states h: the text
        scorer on ste_gemm_f32; the audio scorer (31,936 rows at c2) on the bf16 MFMA over the
        encoder output's [hi | lo] split image hs against [W | W] (~fp32 activations: its gradient
        Σ_l dz_l ⊗ h_l cancels over frames sharing a large common component).  Without hs (the
        wav2vec2 front end) the audio side runs on the bf16 copy hb.  With
        use_attentive_pooling=False: text CLS row (ref:578-580) / audio masked mean (ref:621-636)
        of the fp32 states."""
        s = self.s
        H = h.shape[1]
        w = self._e(nb * L)
        pooled = self._e(nb, H)
        if not self.m.use_attentive_pooling:
            ops.mean_pool_fwd(h, mask32, nb, L, name == "text_pooling", w, pooled)
            sv.update(w=w)
            return pooled
        f32 = name == "text_pooling" or hb is None or hs is not None
        w2, b2 = s.p(name + ".attention.2.weight").view(-1), s.p(name + ".attention.2.bias")
        if f32:
            if hs is not None:
                t = ops.linear(hs, s.w2(name + ".attention.0.weight"), s.p(name + ".attention.0.bias"), act=ACT_TANH)
            else:
                t = ops.linear(h, self._w32(name + ".attention.0.weight"), s.p(name + ".attention.0.bias"),
                               act=ACT_TANH)
            ops.attn_pool_fwd_f32(t, w2, b2, h, mask32, nb, L, w, pooled)
            sv.update(hs=hs)
        else:
            t = ops.linear(hb, s.w(name + ".attention.0.weight"), s.p(name + ".attention.0.bias"), act=ACT_TANH,
                           out_bf16=True)
            ops.attn_pool_fwd(t, w2, b2, hb, mask32, nb, L, w, pooled)
        sv.update(t=t, w=w, h=h if f32 else hb, mask=mask32, f32=f32)
        return pooled

    def _pool_seg_fwd(self, name, h, hs, seg_row, seg_len):
        """_pool_fwd's attentive pooling for G segments of ONE row buffer: h fp32
        [rows, H] and its [hi | lo] split image hs, segment g the rows seg_row[g] .. seg_row[g] +
        seg_len[g] - 1, overlapping freely (the windows of a recording) -> pooled fp32 [G, H].  The
        scorer Linear runs once over the rows with _pool_fwd's operands; ops.attn_pool_seg_fwd then
        pools every segment to the bits of the dense kernels on a copy of its rows."""
        s = self.s
        t = ops.linear(hs, s.w2(name + ".attention.0.weight"), s.p(name + ".attention.0.bias"), act=ACT_TANH)
        return ops.attn_pool_seg_fwd(t, s.p(name + ".attention.2.weight").view(-1), s.p(name + ".attention.2.bias"),
                                     h, seg_row, seg_len)

    def _pool_bwd(self, name, sv, dpooled, dh, nb, L):
        s = self.s
        if not self.m.use_attentive_pooling:
            ops.weighted_pool_bwd(sv["w"], dpooled, nb, L, dh)
            return
        t = sv["t"]
        gw1 = s.g(name + ".attention.0.weight")
        gw2 = s.g(name + ".attention.2.weight")
        w2 = s.p(name + ".attention.2.weight").view(-1)
        dw2 = None if gw2 is None else gw2.view(-1)
        if sv["f32"]:
            dz = self._e(*t.shape)
            ops.attn_pool_bwd_f32(t, w2, sv["h"], sv["w"], dpooled, nb, L, dh, dz, dw2, s.g(name + ".attention.2.bias"),
                                  db1=s.g(name + ".attention.0.bias"), mask=sv["mask"])
            hs = sv.get("hs")
            if hs is None:
                ops.linear_dx(dz, self._w32(name + ".attention.0.weight"), out=dh, beta=1.0)
                self._dw32(dz, sv["h"], name + ".attention.0.weight")
                return
            # audio: dX on the bf16 dz (no cancellation per row); dW = Σ_l dz_l ⊗ h_l to ~fp32 from
            # the split halves: dz_hi·h_hi + dz_lo·h_hi + dz_hi·h_lo (three bf16 MFMA passes)
            Hh, D = t.shape[1], hs.shape[1] // 2
            dzs = ops.split_bf16(dz, 2, 2)
            ops.linear_dx(dzs[:, :Hh], s.w(name + ".attention.0.weight"), out=dh, beta=1.0)
            if gw1 is not None:
                self._dw(dzs[:, :Hh], hs[:, :D], name + ".attention.0.weight")
                self._dw(dzs[:, Hh:], hs[:, :D], name + ".attention.0.weight")
                self._dw(dzs[:, :Hh], hs[:, D:], name + ".attention.0.weight")
            return
        dz = self._e(*t.shape, dtype=BF16)
        dz_lo = self._e(*t.shape, dtype=BF16) if gw1 is not None else None
        # Σ_l dscore_l = 0 makes the scorer's first-Linear gradients small differences of large
        # terms: the bias gradient is summed in fp32 by the kernel, the weight gradient runs on
        # dz = hi + lo (two GEMM passes)
        ops.attn_pool_bwd(t, w2, sv["h"], sv["w"], dpooled, nb, L, dh, dz, dw2, s.g(name + ".attention.2.bias"),
                          db1=s.g(name + ".attention.0.bias"), dz_lo=dz_lo, mask=sv["mask"])
        ops.linear_dx(dz, s.w(name + ".attention.0.weight"), out=dh, beta=1.0)
        self._dw(dz, sv["h"], name + ".attention.0.weight")
        if dz_lo is not None:
            self._dw(dz_lo, sv["h"], name + ".attention.0.weight")

    def _xq_fwd(self, name, qin, kv, mask32, B, S, seeds, p_x):
        """CrossModalAttention (ref:125-168) for len(seeds) query sets of B rows sharing the
        keys/values kv (bf16 [B*S, 2P]), then the fusion input [qin | out_proj(att)] (fp32,
        ref:670-677).  Returns (cat [rows, 2P], saved)."""
        s = self.s
        rows, P = qin.shape
        nh = self.m.xattn_heads
        q = ops.linear(qin, self._w32(name + ".query.weight"), s.p(name + ".query.bias"))
        probs = self._e(rows * nh * S)
        att = self._e(rows, P)
        ops.xattn_fwd(q, kv[:, :P], kv[:, P:], mask32, B, S, nh, probs, att, seeds, drop_p=p_x)
        cat = self._e(rows, 2 * P)
        ops.linear(att, self._w32(name + ".out_proj.weight"), s.p(name + ".out_proj.bias"), out=cat[:, P:])
        ops.copy2d(cat[:, :P], qin)
        return cat, dict(qin=qin, q=q, probs=probs, att=att, cat=cat, kv=kv, mask=mask32, B=B, S=S, seeds=seeds, p=p_x)

    def _xq_bwd(self, name, xs, dcat, d_qin, dkvb):
        """Backward of _xq_fwd from d cat: d_qin (fp32) +=; dkvb (bf16 [B*S, 2P]) written, the
        key/value bias gradient summed in fp32 by the kernel (over both query sets); or dkvb fp32
        (zero-filled by the caller): accumulated, bias gradient left to the caller."""
        s = self.s
        P = d_qin.shape[1]
        datt = dcat[:, P:]
        _add_(d_qin, dcat[:, :P])
        dq_in = ops.linear_dx(datt, self._w32(name + ".out_proj.weight"))
        self._dw32(datt, xs["att"], name + ".out_proj.weight")
        self._db32(datt, name + ".out_proj.bias")
        dq = self._e(*xs["q"].shape)
        kv = xs["kv"]
        ops.xattn_bwd(xs["q"], kv[:, :P], kv[:, P:], xs["probs"], dq_in, xs["B"], xs["S"], self.m.xattn_heads, dq,
                      dkvb[:, :P], dkvb[:, P:], xs["seeds"], drop_p=xs["p"],
                      colsum=s.fused(name + ".key.bias", 2, "g") if dkvb.dtype == BF16 else None, mask=xs["mask"])
        ops.linear_dx(dq, self._w32(name + ".query.weight"), out=d_qin, beta=1.0)
        self._dw32(dq, xs["qin"], name + ".query.weight")
        self._db32(dq, name + ".query.bias")

    def _kv_src_bwd(self, name, src, dkvb, seqb, xb, dx):
        """K/V = Linear_kv(Linear_src(x)) backward (bf16, the shared side): dkvb [rows, 2P] ->
        dx (fp32 +=); the src bias gradient summed in the K/V input-gradient GEMM's epilogue.
        dkvb fp32 (the per-call public API, whose positive and corrupted calls backpropagate
        separately into the same audio states: their contributions cancel in dx and in these
        weights' gradients, so each is carried to ~fp32): every product on split-bf16 operands."""
        s = self.s
        if dkvb.dtype == F32:
            P2 = dkvb.shape[1]
            dkvs = ops.split_bf16(dkvb, 2, 2)
            self._db(dkvb, name + ".key.bias", fused=2)
            self._dw(dkvs[:, :P2], seqb, name + ".key.weight", fused=2)
            self._dw(dkvs[:, P2:], seqb, name + ".key.weight", fused=2)
            dseq = ops.linear(dkvs, s.wt2(name + ".key.weight", 2), colsum=s.g(src + ".bias"))
            P = dseq.shape[1]
            dseqs = ops.split_bf16(dseq, 2, 2)
            self._dw(dseqs[:, :P], xb, src + ".weight")
            self._dw(dseqs[:, P:], xb, src + ".weight")
            ops.linear(dseqs, s.wt2(src + ".weight"), out=dx, beta=1.0)
            return
        dseqb = self._dx(dkvb, name + ".key.weight", 2, out_bf16=True, colsum=s.g(src + ".bias"))
        self._dw(dkvb, seqb, name + ".key.weight", fused=2)
        self._dx(dseqb, src + ".weight", out=dx, beta=1.0)
        self._dw(dseqb, xb, src + ".weight")

    def _fuse_fwd(self, name, cat):
        """text_fusion / audio_fusion (ref:470-477, :672-677): LN(Linear(cat)) in fp32."""
        y = ops.linear(cat, self._w32(name + ".0.weight"), self.s.p(name + ".0.bias"))
        out = self._e(*y.shape)
        st = self._ln(y, name + ".1", 1e-5, y=out)
        return out, (y, st, cat)

    def _fuse_bwd(self, name, d_out, saved):
        y, st, cat = saved
        dy = self._e(*d_out.shape)
        self._ln_bwd(d_out, y, st, name + ".1", dx=dy, dsum=self.s.g(name + ".0.bias"))
        dcat = ops.linear_dx(dy, self._w32(name + ".0.weight"))
        self._dw32(dy, cat, name + ".0.weight")
        return dcat

    def _kv(self, name, src, xb):
        """bf16 K|V [rows, 2P] = Linear_kv(Linear_src(xb)) and the bf16 Linear_src output."""
        s = self.s
        seqb = ops.linear(xb, s.w(src + ".weight"), s.p(src + ".bias"), out_bf16=True)
        kv = ops.linear(seqb, s.fused(name + ".key.weight", 2, "w"), s.fused(name + ".key.bias", 2, "p"), out_bf16=True)
        return kv, seqb

    def heads_forward(self, th, thb, ah, ahb, train, base_seed, ctx):
        self._await_params("late", "text")
        m = self.m
        nb, L = ctx["t_nb"], ctx["t_L"]
        b = nb // 2
        ab, T = ctx["a_b"], ctx["a_T"]
        hs = {}
        tpool_sv, apool_sv, tproj_sv, aproj_sv = {}, {}, {}, {}
        tpooled = self._pool_fwd("text_pooling", th, thb, ctx["t_mask32"], nb, L, tpool_sv)
        apooled = self._pool_fwd("audio_pooling", ah, ahb, ctx["a_mask32"], ab, T, apool_sv, hs=ctx.get("a_hs"))
        tproj = self._proj_fwd("text_projection", tpooled, nb, train, _site_seed(base_seed, 201), tproj_sv)
        aproj = self._proj_fwd("audio_projection", apooled, ab, train, _site_seed(base_seed, 202), aproj_sv)
        hs.update(tpool=tpool_sv, apool=apool_sv, tproj=tproj_sv, aproj=aproj_sv)
        if m.use_cross_modal:
            p_x = m.dropout if train else 0.0
            # audio_seq_to_projection + text->audio K/V: identical for the pos and neg calls of
            # ref:525-542, computed once; pos and neg queries in one launch (each its own seed)
            kva, aseqb = self._kv("text_to_audio_attention", "audio_seq_to_projection", ahb)
            seed_t = _site_seed(base_seed, 203)
            tcat, hs["tx"] = self._xq_fwd("text_to_audio_attention", tproj, kva, ctx["a_mask32"], b, T,
                                          (_site_seed(seed_t, 0), _site_seed(seed_t, 1)), p_x)
            # audio->text (pos call only: the neg call's audio output is discarded, ref:535)
            kvt, tseqb = self._kv("audio_to_text_attention", "text_seq_to_projection", thb[: b * L])
            acat, hs["ax"] = self._xq_fwd("audio_to_text_attention", aproj[:b], kvt, ctx["t_mask32"][: b * L], b, L,
                                          (_site_seed(base_seed, 204),), p_x)
            tfused, hs["tf"] = self._fuse_fwd("text_fusion", tcat)
            afused, hs["af"] = self._fuse_fwd("audio_fusion", acat)
            hs.update(aseqb=aseqb, tseqb=tseqb)
        else:
            tfused, afused = tproj, aproj[:b]
        align = None
        if m.use_word_alignment:
            align = self._align_fwd(th, thb[: b * L], ahb, b, L, T, ctx, train, _site_seed(base_seed, 205), hs)
        ctx["heads"] = hs
        return tfused, afused, align

    def heads_backward(self, d_tfused, d_afused, d_align, ctx, dth, dah):
        m = self.m
        hs = ctx["heads"]
        nb, L = ctx["t_nb"], ctx["t_L"]
        b = nb // 2
        ab, T = ctx["a_b"], ctx["a_T"]
        P = m.projection_dim
        d_tproj = self._z(nb, P)
        d_aproj = self._z(ab, P)
        if d_align is not None and m.use_word_alignment:
            self._align_bwd(d_align, hs, ctx, dth, dah)
        if m.use_cross_modal:
            dtcat = self._fuse_bwd("text_fusion", d_tfused, hs["tf"])
            dacat = self._fuse_bwd("audio_fusion", d_afused, hs["af"])
            # text->audio: dK/dV leave the kernel in bf16 with their fp32 column sums (the fused
            # key/value bias gradient); the K/V input gradient leaves its GEMM in bf16 with the
            # audio_seq_to_projection bias gradient summed in the epilogue
            dkvb = self._e(ab * T, 2 * P, dtype=BF16)
            self._xq_bwd("text_to_audio_attention", hs["tx"], dtcat, d_tproj, dkvb)
            self._kv_src_bwd("text_to_audio_attention", "audio_seq_to_projection", dkvb, hs["aseqb"], ctx["_ahb"],
                             dah)
            del dkvb
            dkvtb = self._e(b * L, 2 * P, dtype=BF16)
            self._xq_bwd("audio_to_text_attention", hs["ax"], dacat, d_aproj[:b], dkvtb)
            self._kv_src_bwd("audio_to_text_attention", "text_seq_to_projection", dkvtb, hs["tseqb"],
                             ctx["_thb"][: b * L], dth[: b * L])
        else:
            _add_(d_tproj, d_tfused)
            _add_(d_aproj[:b], d_afused)
        dtpooled = self._z(nb, self.tcfg.hidden_size)
        dapooled = self._z(ab, self.acfg.hidden_size)
        self._proj_bwd("text_projection", hs["tproj"], d_tproj, dtpooled)
        self._proj_bwd("audio_projection", hs["aproj"], d_aproj, dapooled)
        self._pool_bwd("text_pooling", hs["tpool"], dtpooled, dth, nb, L)
        self._pool_bwd("audio_pooling", hs["apool"], dapooled, dah, ab, T)

    # ------------------------------------ standalone cross-modal attention (public API)
    def _mask32(self, mask_i64, n):
        m = self._e(n, dtype=torch.int32)
        _lib.call("ste_mask_i64_to_f32", mask_i64.contiguous().data_ptr(), None, m.data_ptr(), n, _lib.stream_ptr())
        return m

    def _frame_mask32(self, amask, B, T):
        """An audio mask as int32 [B*T] frames (None stays None): a sample-level wav2vec2 mask [B, N]
        goes through the conv stack's frame_mask, a frame mask [B, T] of any integer dtype through _mask32."""
        if amask is None:
            return None
        if self.raw_audio and amask.shape[-1] != T:
            from .wav2vec2 import frame_mask
            return frame_mask(self.acfg, amask, B, amask.shape[-1], T, self.s.device)[1]
        return self._mask32(amask.to(self.s.device, torch.int64), B * T)

    def _unit(self, x):
        y = self._e(*x.shape)
        ops.l2norm_fwd(x, y, self._e(x.shape[0]))
        return y

    def _frames_to_seconds(self, spans):
        return torch.where(spans < 0, -1.0, spans.float() * self.frame_seconds)

    def _fused_pair_scores(self, att, scores, *, tproj, trows, aproj, arows, qa, arow, kvt, kvblk, tm32, L, live):
        """The tail of score_pairs and score_clips, from the text -> audio attention output att [R, P] to
        the pair scores: out_proj and the text side's [projection | attended] rows, the audio -> text
        attention (row arow[r] of qa over text block kvblk[r], int32, negative = empty pair) and the audio
        side's, the two fusions, and the cosine of pair live[r]'s fused rows into scores [R].  trows /
        arows int64 [R]: the row of tproj / aproj of each pair."""
        s, P = self.s, self.m.projection_dim
        R = att.shape[0]
        tcat, acat = self._e(R, 2 * P), self._e(R, 2 * P)
        ops.linear(att, self._w32("text_to_audio_attention.out_proj.weight"),
                   s.p("text_to_audio_attention.out_proj.bias"), out=tcat[:, P:])
        ops.copy2d(tcat[:, :P], tproj.index_select(0, trows))
        ops.xattn_gather_fwd(qa, arow, kvt[:, :P], kvt[:, P:], kvblk, tm32, R, L, self.m.xattn_heads, att)
        ops.linear(att, self._w32("audio_to_text_attention.out_proj.weight"),
                   s.p("audio_to_text_attention.out_proj.bias"), out=acat[:, P:])
        ops.copy2d(acat[:, :P], aproj.index_select(0, arows))
        tfused, _ = self._fuse_fwd("text_fusion", tcat)
        afused, _ = self._fuse_fwd("audio_fusion", acat)
        ops.topk_target_score(self._unit(afused), self._unit(tfused), live, scores)
        return scores

    def cross_forward(self, tproj, th, tmask, aproj, ah, amask, train, seed):
        """apply_cross_modal_attention (ref:643-682) for one call: text [b,P] + hidden [b,L,Ht],
        audio [b,P] + hidden [b,T,Ha] -> (text_fused, audio_fused) [b,P] fp32 and the saved
        context.  The fused training step shares one audio K/V between the pos and neg calls
        (heads_forward); this is the reference's per-call form behind the public method, on the
        same helpers."""
        m = self.m
        b, L, Ht = th.shape
        T, Ha = ah.shape[1], ah.shape[2]
        p_x = m.dropout if train else 0.0
        thb = ops.cast_bf16(th.contiguous(), self._e(b * L, Ht, dtype=BF16))
        ahb = ops.cast_bf16(ah.contiguous(), self._e(b * T, Ha, dtype=BF16))
        tm32 = self._mask32(tmask, b * L) if tmask is not None else None
        am32 = self._frame_mask32(amask, b, T)
        kva, aseqb = self._kv("text_to_audio_attention", "audio_seq_to_projection", ahb)
        tcat, tx = self._xq_fwd("text_to_audio_attention", tproj.float().contiguous(), kva, am32, b, T,
                                (_site_seed(seed, 1),), p_x)
        kvt, tseqb = self._kv("audio_to_text_attention", "text_seq_to_projection", thb)
        acat, ax = self._xq_fwd("audio_to_text_attention", aproj.float().contiguous(), kvt, tm32, b, L,
                                (_site_seed(seed, 2),), p_x)
        tfused, tf = self._fuse_fwd("text_fusion", tcat)
        afused, af = self._fuse_fwd("audio_fusion", acat)
        sv = dict(b=b, L=L, T=T, thb=thb, ahb=ahb, aseqb=aseqb, tseqb=tseqb, tx=tx, ax=ax, tf=tf, af=af)
        return tfused, afused, sv

    @torch.no_grad()
    def score_pairs(self, tproj, th, tmask, aproj, ah, amask, candidates, audio_context=None):
        """The fused pair score the model is trained on (ref:525-563; cv_inference.py:148-161), for
        C candidate transcripts per clip: text [U,P] + hidden [U,L,Ht] + mask [U,L] (the DISTINCT
        transcripts), audio [B,P] + hidden [B,T,Ha] + mask, candidates int [B,C] with values in
        [-1, U) -> scores fp32 [B,C], -inf for an empty (-1) slot.

        The audio K/V is projected once per clip and the text K/V once per distinct transcript;
        slot (b, c)'s text query attends over clip b's audio (xattn_mq_fwd, queries gathered in the
        kernel) and clip b's audio query over transcript candidates[b, c] (xattn_gather_fwd).
        audio_context=None is the pair form (each pair's audio embedding is fused with its own
        candidate); audio_context=j fuses every row's audio with column j's transcript, which with
        candidates [clean, corrupted] and j = 0 is the training forward's (s_pos, s_neg).  Without
        use_cross_modal the score is the cosine of the projections.  Inference arithmetic (no
        dropout), nothing saved.  Scores come from the fp32 MFMA chain of topk_target_score."""
        m, dev = self.m, self.s.device
        U, L, Ht = th.shape
        B, T, Ha = ah.shape
        P = m.projection_dim
        cand, _, _ = _candidates(candidates, B, U, "C", dev)
        C = cand.shape[1]
        if audio_context is not None and not 0 <= int(audio_context) < C:
            raise ValueError(f"audio_context must be a column of candidates, got {audio_context}")
        R = B * C
        slot = cand.view(-1)
        tproj, aproj = tproj.float().contiguous(), aproj.float().contiguous()
        scores = torch.full((R,), float("-inf"), device=dev, dtype=F32)
        arep = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(C)   # clip of each pair
        if not m.use_cross_modal:
            ops.topk_target_score(self._unit(aproj).index_select(0, arep.long()), self._unit(tproj), slot, scores)
            return scores.view(B, C)
        thb = ops.cast_bf16(th.contiguous(), self._e(U * L, Ht, dtype=BF16))
        ahb = ops.cast_bf16(ah.contiguous(), self._e(B * T, Ha, dtype=BF16))
        tm32 = self._mask32(tmask, U * L) if tmask is not None else None
        am32 = self._frame_mask32(amask, B, T)
        kva, _ = self._kv("text_to_audio_attention", "audio_seq_to_projection", ahb)    # once per clip
        kvt, _ = self._kv("audio_to_text_attention", "text_seq_to_projection", thb)     # once per transcript
        s = self.s
        qt = ops.linear(tproj, self._w32("text_to_audio_attention.query.weight"),
                        s.p("text_to_audio_attention.query.bias"))
        qa = ops.linear(aproj, self._w32("audio_to_text_attention.query.weight"),
                        s.p("audio_to_text_attention.query.bias"))
        # the transcript each pair's audio attends over; a pair is empty when either side is
        ctx_t = slot if audio_context is None else cand[:, int(audio_context)].repeat_interleave(C)
        kvblk = torch.where(slot < 0, slot, ctx_t).contiguous()
        live = torch.where(kvblk < 0, kvblk, torch.arange(R, device=dev, dtype=torch.int32))
        att = self._e(R, P)
        ops.xattn_mq_fwd(qt, slot, kva[:, :P], kva[:, P:], am32, B, C, T, m.xattn_heads, att)
        return self._fused_pair_scores(att, scores, tproj=tproj, trows=slot.clamp(min=0).long(), aproj=aproj,
                                       arows=arep.long(), qa=qa, arow=arep, kvt=kvt, kvblk=kvblk, tm32=tm32, L=L,
                                       live=live).view(B, C)

    @torch.no_grad()
    def score_clips(self, tproj, th, tmask, store, candidates):
        """score_pairs in the other direction: the fused pair score of k candidate corpus
        clips per text query.  text [Q,P] + hidden [Q,L,Ht] + mask [Q,L]; store: a
        retrieval.AudioStateStore built with these weights (else RuntimeError); candidates int [Q,k]
        of clip ids in [-1, len(store)) -> scores fp32 [Q,k], -inf for an empty (-1) slot.

        The pair form of score_pairs: the text K/V is projected once per query and the audio query
        once per DISTINCT candidate clip; the pairs are grouped by clip (retrieval.plan_clip_pairs),
        pair (i, n)'s text query attends over clip n's stored K/V rows in place (xattn_seg_fwd) and
        clip n's audio query over text i (xattn_gather_fwd); then score_pairs' chain.  Without
        use_cross_modal the score is the cosine of the stored unit row."""
        from .retrieval import plan_clip_pairs
        m, dev, s = self.m, self.s.device, self.s
        Q, L, Ht = th.shape
        P = m.projection_dim
        cand, _, hi = _candidates(candidates, Q, len(store), "k", dev)
        store.check()
        k = cand.shape[1]
        R = Q * k
        tproj = tproj.float().contiguous()
        if not m.use_cross_modal:
            scores = torch.full((R,), float("-inf"), device=dev, dtype=F32)
            qs = self._unit(tproj).repeat_interleave(k, 0)
            for base, rows in store.index.chunks:
                ops.topk_target_score(qs, rows, cand.view(-1), scores, index_base=base)
            return scores.view(Q, k)
        if hi < 0:
            return torch.full((Q, k), float("-inf"), device=dev, dtype=F32)
        plan = plan_clip_pairs(cand)
        qrow, pseg = plan["qrow"], plan["pseg"]
        clips = plan["unique"].long()
        thb = ops.cast_bf16(th.contiguous(), self._e(Q * L, Ht, dtype=BF16))
        tm32 = self._mask32(tmask, Q * L) if tmask is not None else None
        kvt, _ = self._kv("audio_to_text_attention", "text_seq_to_projection", thb)     # once per query
        aproj = store.aproj.index_select(0, clips)                                      # the distinct clips
        qt = ops.linear(tproj, self._w32("text_to_audio_attention.query.weight"),
                        s.p("text_to_audio_attention.query.bias"))
        qa = ops.linear(aproj, self._w32("audio_to_text_attention.query.weight"),
                        s.p("audio_to_text_attention.query.bias"))
        live = torch.where(pseg < 0, pseg, torch.arange(R, device=dev, dtype=torch.int32))
        att = self._e(R, P)
        kx, vx, scales = store.kv_bank.xattn_operands()   # bf16 rows, or e4m3 bytes and their scales (§19)
        ops.xattn_seg_fwd(qt, qrow, pseg, kx, vx, store.seg_row.index_select(0, clips),
                          store.frames.index_select(0, clips), plan["tile_first"], plan["tile_cnt"], m.xattn_heads, att,
                          **scales)
        scores = torch.full((R,), float("-inf"), device=dev, dtype=F32)
        self._fused_pair_scores(att, scores, tproj=tproj, trows=qrow.clamp(min=0).long(), aproj=aproj,
                                arows=pseg.clamp(min=0).long(), qa=qa, arow=pseg, kvt=kvt, kvblk=qrow, tm32=tm32, L=L,
                                live=live)
        return scores.index_select(0, plan["inverse"].view(-1)).view(Q, k)

    def cross_backward(self, sv, d_tf, d_af):
        """-> (d text_projected [b,P], d text_hidden [b*L,Ht], d audio_projected [b,P],
        d audio_hidden [b*T,Ha]) fp32; parameter gradients += into the flat gradient buffer."""
        b, L, T = sv["b"], sv["L"], sv["T"]
        P = self.m.projection_dim
        Ht, Ha = sv["thb"].shape[1], sv["ahb"].shape[1]
        d_tproj, d_aproj = self._z(b, P), self._z(b, P)
        dth, dah = self._z(b * L, Ht), self._z(b * T, Ha)
        dtcat = self._fuse_bwd("text_fusion", d_tf.float().contiguous(), sv["tf"])
        dacat = self._fuse_bwd("audio_fusion", d_af.float().contiguous(), sv["af"])
        # per call, fp32 dK/dV and split-bf16 K/V products: the positive and corrupted calls'
        # contributions to the shared audio side cancel once the caller's autograd sums them
        dkv = self._z(b * T, 2 * P)
        self._xq_bwd("text_to_audio_attention", sv["tx"], dtcat, d_tproj, dkv)
        self._kv_src_bwd("text_to_audio_attention", "audio_seq_to_projection", dkv, sv["aseqb"], sv["ahb"], dah)
        dkvt = self._z(b * L, 2 * P)
        self._xq_bwd("audio_to_text_attention", sv["ax"], dacat, d_aproj, dkvt)
        self._kv_src_bwd("audio_to_text_attention", "text_seq_to_projection", dkvt, sv["tseqb"], sv["thb"], dth)
        return d_tproj, dth, d_aproj, dah

    # ------------------------------------------------------- word alignment
    def _align_fwd(self, th, thb_pos, ahb, b, L, T, ctx, train, seed, hs):
        from .align import align_forward
        return align_forward(self, th, thb_pos, ahb, b, L, T, ctx, train, seed, hs)

    def _align_bwd(self, d_align, hs, ctx, dth, dah):
        from .align import align_backward
        align_backward(self, d_align, hs, ctx, dth, dah)

    @property
    def frame_seconds(self):
        """Seconds per encoder frame: two stacked fbank hops (w2v-bert), or the conv stack's total
        stride in samples (wav2vec2), at 16 kHz — 0.02 for both families."""
        from .features import HOP, SAMPLE_RATE, STACK
        samples = math.prod(self.acfg.conv_stride) if self.raw_audio else HOP * STACK
        return samples / SAMPLE_RATE

    @torch.no_grad()
    def _spot(self, emit, ntok, nfrm, lead, trail, spot_bias):
        """The free-endpoint decode of pairs' emissions: ops.align_spot over the phrase tokens
        lead .. n-1-trail of each pair (n = ntok; a pair with no frame, or with n - lead - trail < 1, is
        infeasible) against bg = -log(nfrm) + spot_bias in fp32 on the device: the head's rows sum to 1
        over a clip's frames, so at spot_bias = 0 a frame gains exactly when its token attends to it
        more than uniformly.  -> (spans int32 [R, L, 2], hit int32 [R, 2], score fp32 [R])."""
        if lead < 0 or trail < 0:
            raise ValueError(f"lead and trail count tokens, got {lead}, {trail}")
        L = emit.shape[2]
        if lead >= L:      # no phrase column is left: every pair is infeasible, and the kernel refuses such a lead
            lead, m = 0, torch.zeros_like(ntok)
        else:
            m = (ntok - (lead + trail)).clamp(min=0).to(torch.int32)
        bg = -torch.log(nfrm.clamp(min=1).to(F32)) + float(spot_bias)
        return ops.align_spot(emit, m.contiguous(), nfrm, bg.contiguous(), lead)

    def _align_result(self, spans, scores, path, hits=None, matrix=None, word_ids=None, shape=None):
        """The dict align_pairs and locate_clips return, from per-pair rows: token spans / seconds, scores,
        path score, hit spans / seconds and the matrix where given, and the word-level entries with
        word_ids int [R, L].  shape = (Q, k) views every entry [R, ...] as [Q, k, ...]."""
        from .align import words_from_tokens
        sec = self._frames_to_seconds
        out = dict(token_spans=spans, token_seconds=sec(spans), scores=scores, path_score=path)
        if hits is not None:
            out.update(hit_spans=hits, hit_seconds=sec(hits))
        if matrix is not None:
            out["matrix"] = matrix
        if word_ids is not None:
            ws, wsc = words_from_tokens(spans, scores, word_ids)
            out.update(word_spans=ws, word_seconds=sec(ws), word_scores=wsc)
        if shape is not None:
            out = {name: t.view(*shape, *t.shape[1:]) for name, t in out.items()}
        return out

    @torch.no_grad()
    def align_pairs(self, th, tmask, ah, amask, word_ids=None, return_matrix=False, *, free_ends=False, lead=1,
                    trail=1, spot_bias=0.0):
        """Word timestamps from the alignment head: clip b against transcript b, text
        hidden [B,L,Ht] + mask [B,L], audio hidden [B,T,Ha] + mask (frames, or wav2vec2 samples; None
        = every frame valid).  align_infer gives the confidence, the head-mean alignment matrix and its
        frame-major log; ops.align_decode turns that into one frame span per token over the pair's
        ntok = Σ text mask tokens and nfrm = Σ frame mask frames.  Both masks must be prefix masks
        (checked on the device, one sync).  Inference arithmetic, nothing saved.  free_ends=True
        decodes the same emissions with ops.align_spot instead (_spot; lead, trail and
        spot_bias are read in this mode only).  -> dict, see EnhancedAudioTextModel.align."""
        from .align import align_infer
        dev = self.s.device
        B, L, Ht = th.shape
        T, Ha = ah.shape[1], ah.shape[2]
        if ah.shape[0] != B:
            raise ValueError(f"align pairs clip b with transcript b: {ah.shape[0]} clips, {B} transcripts")
        tm = (torch.ones(B, L, dtype=torch.int64, device=dev) if tmask is None
              else tmask.to(dev, torch.int64).contiguous())
        am32 = self._frame_mask32(amask, B, T)
        bad = (tm[:, 1:] > tm[:, :-1]).any()
        if am32 is not None:
            fm = am32.view(B, T)
            bad = bad | ((fm[:, 1:] != 0) & (fm[:, :-1] == 0)).any()
        if bool(bad):
            raise ValueError("align needs prefix masks (right-padded transcripts and clips)")
        ntok = (tm != 0).sum(1, dtype=torch.int32)
        nfrm = (torch.full((B,), T, dtype=torch.int32, device=dev) if am32 is None
                else (am32.view(B, T) != 0).sum(1, dtype=torch.int32))
        thf = th.reshape(B * L, Ht).float().contiguous()
        thb = ops.cast_bf16(thf, self._e(B * L, Ht, dtype=BF16))
        ahb = ops.cast_bf16(ah.reshape(B * T, Ha).float().contiguous(), self._e(B * T, Ha, dtype=BF16))
        scores, matrix, emit = align_infer(self, thf, thb, ahb, B, L, T, {"a_mask32": am32, "_tmask_i64": tm},
                                           want_matrix=return_matrix, want_emit=True)
        if free_ends:
            spans, hits, path = self._spot(emit, ntok, nfrm, lead, trail, spot_bias)
        else:
            (spans, path), hits = ops.align_decode(emit, ntok, nfrm), None
        return self._align_result(spans, scores, path, hits, matrix if return_matrix else None,
                                  None if word_ids is None else word_ids.to(dev))

    @torch.no_grad()
    def locate_clips(self, th, tmask, store, candidates, word_ids=None, lead=1, trail=1, pair_batch=128,
                     return_matrix=False, return_emit=False, *, free_ends=False, spot_bias=0.0):
        """Where in each of k candidate corpus clips is a text query spoken: align_pairs for
        (query, stored clip) pairs, without the waveforms and without an audio-encoder pass.  Text
        hidden [Q,L,Ht] + prefix mask [Q,L] (None = every token valid); store: a
        retrieval.AudioStateStore(align_rows=True) built with these weights (else ValueError /
        RuntimeError); candidates int [Q,k] of clip ids in [-1, len(store)), -1 = empty slot.

        The head's queries are projected once per query; pair (i, n) runs query block i over clip n's
        stored alignment K|V rows in place (ops.align_matrix_seg_fwd on the alignment bank's operands,
        whichever its dtype; the clip ids being the segment indices of the store's own table), then
        align.confidence_tail and ops.align_decode with ntok from the query and nfrm from the clip.  The
        pairs run in chunks of pair_batch, which bounds the emissions buffer at pair_batch·Tmax·L·4 bytes;
        Tmax, the longest candidate clip, comes with the one device -> host sync of the argument checks.

        -> dict of [Q, k, ...] tensors: token_spans int32 [Q,k,L,2] and token_seconds, scores fp32
        [Q,k,L], path_score fp32 [Q,k], hit_spans int32 [Q,k,2] and hit_seconds (align.hit_spans:
        first frame of token `lead` to the end of token n-1-trail), word_spans / word_seconds /
        word_scores with word_ids int [Q,L]; matrix fp32 [Q,k,L,Tmax] / emit fp32 [Q,k,Tmax,L] on
        request (frames past a clip's own are 0 / -inf).  An empty slot and an infeasible pair (fewer
        frames than tokens) have spans (-1, -1), path_score -inf and scores 0.

        free_ends=True replaces the decode alone: ops.align_spot over the phrase tokens
        lead .. n-1-trail against the background -log(nfrm) + spot_bias (_spot), for a typed phrase
        that is a fragment of what the clip says.  token_spans then hold the phrase tokens' spans and
        (-1, -1) on the lead / trail tokens and the padding, hit_spans the kernel's hit, and path_score the
        summed gain over the hit (a log-likelihood ratio; <= 0: the phrase nowhere beats the
        background); scores, matrix and emit are the default mode's bits."""
        from .align import confidence_tail, hit_spans, text_queries
        m, dev = self.m, self.s.device
        if not m.use_word_alignment:
            raise ValueError("locate_clips needs a model built with use_word_alignment=True")
        if not getattr(store, "align_rows", False):
            raise ValueError("locate_clips needs an AudioStateStore built with align_rows=True")
        Q, L, Ht = th.shape
        P = m.projection_dim
        N = len(store)
        tm = (torch.ones(Q, L, dtype=torch.int64, device=dev) if tmask is None
              else tmask.to(dev, torch.int64).contiguous())
        cand = _candidate_lists(candidates, Q, "k", dev)
        k = cand.shape[1]
        R = Q * k
        pseg = cand.view(-1)
        live = (pseg >= 0) & (pseg < N)          # a clip id outside the store is refused below, never looked up
        nfrm = (store.frames.index_select(0, torch.where(live, pseg, 0).long()) * live if N
                else torch.zeros(R, dtype=torch.int32, device=dev)).to(torch.int32)
        bad = (tm[:, 1:] > tm[:, :-1]).any()
        # the text-mask check and the longest candidate clip come with the candidates' one sync
        _, _, _, bad, Tmax = _candidates(cand, Q, N, "k", dev, (bad.to(torch.int32), nfrm.max()))
        if bad:
            raise ValueError("locate_clips needs prefix text masks (right-padded transcripts)")
        store.check()
        qblk = torch.where(live, torch.arange(R, device=dev, dtype=torch.int32) // k, -1).to(torch.int32)
        ntok = ((tm != 0).sum(1, dtype=torch.int32).repeat_interleave(k) * live).to(torch.int32)
        spans = torch.full((R, L, 2), -1, dtype=torch.int32, device=dev)
        scores = torch.zeros(R, L, device=dev, dtype=F32)
        path = torch.full((R,), float("-inf"), device=dev, dtype=F32)
        hits = torch.full((R, 2), -1, dtype=torch.int32, device=dev) if free_ends else None
        Tm = max(Tmax, 1)
        matrix = torch.zeros(R, L, Tm, device=dev, dtype=F32) if return_matrix else None
        emit_all = torch.full((R, Tm, L), float("-inf"), device=dev, dtype=F32) if return_emit else None
        if Tmax > 0:                            # else every slot is empty
            nh = m.word_level_alignment.num_heads
            thf = th.reshape(Q * L, Ht).float().contiguous()
            q = text_queries(self, ops.cast_bf16(thf, self._e(Q * L, Ht, dtype=BF16)))      # once per query
            seg_row, seg_len = store.seg_row, store.frames
            akv, scales = store.align_bank.align_operands()   # bf16 rows, or e4m3 bytes + scales, in place (§21)
            step = max(int(pair_batch), 1)
            for r0 in range(0, R, step):
                r1 = min(r0 + step, R)
                n = r1 - r0
                qb, row = qblk[r0:r1].contiguous(), qblk[r0:r1].clamp(min=0).long()
                emit = emit_all[r0:r1] if return_emit else self._e(n, Tmax, L)
                att = self._e(n * L, P, dtype=BF16)
                ops.align_matrix_seg_fwd(q, qb, pseg[r0:r1].contiguous(), akv, seg_row, seg_len, L, Tmax, nh,
                                         matrix=None if matrix is None else matrix[r0:r1], emit=emit, out=att, **scales)
                th_rows = thf.view(Q, L, Ht).index_select(0, row).view(n * L, Ht)
                tm_rows = (tm.index_select(0, row) * (qb >= 0).view(n, 1)).contiguous()
                scores[r0:r1] = confidence_tail(self, att, th_rows, tm_rows, n * L).view(n, L)
                if free_ends:
                    spans[r0:r1], hits[r0:r1], path[r0:r1] = self._spot(emit, ntok[r0:r1], nfrm[r0:r1].contiguous(),
                                                                        lead, trail, spot_bias)
                else:
                    spans[r0:r1], path[r0:r1] = ops.align_decode(emit, ntok[r0:r1].contiguous(),
                                                                 nfrm[r0:r1].contiguous())
        if not free_ends:
            hits = hit_spans(spans, ntok, lead, trail)
        out = self._align_result(spans, scores, path, hits, matrix,
                                 None if word_ids is None else word_ids.to(dev).repeat_interleave(k, 0), (Q, k))
        if return_emit:
            out["emit"] = emit_all.view(Q, k, Tm, L)
        return out

    # ============================================================== full step
    def forward(self, batch, train: bool, save: bool = True):
        """compute_pos_neg_embeddings (ref:502-565) -> (tp_fused, tn_fused, a_fused, align, ctx).
        save=False (forward-only evaluation, ref:1165-1284 under no_grad): no encoder layer keeps
        its activations, so each layer's buffers return to the allocator as the next one runs, and
        the FFN GEMMs skip the pre-activation copies only backward reads."""
        ctx = Ctx()
        base_seed = int(torch.randint(0, 2**62, (1,)).item()) if train else 0
        ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]], 0)
        tmask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]], 0).contiguous()
        ctx["_tmask_i64"] = tmask  # rows [0, b) = positive transcripts (alignment head's text mask)
        side = self._side_stream()
        text = {}
        if side is not None:  # text encoder on the side stream, audio encoder on the main stream
            main = torch.cuda.current_stream(self.s.device)
            ready = torch.cuda.Event()
            ready.record(main)   # the text inputs (and everything the main stream did before them)

            def enqueue_text():
                side.wait_event(ready)
                with torch.cuda.stream(side):
                    text["h"] = self.text_forward(ids.contiguous(), tmask, train, _site_seed(base_seed, 2), ctx, save)
            if self.text_after_first_layer:
                # the host enqueues the text forward (~200 launches) after the audio encoder's first
                # layer, so the main stream has work queued meanwhile (the kernel trace showed it idle
                # at the step start; untraced the gain is ~0.2 %, DESIGN §3 "Two HIP streams")
                ctx["_text_enqueue"] = enqueue_text
            else:
                enqueue_text()
        else:
            text["h"] = self.text_forward(ids.contiguous(), tmask, train, _site_seed(base_seed, 2), ctx, save)
        amask = batch.get("attention_mask_audio")
        # host-known clip lengths in the mask's units (fbank frames / raw samples), for SpecAugment's
        # span sampling without a device sync: given by the caller, or summed from a host mask
        alens = batch.get("audio_lengths")
        if alens is None and amask is not None and amask.device.type == "cpu":
            alens = amask.sum(-1).tolist()
        if amask is not None and amask.device != self.s.device:
            amask = amask.to(self.s.device, non_blocking=True)
        ah, ahb = self.audio_forward(batch["input_values"].contiguous(),
                                     None if amask is None else amask.contiguous(), train, _site_seed(base_seed, 3),
                                     ctx, save, lengths=None if alens is None else [int(n) for n in alens])
        if "_text_enqueue" in ctx:   # an audio path that ran no Conformer layer loop (wav2vec2 front-end)
            ctx.pop("_text_enqueue")()
        th, thb = text["h"]
        if side is not None:
            main.wait_stream(side)
        ctx["_thb"], ctx["_ahb"] = thb, ahb
        tf, af, align = self.heads_forward(th, thb, ah, ahb, train, _site_seed(base_seed, 4), ctx)
        b = batch["input_ids_pos"].shape[0]
        return tf[:b], tf[b:], af, align, ctx

    def backward(self, ctx, d_tp, d_tn, d_af, d_align, stage_done=None):
        """Backward of the whole step.  stage_done(name) is called once the gradients of a
        parameter block are final, so a data-parallel caller can start their collective while the
        rest of the backward runs: "heads", then (text on its side stream) "text_layers" and "text"
        with the current stream set to that side stream, "audio_layers", "audio"; on one stream the
        GradSync.STAGES order "heads", "audio_layers", "audio", "text_layers", "text"."""
        nb = ctx["t_nb"]
        d_tf = self._e(nb, self.m.projection_dim)
        _copy_f32(d_tp, d_tf[: nb // 2])
        _copy_f32(d_tn, d_tf[nb // 2:])
        dth = self._z(nb * ctx["t_L"], self.tcfg.hidden_size)
        dah = self._z(ctx["a_b"] * ctx["a_T"], self.acfg.hidden_size)
        self.heads_backward(d_tf, d_af, d_align, ctx, dth, dah)
        ctx.pop("heads", None)
        if stage_done:
            stage_done("heads")
        side = self._side_stream()
        if side is not None:  # text backward on the side stream, concurrent with the audio backward
            main = torch.cuda.current_stream(self.s.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self.text_backward(dth, ctx, (lambda: stage_done("text_layers")) if stage_done else None)
                if stage_done:
                    # the text block is final once the side stream has run its backward: its
                    # collectives (dense all-reduce, word-table row exchange) are queued behind it on
                    # the side stream and overlap the audio backward's frozen layers, instead of
                    # waiting for the join
                    stage_done("text")
            self.audio_backward(dah, ctx, (lambda: stage_done("audio_layers")) if stage_done else None)
            main.wait_stream(side)
            del dah
            if stage_done:
                stage_done("audio")
        else:
            self.audio_backward(dah, ctx, (lambda: stage_done("audio_layers")) if stage_done else None)
            del dah
            if stage_done:
                stage_done("audio")
            self.text_backward(dth, ctx, (lambda: stage_done("text_layers")) if stage_done else None)
            if stage_done:
                stage_done("text")
        ctx.clear()


def _candidate_lists(candidates, rows, name, device=None):
    """Candidate lists as int32, contiguous, on device, of shape [rows, name >= 1], else ValueError."""
    cand = candidates.to(device=device, dtype=torch.int32).contiguous()
    if cand.dim() != 2 or cand.shape[0] != rows or cand.shape[1] < 1:
        raise ValueError(f"candidates must be [{rows}, {name} >= 1], got {tuple(cand.shape)}")
    return cand


def _candidates(candidates, rows, n, name, device=None, more=()):
    """_candidate_lists, then the values in [-1, n), else ValueError, in ONE device -> host transfer that
    also reads the 0-d integer tensors of more.  -> (cand, lo, hi, *their values)."""
    cand = _candidate_lists(candidates, rows, name, device)
    lo, hi, *rest = (int(x) for x in torch.stack((cand.min(), cand.max(), *more)).tolist())
    if lo < -1 or hi >= n:
        raise ValueError(f"candidates must lie in [-1, {n}), got [{lo}, {hi}]")
    return (cand, lo, hi, *rest)


def _copy_f32(src, dst):
    ops.copy2d(dst, src)


def _add_(dst, src):
    ops.axpby(dst, src, 1.0, 1.0)
