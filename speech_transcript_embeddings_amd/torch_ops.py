"""PyTorch custom operators over the libste.so C ABI (torch.library, namespace `ste::`).

SURVEY §8(b)'s custom-op layer: each op is a schema'd `torch.ops.ste.*` operator whose
implementation is the HIP kernel behind include/ste.h (launched on the current stream through
ops.py), with a fake (meta) implementation for shape propagation and, where the reference's op
is differentiable, an autograd formula registered with torch.library.register_autograd whose
backward is again a HIP kernel.  They let code outside this package build the step op by op
(tests/test_torch_ops_gpu.py drives the reference's _forward() body, trainer_unfreeze.py:1068-1081,
through them); the fused training step itself calls the C ABI directly (engine.py, train.py).

    ste::fbank(wav, lengths, t_max, pad_value, mask_mode) -> (features, mask)
        SeamlessM4TFeatureExtractor + custom_collate_fn (ref :856-866, :880-921)
    ste::resample(wav, lengths, sr_in, sr_out) -> (wav_out, lengths_out)
        Audio(sampling_rate=16000) / librosa.resample of the data workers (ref :1927, processor.py:82-85)
    ste::linear(x, weight, bias?) -> y                       nn.Linear, bf16 MFMA / fp32 accumulate
    ste::layer_norm(x, weight, bias, eps) -> (y, mean, rstd) nn.LayerNorm
    ste::attention(q, k, v, key_mask?, rel_E?, scale, rel_left, rel_right) -> (o, lse, o_lo)
        Wav2Vec2BertSelfAttention relative_key core (tf:…wav2vec2_bert…:229-337) / SDPA
    ste::pair_loss(s_pos, s_neg, alignment_scores?, temperature, alignment_weight, corrupt_gamma) -> loss
        AlignmentAwareInfoNCE (ref :702-742)
    ste::adamw_(p!, g, m!, v!, p_bf16!, lr, beta1, beta2, eps, weight_decay, step, sumsq?, max_norm)
        AdamW.step with clip_grad_norm_'s coefficient folded in (ref :1108-1110)
    ste::topk_sim(q, corpus, k) -> (values, indices)
        the k best corpus rows per query by dot product (retrieval over processor.py:128-146's embeddings)
    ste::xattn_mq(q, qrow, k, v, mask?, C, nh) -> out
        CrossModalAttention core (ref :125-168) for C candidate queries per clip sharing its keys/values
    ste::xattn_seg(q, qrow, pseg, k, v, seg_row, seg_len, tile_first, tile_cnt, nh) -> out
        the same core for (text query, stored corpus clip) pairs: segments of one K/V buffer
    ste::xattn_seg_mx8(q, qrow, pseg, k, v, ks, vs, seg_row, seg_len, tile_first, tile_cnt, nh) -> out
        ste::xattn_seg on rows stored as MX-fp8 bytes and E8M0 block scales
    ste::align_matrix(q, kv, kmask?, nh) -> (matrix, emit, out)
        WordLevelAlignmentModule's head-averaged alignment_matrix (ref :295), its frame-major log, the output
    ste::align_matrix_seg(q, qblk, pseg, kv, seg_row, seg_len, Tmax, nh) -> (matrix, emit, out)
        ste::align_matrix for (text query, stored corpus clip) pairs: segments of one K|V buffer
    ste::align_matrix_seg_mx8(q, qblk, pseg, kv, scales, seg_row, seg_len, Tmax, nh) -> (matrix, emit, out)
        ste::align_matrix_seg on rows stored as MX-fp8 bytes and E8M0 block scales
    ste::align_decode(emit, ntok, nfrm) -> (spans, score)
        monotone (Viterbi) decode of that log matrix into one frame span per token
    ste::align_spot(emit, ntok, nfrm, bg, lead=0) -> (spans, hit, score)
        the same decode with both ends free against a per-pair background: phrase spotting
    ste::attn_pool_seg(t, w2, b2, h, seg_row, seg_len) -> pooled
        AttentivePooling (ref :171-211) of overlapping segments of one row buffer: a recording's windows

Every op fails loudly (SteError) without the HIP library; there is no CPU implementation.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from . import _lib, ops

BF16, F32 = torch.bfloat16, torch.float32


def _bf16(t: Tensor) -> Tensor:
    """bf16 contiguous 2-D operand (fp32 inputs cast on the ste cast kernel)."""
    t = t.contiguous()
    if t.dtype == BF16:
        return t
    if t.dtype != F32:
        raise TypeError(f"ste ops take fp32 or bf16 tensors, got {t.dtype}")
    return ops.cast_bf16(t, torch.empty(t.shape, device=t.device, dtype=BF16))


def _i32(t: Tensor) -> Tensor:
    return t.reshape(-1).to(torch.int32).contiguous()


# ------------------------------------------------------------------------ fbank
@torch.library.custom_op("ste::fbank", mutates_args=())
def fbank(wav: Tensor, lengths: Tensor, t_max: int, pad_value: float = 1.0, mask_mode: int = 0) -> tuple[Tensor, Tensor]:
    return ops.fbank(wav.float().contiguous(), lengths.to(torch.int32).contiguous(), int(t_max), pad_value=pad_value,
                     mask_mode=mask_mode)


@fbank.register_fake
def _fbank_fake(wav, lengths, t_max, pad_value=1.0, mask_mode=0):
    return wav.new_empty(wav.shape[0], t_max, 160, dtype=F32), wav.new_empty(wav.shape[0], t_max, dtype=torch.int64)


# --------------------------------------------------------------------- resample
@torch.library.custom_op("ste::resample", mutates_args=())
def resample(wav: Tensor, lengths: Tensor, sr_in: int, sr_out: int = 16000) -> tuple[Tensor, Tensor]:
    wav, lengths = wav.float().contiguous(), lengths.to(torch.int32).contiguous()
    if sr_in == sr_out:   # a custom op may not return its inputs: copies here, ops.resample returns them as they are
        return wav.clone(), lengths.clone()
    return ops.resample(wav, lengths, int(sr_in), int(sr_out))


@resample.register_fake
def _resample_fake(wav, lengths, sr_in, sr_out=16000):
    g = math.gcd(sr_in, sr_out)
    M, L = sr_in // g, sr_out // g
    return (wav.new_empty(wav.shape[0], (wav.shape[1] * L + M - 1) // M, dtype=F32),
            wav.new_empty(wav.shape[0], dtype=torch.int32))


# ----------------------------------------------------------------------- linear
@torch.library.custom_op("ste::linear", mutates_args=())
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    x2 = x.reshape(-1, x.shape[-1])
    y = ops.linear(_bf16(x2), _bf16(weight), None if bias is None else bias.float().contiguous())
    return y.view(*x.shape[:-1], weight.shape[0])


@linear.register_fake
def _linear_fake(x, weight, bias=None):
    return x.new_empty(*x.shape[:-1], weight.shape[0], dtype=F32)


def _linear_setup(ctx, inputs, output):
    x, weight, bias = inputs
    ctx.save_for_backward(x, weight)
    ctx.has_bias = bias is not None
    ctx.dtypes = (x.dtype, weight.dtype, None if bias is None else bias.dtype)


def _linear_bwd(ctx, dy):
    x, weight = ctx.saved_tensors
    N, K = weight.shape
    dy2 = _bf16(dy.reshape(-1, N).float())
    dx = ops.linear_dx(dy2, _bf16(weight)).view(*x.shape[:-1], K)
    dw = ops.linear_dw(dy2, _bf16(x.reshape(-1, K)))
    db = None
    if ctx.has_bias:
        db = ops.colsum(dy.reshape(-1, N).float().contiguous(), torch.zeros(N, device=dy.device, dtype=F32))
    xd, wd, bd = ctx.dtypes
    return dx.to(xd), dw.to(wd), (db.to(bd) if db is not None else None)


torch.library.register_autograd("ste::linear", _linear_bwd, setup_context=_linear_setup)


# ------------------------------------------------------------------- layer norm
@torch.library.custom_op("ste::layer_norm", mutates_args=())
def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5) -> tuple[Tensor, Tensor, Tensor]:
    x2 = x.float().reshape(-1, x.shape[-1]).contiguous()
    y = torch.empty_like(x2)
    mean, rstd = ops.layernorm_fwd(x2, weight.float().contiguous(), bias.float().contiguous(), eps, y=y)
    return y.view(x.shape), mean, rstd


@layer_norm.register_fake
def _layer_norm_fake(x, weight, bias, eps=1e-5):
    rows = x.numel() // x.shape[-1]
    return x.new_empty(x.shape, dtype=F32), x.new_empty(rows, dtype=F32), x.new_empty(rows, dtype=F32)


def _ln_setup(ctx, inputs, output):
    x, weight, bias, eps = inputs
    ctx.save_for_backward(x, weight, bias, output[1], output[2])


def _ln_bwd(ctx, dy, _dmean, _drstd):
    x, weight, bias, mean, rstd = ctx.saved_tensors
    C = x.shape[-1]
    x2 = x.float().reshape(-1, C).contiguous()
    dx = torch.empty_like(x2)
    dg = torch.zeros(C, device=x.device, dtype=F32)
    db = torch.zeros(C, device=x.device, dtype=F32)
    ops.layernorm_bwd(dy.float().reshape(-1, C).contiguous(), x2, mean, rstd, weight.float().contiguous(),
                      beta=bias.float().contiguous(), dx=dx, dgamma=dg, dbeta=db)
    return dx.view(x.shape).to(x.dtype), dg.to(weight.dtype), db.to(bias.dtype), None


torch.library.register_autograd("ste::layer_norm", _ln_bwd, setup_context=_ln_setup)


# -------------------------------------------------------------------- attention
@torch.library.custom_op("ste::attention", mutates_args=())
def attention(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], rel_E: Optional[Tensor], scale: float,
              rel_left: int = 64, rel_right: int = 8) -> tuple[Tensor, Tensor, Tensor]:
    """q/k/v [B, T, H*64] (bf16 or fp32), key_mask [B, T] (nonzero = valid) or None, rel_E
    [rel_left + rel_right + 1, 64] or None -> (o bf16 [B, T, H*64], lse fp32 [B*H*T], o_lo bf16)."""
    B, T, W = q.shape
    H = W // 64
    qb, kb, vb = (_bf16(t.reshape(B * T, W)) for t in (q, k, v))
    o = torch.empty(B * T, W, device=q.device, dtype=BF16)
    o_lo = torch.empty_like(o)
    lse = torch.empty(B * H * T, device=q.device, dtype=F32)
    km = None if key_mask is None else key_mask.to(torch.int32).reshape(-1).contiguous()
    E = None if rel_E is None else _bf16(rel_E)
    ops.attention_fwd(qb, kb, vb, B=B, T=T, H=H, o=o, lse=lse, key_mask=km, rel_E=E, rel_left=rel_left,
                      rel_right=rel_right, scale=scale, o_lo=o_lo)
    return o.view(B, T, W), lse, o_lo.view(B, T, W)


@attention.register_fake
def _attention_fake(q, k, v, key_mask, rel_E, scale, rel_left=64, rel_right=8):
    B, T, W = q.shape
    return (q.new_empty(B, T, W, dtype=BF16), q.new_empty(B * (W // 64) * T, dtype=F32),
            q.new_empty(B, T, W, dtype=BF16))


def _attn_setup(ctx, inputs, output):
    q, k, v, key_mask, rel_E, scale, rel_left, rel_right = inputs
    o, lse, o_lo = output
    ctx.save_for_backward(q, k, v, key_mask, rel_E, o, lse, o_lo)
    ctx.args = (scale, rel_left, rel_right)


def _attn_bwd(ctx, do, _dlse, _dolo):
    q, k, v, key_mask, rel_E, o, lse, o_lo = ctx.saved_tensors
    scale, rel_left, rel_right = ctx.args
    B, T, W = q.shape
    H = W // 64
    qb, kb, vb = (_bf16(t.reshape(B * T, W)) for t in (q, k, v))
    dq, dk, dv = (torch.empty(B * T, W, device=q.device, dtype=BF16) for _ in range(3))
    delta = torch.empty(B * H * T, device=q.device, dtype=F32)
    km = None if key_mask is None else key_mask.to(torch.int32).reshape(-1).contiguous()
    E = None if rel_E is None else _bf16(rel_E)
    dE = None if rel_E is None else torch.zeros(rel_E.shape, device=q.device, dtype=F32)
    gwork = None if rel_E is None else torch.empty(B * H * T * 80, device=q.device, dtype=F32)
    ops.attention_bwd(qb, kb, vb, o.reshape(B * T, W), lse, _bf16(do.reshape(B * T, W)), dq, dk, dv, B=B, T=T, H=H,
                      delta=delta, key_mask=km, rel_E=E, rel_left=rel_left, rel_right=rel_right, scale=scale, dE=dE,
                      gwork=gwork, o_lo=o_lo.reshape(B * T, W))
    return (dq.view(B, T, W).to(q.dtype), dk.view(B, T, W).to(k.dtype), dv.view(B, T, W).to(v.dtype), None,
            None if dE is None else dE.to(rel_E.dtype), None, None, None)


torch.library.register_autograd("ste::attention", _attn_bwd, setup_context=_attn_setup)


# -------------------------------------------------------------------- pair loss
@torch.library.custom_op("ste::pair_loss", mutates_args=())
def pair_loss(s_pos: Tensor, s_neg: Tensor, alignment_scores: Optional[Tensor], temperature: float = 0.1,
              alignment_weight: float = 0.3, corrupt_gamma: float = 0.35) -> Tensor:
    B = s_pos.shape[0]
    flat = torch.cat([s_pos.float(), s_neg.float()]).contiguous()
    sp, sn = torch.empty(B, device=s_pos.device), torch.empty(B, device=s_pos.device)
    loss = torch.empty(1, device=s_pos.device)
    al = None if alignment_scores is None else alignment_scores.float().contiguous()
    L = 0 if al is None else al.shape[1]
    # ste_pair_loss_fwd reads S[i*ldS + i] / S[i*ldS + off_neg + i]: ldS = 0 makes that flat[i] / flat[B + i]
    _lib.call("ste_pair_loss_fwd", flat.data_ptr(), 0, B, None if al is None else al.data_ptr(), B, L,
              float(temperature), float(alignment_weight), float(corrupt_gamma), sp.data_ptr(), sn.data_ptr(),
              loss.data_ptr(), _lib.stream_ptr())
    return loss.reshape(())


@pair_loss.register_fake
def _pair_loss_fake(s_pos, s_neg, alignment_scores, temperature=0.1, alignment_weight=0.3, corrupt_gamma=0.35):
    return s_pos.new_empty((), dtype=F32)


def _pl_setup(ctx, inputs, output):
    s_pos, s_neg, al, temperature, aw, gamma = inputs
    ctx.save_for_backward(s_pos, s_neg, al)
    ctx.args = (temperature, aw, gamma)


def _pl_bwd(ctx, dloss):
    s_pos, s_neg, al = ctx.saved_tensors
    tau, aw, gamma = ctx.args
    B = s_pos.shape[0]
    dsp, dsn = torch.empty(B, device=s_pos.device), torch.empty(B, device=s_pos.device)
    alf = None if al is None else al.float().contiguous()
    L = 0 if alf is None else alf.shape[1]
    dal = None if alf is None else torch.empty(B, L, device=s_pos.device)
    ops.pair_loss_bwd(s_pos.float().contiguous(), s_neg.float().contiguous(), alf, B, L, tau, aw, gamma,
                      dloss.reshape(1).float().contiguous(), dsp, dsn, dal)
    return (dsp.to(s_pos.dtype), dsn.to(s_neg.dtype), None if dal is None else dal.to(al.dtype), None, None, None)


torch.library.register_autograd("ste::pair_loss", _pl_bwd, setup_context=_pl_setup)


# ------------------------------------------------------------------------ AdamW
@torch.library.custom_op("ste::adamw_", mutates_args=("p", "m", "v", "p_bf16"))
def adamw_(p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Tensor, lr: float, beta1: float, beta2: float,
           eps: float, weight_decay: float, step: int, sumsq: Optional[Tensor] = None, max_norm: float = 1.0) -> None:
    """One AdamW step (torch.optim.AdamW semantics, decoupled decay) on flat fp32 p/g/m/v; g is
    scaled by clip_grad_norm_'s min(1, max_norm/(sqrt(sumsq)+1e-6)) when sumsq (fp64 Σg²) is given;
    p_bf16 receives the bf16 copy of the new p."""
    ops.adamw(p, g, m, v, p_bf16, lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=weight_decay, step=step,
              sumsq_acc=sumsq, max_norm=max_norm)


@adamw_.register_fake
def _adamw_fake(p, g, m, v, p_bf16, lr, beta1, beta2, eps, weight_decay, step, sumsq=None, max_norm=1.0):
    return None


# --------------------------------------------------------------------- retrieval
@torch.library.custom_op("ste::topk_sim", mutates_args=())
def topk_sim(q: Tensor, corpus: Tensor, k: int) -> tuple[Tensor, Tensor]:
    """The k best corpus rows per query by dot product: q [Q, P], corpus [N, P] (fp32 or bf16) ->
    (values fp32 [Q, k], indices int32 [Q, k]), value descending then index ascending."""
    corpus = corpus.contiguous()
    if corpus.dtype not in (BF16, F32):
        corpus = corpus.float()
    return ops.topk_sim(q.float().contiguous(), corpus, int(k))


@topk_sim.register_fake
def _topk_sim_fake(q, corpus, k):
    return q.new_empty(q.shape[0], k, dtype=F32), q.new_empty(q.shape[0], k, dtype=torch.int32)


@torch.library.custom_op("ste::xattn_mq", mutates_args=())
def xattn_mq(q: Tensor, qrow: Tensor, k: Tensor, v: Tensor, mask: Optional[Tensor], C: int, nh: int) -> Tensor:
    """C single-vector queries per clip against that clip's keys/values (forward only): q [U, P],
    qrow int [B*C] (row of q per slot, -1 = empty slot -> zero row), k / v [B*S, P] (bf16, or fp32
    cast to bf16), mask int [B*S] (0 = masked key) or None -> out fp32 [B*C, P]."""
    B = qrow.numel() // int(C)
    if B * int(C) != qrow.numel() or B == 0 or k.shape[0] % B or k.shape != v.shape:
        raise ValueError(f"xattn_mq: qrow of {qrow.numel()} slots, C = {C}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    P = q.shape[-1]
    out = torch.empty(B * int(C), P, device=q.device, dtype=F32)
    m32 = None if mask is None else mask.reshape(-1).to(torch.int32).contiguous()
    ops.xattn_mq_fwd(q.float().contiguous(), qrow.reshape(-1).to(torch.int32).contiguous(), _bf16(k), _bf16(v), m32,
                     B, int(C), k.shape[0] // B, int(nh), out)
    return out


@xattn_mq.register_fake
def _xattn_mq_fake(q, qrow, k, v, mask, C, nh):
    return q.new_empty(qrow.numel(), q.shape[-1], dtype=F32)


def _xattn_seg(q, qrow, pseg, k, v, seg_row, seg_len, tile_first, tile_cnt, nh, ks=None, vs=None):
    """The body of ste::xattn_seg (no scales: k / v to bf16) and ste::xattn_seg_mx8 (k / v as given)."""
    out = torch.empty(qrow.numel(), q.shape[-1], device=q.device, dtype=F32)
    rows = _bf16 if ks is None else (lambda t: t)
    ops.xattn_seg_fwd(q.float().contiguous(), _i32(qrow), _i32(pseg), rows(k), rows(v),
                      seg_row.reshape(-1).to(torch.int64).contiguous(), _i32(seg_len), _i32(tile_first),
                      _i32(tile_cnt), int(nh), out, ks=ks, vs=vs)
    return out


@torch.library.custom_op("ste::xattn_seg", mutates_args=())
def xattn_seg(q: Tensor, qrow: Tensor, pseg: Tensor, k: Tensor, v: Tensor, seg_row: Tensor, seg_len: Tensor,
              tile_first: Tensor, tile_cnt: Tensor, nh: int) -> Tensor:
    """(query, segment) pairs against runs of rows of one K/V buffer (forward only): q [U, P], qrow /
    pseg int [R] (sorted by segment, -1 = empty pair -> zero row), k / v [rows, P] (bf16, or fp32 cast
    to bf16), seg_row int64 [G] / seg_len int [G] (first row and length of a segment), tile_first /
    tile_cnt int [tiles] (retrieval.plan_clip_pairs) -> out fp32 [R, P]."""
    return _xattn_seg(q, qrow, pseg, k, v, seg_row, seg_len, tile_first, tile_cnt, nh)


@xattn_seg.register_fake
def _xattn_seg_fake(q, qrow, pseg, k, v, seg_row, seg_len, tile_first, tile_cnt, nh):
    return q.new_empty(qrow.numel(), q.shape[-1], dtype=F32)


@torch.library.custom_op("ste::xattn_seg_mx8", mutates_args=())
def xattn_seg_mx8(q: Tensor, qrow: Tensor, pseg: Tensor, k: Tensor, v: Tensor, ks: Tensor, vs: Tensor,
                  seg_row: Tensor, seg_len: Tensor, tile_first: Tensor, tile_cnt: Tensor, nh: int) -> Tensor:
    """ste::xattn_seg on MX-fp8 rows (forward only): k / v uint8 [rows, P] (OCP e4m3 bytes, views of one
    buffer), ks / vs uint8 [rows, P/32] (their E8M0 block scales, views of one buffer); the other
    operands and out fp32 [R, P] as ste::xattn_seg.  The same bits as ste::xattn_seg on the dequantised
    rows (ops.mx8_dequant)."""
    return _xattn_seg(q, qrow, pseg, k, v, seg_row, seg_len, tile_first, tile_cnt, nh, ks=ks, vs=vs)


@xattn_seg_mx8.register_fake
def _xattn_seg_mx8_fake(q, qrow, pseg, k, v, ks, vs, seg_row, seg_len, tile_first, tile_cnt, nh):
    return q.new_empty(qrow.numel(), q.shape[-1], dtype=F32)


# -------------------------------------------------------------------- alignment
@torch.library.custom_op("ste::align_matrix", mutates_args=())
def align_matrix(q: Tensor, kv: Tensor, kmask: Optional[Tensor], nh: int) -> tuple[Tensor, Tensor, Tensor]:
    """q [B, L, P], kv [B, T, 2P] = [K | V] (bf16, or fp32 cast to bf16), kmask int [B, T] (0 = padded
    frame) or None -> (matrix fp32 [B, L, T], the head mean of softmax(q_h·k_h/√d); emit fp32
    [B, T, L] = log(max(matrix, FLT_MIN)) frame-major; out bf16 [B, L, P], the attention output).
    Forward only."""
    B, L, P = q.shape
    T = kv.shape[1]
    if kv.shape[0] != B or kv.shape[2] != 2 * P:
        raise ValueError(f"align_matrix: q {tuple(q.shape)}, kv {tuple(kv.shape)}")
    matrix = torch.empty(B, L, T, device=q.device, dtype=F32)
    emit = torch.empty(B, T, L, device=q.device, dtype=F32)
    out = torch.empty(B * L, P, device=q.device, dtype=BF16)
    km = None if kmask is None else kmask.reshape(-1).to(torch.int32).contiguous()
    ops.align_matrix_fwd(_bf16(q.reshape(B * L, P)), _bf16(kv.reshape(B * T, 2 * P)), km, B, L, T, int(nh),
                         matrix=matrix, emit=emit, out=out)
    return matrix, emit, out.view(B, L, P)


@align_matrix.register_fake
def _align_matrix_fake(q, kv, kmask, nh):
    B, L, P = q.shape
    T = kv.shape[1]
    return (q.new_empty(B, L, T, dtype=F32), q.new_empty(B, T, L, dtype=F32), q.new_empty(B, L, P, dtype=BF16))


def _align_matrix_seg(q, qblk, pseg, kv, seg_row, seg_len, Tmax, nh, scales=None):
    """The body of ste::align_matrix_seg (no scales: kv to bf16) and ste::align_matrix_seg_mx8 (kv as given)."""
    U, L, P = q.shape
    R, Tmax = qblk.numel(), int(Tmax)
    matrix = torch.zeros(R, L, Tmax, device=q.device, dtype=F32)
    emit = torch.full((R, Tmax, L), float("-inf"), device=q.device, dtype=F32)
    out = torch.empty(R * L, P, device=q.device, dtype=BF16)
    ops.align_matrix_seg_fwd(_bf16(q.reshape(U * L, P)), _i32(qblk), _i32(pseg), _bf16(kv) if scales is None else kv,
                             seg_row.reshape(-1).to(torch.int64).contiguous(), _i32(seg_len), L, Tmax, int(nh),
                             scales=scales, matrix=matrix, emit=emit, out=out)
    return matrix, emit, out.view(R, L, P)


@torch.library.custom_op("ste::align_matrix_seg", mutates_args=())
def align_matrix_seg(q: Tensor, qblk: Tensor, pseg: Tensor, kv: Tensor, seg_row: Tensor, seg_len: Tensor, Tmax: int,
                     nh: int) -> tuple[Tensor, Tensor, Tensor]:
    """ste::align_matrix for R (query, segment) pairs over runs of rows of one K|V buffer (forward only):
    q [U, L, P], qblk / pseg int [R] (query block and segment of a pair, negative = empty pair), kv
    [rows, 2P] (bf16, or fp32 cast to bf16), seg_row int64 [G] / seg_len int [G] (first row and length
    of a segment), Tmax >= the pairs' segment lengths -> (matrix fp32 [R, L, Tmax], emit fp32
    [R, Tmax, L], out bf16 [R, L, P]).  A pair with F frames fills frames [:F]; the frames beyond,
    and an empty pair's, are 0 in matrix and -inf in emit."""
    P = q.shape[2]
    if kv.dim() != 2 or kv.shape[1] != 2 * P:
        raise ValueError(f"align_matrix_seg: q {tuple(q.shape)}, kv {tuple(kv.shape)}")
    return _align_matrix_seg(q, qblk, pseg, kv, seg_row, seg_len, Tmax, nh)


@align_matrix_seg.register_fake
def _align_matrix_seg_fake(q, qblk, pseg, kv, seg_row, seg_len, Tmax, nh):
    _, L, P = q.shape
    R = qblk.numel()
    return (q.new_empty(R, L, Tmax, dtype=F32), q.new_empty(R, Tmax, L, dtype=F32), q.new_empty(R, L, P, dtype=BF16))


@torch.library.custom_op("ste::align_matrix_seg_mx8", mutates_args=())
def align_matrix_seg_mx8(q: Tensor, qblk: Tensor, pseg: Tensor, kv: Tensor, scales: Tensor, seg_row: Tensor,
                         seg_len: Tensor, Tmax: int, nh: int) -> tuple[Tensor, Tensor, Tensor]:
    """ste::align_matrix_seg on MX-fp8 rows (forward only): kv uint8 [rows, 2P] (OCP e4m3 bytes), scales uint8
    [rows, 2P/32] (their E8M0 block scales); the other operands and (matrix, emit, out) as
    ste::align_matrix_seg.  The same bits as ste::align_matrix_seg on the dequantised rows
    (ops.mx8_dequant)."""
    P = q.shape[2]
    if (kv.dim() != 2 or kv.shape[1] != 2 * P or kv.dtype != torch.uint8 or scales.dtype != torch.uint8
            or scales.shape != (kv.shape[0], 2 * P // 32)):
        raise ValueError(f"align_matrix_seg_mx8: q {tuple(q.shape)}, kv {tuple(kv.shape)} {kv.dtype}, "
                         f"scales {tuple(scales.shape)} {scales.dtype}")
    return _align_matrix_seg(q, qblk, pseg, kv, seg_row, seg_len, Tmax, nh, scales=scales)


@align_matrix_seg_mx8.register_fake
def _align_matrix_seg_mx8_fake(q, qblk, pseg, kv, scales, seg_row, seg_len, Tmax, nh):
    _, L, P = q.shape
    R = qblk.numel()
    return (q.new_empty(R, L, Tmax, dtype=F32), q.new_empty(R, Tmax, L, dtype=F32), q.new_empty(R, L, P, dtype=BF16))


@torch.library.custom_op("ste::align_decode", mutates_args=())
def align_decode(emit: Tensor, ntok: Tensor, nfrm: Tensor) -> tuple[Tensor, Tensor]:
    """Monotone (Viterbi) path through emit fp32 [B, T, L] (frame-major log alignment) for ntok[b]
    tokens over nfrm[b] frames -> (spans int32 [B, L, 2] = (first frame, last frame + 1), -1 past a
    pair's tokens; score fp32 [B]).  Forward only."""
    return ops.align_decode(emit.float().contiguous(), ntok.to(torch.int32).contiguous(),
                            nfrm.to(torch.int32).contiguous())


@align_decode.register_fake
def _align_decode_fake(emit, ntok, nfrm):
    B, _, L = emit.shape
    return emit.new_empty(B, L, 2, dtype=torch.int32), emit.new_empty(B, dtype=F32)


@torch.library.custom_op("ste::align_spot", mutates_args=())
def align_spot(emit: Tensor, ntok: Tensor, nfrm: Tensor, bg: Tensor, lead: int = 0) -> tuple[Tensor, Tensor, Tensor]:
    """Free-endpoint decode of emit fp32 [B, T, L]: where in nfrm[b] frames do the ntok[b] phrase tokens
    of columns lead.. beat a background of bg[b] per frame -> (spans int32 [B, L, 2], -1
    outside the phrase; hit int32 [B, 2]; score fp32 [B], the summed gain over the hit).  Forward only."""
    return ops.align_spot(emit.float().contiguous(), ntok.to(torch.int32).contiguous(),
                          nfrm.to(torch.int32).contiguous(), bg.float().contiguous(), int(lead))


@align_spot.register_fake
def _align_spot_fake(emit, ntok, nfrm, bg, lead=0):
    B, _, L = emit.shape
    return (emit.new_empty(B, L, 2, dtype=torch.int32), emit.new_empty(B, 2, dtype=torch.int32),
            emit.new_empty(B, dtype=F32))


@torch.library.custom_op("ste::attn_pool_seg", mutates_args=())
def attn_pool_seg(t: Tensor, w2: Tensor, b2: Tensor, h: Tensor, seg_row: Tensor, seg_len: Tensor) -> Tensor:
    """AttentivePooling (ref :171-211, after its first Linear + tanh) of G segments of one row buffer
    (DESIGN §23): t [rows, Hh], h [rows, H], both fp32 or both bf16; segment g is rows seg_row[g] ..
    seg_row[g] + seg_len[g] - 1, overlapping freely -> pooled fp32 [G, H], each row the bits of the dense
    pooling of a copy of its rows.  Forward only."""
    return ops.attn_pool_seg_fwd(t.contiguous(), w2.float().reshape(-1).contiguous(), b2.float().reshape(-1).contiguous(),
                                 h.contiguous(), seg_row.reshape(-1).to(torch.int64).contiguous(), _i32(seg_len))


@attn_pool_seg.register_fake
def _attn_pool_seg_fake(t, w2, b2, h, seg_row, seg_len):
    return h.new_empty(seg_len.numel(), h.shape[1], dtype=F32)


OPS = ("fbank", "linear", "layer_norm", "attention", "pair_loss", "adamw_", "resample", "topk_sim", "xattn_mq",
       "xattn_seg", "xattn_seg_mx8", "align_matrix", "align_matrix_seg", "align_matrix_seg_mx8", "align_decode",
       "align_spot", "attn_pool_seg")
