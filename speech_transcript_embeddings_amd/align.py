"""WordLevelAlignmentModule forward/backward on the HIP kernels (config 4).

ref = /root/reference/training/trainer_unfreeze.py:214-310, invoked at :550-558 on the
positive transcript: text/audio projections -> 4-head text->audio attention with the
audio key-padding mask -> out_proj -> LN(text_hidden + output_projection(.)) ->
confidence MLP (Linear -> ReLU -> Linear) -> scores * text_mask = model.last_alignment_scores
(fed to AlignmentAwareInfoNCE's per-sample weighting, ref:730-734).  The training path never
uses the head-averaged alignment matrix the reference also returns, so it does not materialise it;
the forward-only route align_infer does (ste_align_matrix_fwd), for model.align's word timestamps.
"""
from __future__ import annotations

import torch

from . import _lib, ops
from ._lib import ACT_RELU, ACT_RELU_BWD

BF16, F32 = torch.bfloat16, torch.float32
PRE = "word_level_alignment."


def align_forward(eng, th, thb_pos, ahb, b, L, T, ctx, train, seed, hs):
    s = eng.s
    m = eng.m
    P = m.projection_dim
    nh = m.word_level_alignment.num_heads
    p_drop = m.dropout if train else 0.0
    W = s.w(PRE + "alignment_attention.in_proj_weight")
    bW = s.p(PRE + "alignment_attention.in_proj_bias")
    tp = ops.linear(thb_pos, s.w(PRE + "text_projection.weight"), s.p(PRE + "text_projection.bias"), out_bf16=True)
    ap = ops.linear(ahb, s.w(PRE + "audio_projection.weight"), s.p(PRE + "audio_projection.bias"), out_bf16=True)
    q = ops.linear(tp, W[:P], bW[:P], out_bf16=True)
    kv = ops.linear(ap, W[P:], bW[P:], out_bf16=True)
    probs = eng._e(b * nh * L * T)
    att = eng._e(b * L, P, dtype=BF16)
    ops.align_attn_fwd(q, kv, ctx["a_mask32"], b, L, T, nh, probs, att, drop_p=p_drop, seed=seed)
    o2 = ops.linear(att, s.w(PRE + "alignment_attention.out_proj.weight"),
                    s.p(PRE + "alignment_attention.out_proj.bias"), out_bf16=True)
    y = ops.linear(o2, s.w(PRE + "output_projection.weight"), s.p(PRE + "output_projection.bias"),
                   residual=th[: b * L])
    aligned_b = eng._e(b * L, P, dtype=BF16)
    st = eng._ln(y, PRE + "layer_norm", 1e-5, yb=aligned_b)
    c1 = ops.linear(aligned_b, s.w(PRE + "alignment_confidence.0.weight"), s.p(PRE + "alignment_confidence.0.bias"),
                    act=ACT_RELU, out_bf16=True)
    tmask = eng._e(b * L)
    _lib.call("ste_mask_i64_to_f32", ctx["_tmask_i64"].data_ptr(), tmask.data_ptr(), None, b * L, _lib.stream_ptr())
    scores = ops.linear(c1, s.w(PRE + "alignment_confidence.2.weight"), s.p(PRE + "alignment_confidence.2.bias"),
                        row_scale=tmask)
    hs["align"] = dict(tp=tp, ap=ap, q=q, kv=kv, probs=probs, att=att, o2=o2, y=y, st=st, aligned_b=aligned_b, c1=c1,
                       tmask=tmask, p=p_drop, seed=seed, b=b, L=L, T=T, nh=nh)
    return scores.view(b, L)


def align_infer(eng, th, thb, ahb, b, L, T, ctx, *, want_matrix=False, want_emit=True):
    """The forward-only route: align_forward's eval arithmetic with the attention on
    ste_align_matrix_fwd, which also gives what the reference's forward returns next to the
    confidence — the head-averaged alignment matrix (ref:295) — and its frame-major log for
    ops.align_decode.  No [b, nh, L, T] probabilities buffer is allocated.
    -> (scores fp32 [b, L], matrix fp32 [b, L, T] or None, emit fp32 [b, T, L] or None)."""
    P = eng.m.projection_dim
    nh = eng.m.word_level_alignment.num_heads
    q = text_queries(eng, thb)
    kv = audio_kv(eng, ahb)
    matrix = eng._e(b, L, T) if want_matrix else None
    emit = eng._e(b, T, L) if want_emit else None
    att = eng._e(b * L, P, dtype=BF16)
    ops.align_matrix_fwd(q, kv, ctx["a_mask32"], b, L, T, nh, matrix=matrix, emit=emit, out=att)
    return confidence_tail(eng, att, th[: b * L], ctx["_tmask_i64"], b * L).view(b, L), matrix, emit


def text_queries(eng, thb):
    """The head's bf16 queries [rows, P] of bf16 text hidden rows: text_projection, then the query
    third of the attention's in_proj."""
    s = eng.s
    P = eng.m.projection_dim
    tp = ops.linear(thb, s.w(PRE + "text_projection.weight"), s.p(PRE + "text_projection.bias"), out_bf16=True)
    return ops.linear(tp, s.w(PRE + "alignment_attention.in_proj_weight")[:P],
                      s.p(PRE + "alignment_attention.in_proj_bias")[:P], out_bf16=True)


def audio_kv(eng, ahb):
    """The head's bf16 K|V rows [rows, 2P] of bf16 audio hidden rows: audio_projection, then the key
    and value thirds of in_proj in one GEMM.  A row depends on its own frame alone, which is what
    lets an AudioStateStore keep the rows of a clip's valid frames."""
    s = eng.s
    P = eng.m.projection_dim
    ap = ops.linear(ahb, s.w(PRE + "audio_projection.weight"), s.p(PRE + "audio_projection.bias"), out_bf16=True)
    return ops.linear(ap, s.w(PRE + "alignment_attention.in_proj_weight")[P:],
                      s.p(PRE + "alignment_attention.in_proj_bias")[P:], out_bf16=True)


def confidence_tail(eng, att, th_rows, tmask_i64, n):
    """What follows the attention output att bf16 [n, P]: out_proj -> LN(text hidden + output_projection)
    -> confidence MLP -> x text mask.  th_rows fp32 [n, Ht] are the rows' text hidden states,
    tmask_i64 their int64 mask (its first n entries).  -> scores fp32 [n]."""
    s = eng.s
    P = eng.m.projection_dim
    o2 = ops.linear(att, s.w(PRE + "alignment_attention.out_proj.weight"),
                    s.p(PRE + "alignment_attention.out_proj.bias"), out_bf16=True)
    y = ops.linear(o2, s.w(PRE + "output_projection.weight"), s.p(PRE + "output_projection.bias"),
                   residual=th_rows)
    aligned_b = eng._e(n, P, dtype=BF16)
    eng._ln(y, PRE + "layer_norm", 1e-5, yb=aligned_b)
    c1 = ops.linear(aligned_b, s.w(PRE + "alignment_confidence.0.weight"), s.p(PRE + "alignment_confidence.0.bias"),
                    act=ACT_RELU, out_bf16=True)
    tmask = eng._e(n)
    _lib.call("ste_mask_i64_to_f32", tmask_i64.data_ptr(), tmask.data_ptr(), None, n, _lib.stream_ptr())
    scores = ops.linear(c1, s.w(PRE + "alignment_confidence.2.weight"), s.p(PRE + "alignment_confidence.2.bias"),
                        row_scale=tmask)
    return scores.view(n)


def hit_spans(token_spans, ntok, lead=1, trail=1):
    """The phrase's span inside each pair's decoded path: from the first frame of token `lead` to the
    end of token n - 1 - trail, n = ntok.  With lead = trail = 1 that is the transcript without its
    <s> and </s>, which absorb the audio before and after the phrase.  token_spans int
    [..., L, 2], ntok int [...] -> int32 [..., 2]; (-1, -1) when n < lead + trail + 1 or the pair has
    no path (its spans are -1).  Pure torch, any device."""
    if lead < 0 or trail < 0:
        raise ValueError(f"lead and trail count tokens, got {lead}, {trail}")
    L = token_spans.shape[-2]
    n = ntok.to(token_spans.device, torch.int64)
    ok = (n >= lead + trail + 1) & (n <= L)
    first = torch.full_like(n, min(lead, L - 1)).unsqueeze(-1)
    last = (n - 1 - trail).clamp(0, L - 1).unsqueeze(-1)
    start = token_spans[..., 0].to(torch.int64).gather(-1, first).squeeze(-1)
    end = token_spans[..., 1].to(torch.int64).gather(-1, last).squeeze(-1)
    ok = ok & (start >= 0) & (end >= 0)
    neg = torch.full_like(start, -1)
    return torch.stack([torch.where(ok, start, neg), torch.where(ok, end, neg)], -1).to(torch.int32)


def words_from_tokens(token_spans, token_scores, word_ids):
    """Token spans -> word spans, on the tensors' device (plain torch scatter-reduce).
    token_spans int [B, L, 2] ((-1, -1) for a token without a span), token_scores [B, L], word_ids
    int [B, L] as a fast tokenizer's word_ids() gives them, -1 for special and padding tokens.
    -> (word_spans int32 [B, W, 2], word_scores fp32 [B, W]), W = max word id + 1: a word's span is
    the min start to the max end over its tokens, its score the mean of their confidences; a word
    id no token carries gives (-1, -1) and score 0."""
    B, L = word_ids.shape
    wid = word_ids.to(token_spans.device, torch.int64)
    W = max(int(wid.max().item()) + 1, 0) if wid.numel() else 0
    start, end = token_spans[..., 0].to(torch.int64), token_spans[..., 1].to(torch.int64)
    valid = (wid >= 0) & (start >= 0)
    idx = torch.where(valid, wid, torch.full_like(wid, W))          # everything else to a spare column
    big = torch.iinfo(torch.int32).max
    ws = torch.full((B, W + 1), big, dtype=torch.int64, device=wid.device).scatter_reduce(1, idx, start, "amin")
    we = torch.full((B, W + 1), -1, dtype=torch.int64, device=wid.device).scatter_reduce(1, idx, end, "amax")
    cnt = torch.zeros(B, W + 1, dtype=F32, device=wid.device).scatter_add(1, idx, valid.to(F32))
    tot = torch.zeros(B, W + 1, dtype=F32, device=wid.device).scatter_add(1, idx, token_scores.to(F32) * valid)
    live = cnt[:, :W] > 0
    spans = torch.stack([torch.where(live, ws[:, :W], -1), torch.where(live, we[:, :W], -1)], -1).to(torch.int32)
    return spans, torch.where(live, tot[:, :W] / cnt[:, :W].clamp(min=1), 0.0)


def align_backward(eng, d_align, hs, ctx, dth, dah):
    s = eng.s
    m = eng.m
    P = m.projection_dim
    a = hs["align"]
    b, L, T, nh = a["b"], a["L"], a["T"], a["nh"]
    # scores = mlp(aligned) * text_mask  ->  d(mlp out) = d_align * text_mask
    dsc = eng._e(b * L)
    ops.copy2d(dsc, d_align.reshape(b * L))
    _lib.call("ste_scale_rows", dsc.data_ptr(), a["tmask"].data_ptr(), b * L, 1, 1, _lib.stream_ptr())
    # confidence head: Linear(P/2 -> 1) backward through the ReLU, then Linear(P -> P/2)
    c1 = a["c1"]
    dc1 = eng._e(*c1.shape, dtype=BF16)
    g2 = s.g(PRE + "alignment_confidence.2.weight")
    ops.rank1_bwd(dsc, s.p(PRE + "alignment_confidence.2.weight").view(-1), c1, ACT_RELU_BWD, dc1,
                  None if g2 is None else g2.view(-1), s.g(PRE + "alignment_confidence.2.bias"))
    dal = ops.linear_dx(dc1, s.w(PRE + "alignment_confidence.0.weight"))
    eng._dw(dc1, a["aligned_b"], PRE + "alignment_confidence.0.weight")
    eng._db(dc1, PRE + "alignment_confidence.0.bias")
    # LN(text_hidden + output_projection(o2))
    dy = eng._e(b * L, P)
    dyb = eng._e(b * L, P, dtype=BF16)
    eng._ln_bwd(dal, a["y"], a["st"], PRE + "layer_norm", dx=dy, dxb=dyb, dsum=s.g(PRE + "output_projection.bias"))
    ops.axpby(dth[: b * L], dy)
    do2 = ops.linear_dx(dyb, s.w(PRE + "output_projection.weight"), out_bf16=True)
    eng._dw(dyb, a["o2"], PRE + "output_projection.weight")
    datt = ops.linear_dx(do2, s.w(PRE + "alignment_attention.out_proj.weight"), out_bf16=True)
    eng._dw(do2, a["att"], PRE + "alignment_attention.out_proj.weight")
    eng._db(do2, PRE + "alignment_attention.out_proj.bias")
    dq = eng._e(b * L, P, dtype=BF16)
    dkv = eng._e(b * T, 2 * P)
    dsbuf = eng._e(b * nh * L * T)
    ops.align_attn_bwd(a["q"], a["kv"], a["probs"], datt, b, L, T, nh, dsbuf, dq, dkv, drop_p=a["p"], seed=a["seed"])
    W = s.w(PRE + "alignment_attention.in_proj_weight")
    gW = s.g(PRE + "alignment_attention.in_proj_weight")
    gB = s.g(PRE + "alignment_attention.in_proj_bias")
    dtp = ops.linear_dx(dq, W[:P], out_bf16=True)
    if gW is not None:
        ops.linear_dw(dq, a["tp"], out=gW[:P], beta=1.0, ws=eng.ws)
        ops.colsum(dq, gB[:P])
    dkvb = ops.cast_bf16(dkv, eng._e(b * T, 2 * P, dtype=BF16))
    dap = ops.linear_dx(dkvb, W[P:], out_bf16=True)
    if gW is not None:
        ops.linear_dw(dkvb, a["ap"], out=gW[P:], beta=1.0, ws=eng.ws)
        ops.colsum(dkv, gB[P:])
    ops.linear_dx(dtp, s.w(PRE + "text_projection.weight"), out=dth[: b * L], beta=1.0)
    eng._dw(dtp, ctx["_thb"][: b * L], PRE + "text_projection.weight")
    eng._db(dtp, PRE + "text_projection.bias")
    ops.linear_dx(dap, s.w(PRE + "audio_projection.weight"), out=dah, beta=1.0)
    eng._dw(dap, ctx["_ahb"], PRE + "audio_projection.weight")
    eng._db(dap, PRE + "audio_projection.bias")


