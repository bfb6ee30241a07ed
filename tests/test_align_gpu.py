"""Word timestamps end to end (model.align / Engine.align_pairs / align.align_infer) on
the mini alignment model of the golden fixtures: P = 128, 4 alignment heads (d = 32), B = 2 clips of
T = 49 frames (49 and 39 valid), L = 12 (12 and 9 tokens).

Tolerances.  Confidence scores: within 1.5·e_old + 1e-4 of the float64 oracle, e_old the distance of
the existing no_grad model(batch).last_alignment_scores to the same oracle on the same batch (the
rule of tests/test_rerank_gpu.py).  Matrix: max |matrix - float64 reference on the head's own bf16
q / kv| at most 1.5 x that of the head mean of ste_align_attn_fwd's probabilities, plus 1e-6 (the
running head sum adds one fp32 rounding per head).  Spans and path scores: exact.  Every test
prints its figures.
"""
import numpy as np
import pytest
import torch

from kref_align import align_matrix_ref, viterbi_batch_ref
from oracle import ref_model as R
from test_model_gpu import batch_of, load, mini_model, oracle_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
PRE = "word_level_alignment."


@pytest.fixture(scope="module")
def fx():
    """The model, the batch, the training path's scores, the float64 oracle's, and align()'s result,
    computed once."""
    meta, z = load("align")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    with torch.no_grad():
        model(batch)
        s_old = model.last_alignment_scores.double().cpu()
    p = {n: v.detach().double() for n, v in oracle_params(meta).items()}
    cb = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items()}
    with torch.no_grad():
        s_ref = R.compute_pos_neg_embeddings(p, cb, R.mini_cfg(meta))[3]
    res = _align(model, batch, return_matrix=True)
    return dict(meta=meta, model=model, batch=batch, s_old=s_old, s_ref=s_ref, res=res,
                e_old=(s_old - s_ref).abs().max().item())


def _align(model, b, **kw):
    return model.align(b["input_values"], b["attention_mask_audio"], b["input_ids_pos"], b["attention_mask_pos"], **kw)


def test_result_shapes_and_dtypes(fx):
    r, m = fx["res"], fx["model"]
    assert set(r) == {"token_spans", "token_seconds", "scores", "path_score", "matrix"}
    assert r["token_spans"].shape == (2, 12, 2) and r["token_spans"].dtype == torch.int32
    assert r["token_seconds"].shape == (2, 12, 2) and r["token_seconds"].dtype == torch.float32
    assert r["scores"].shape == (2, 12) and r["path_score"].shape == (2,) and r["matrix"].shape == (2, 12, 49)
    assert not any(v.requires_grad for v in r.values())
    assert m.engine.frame_seconds == 0.02
    sp = r["token_spans"].cpu()
    assert torch.equal(r["token_seconds"].cpu(), torch.where(sp < 0, -1.0, sp.float() * 0.02))
    # the spans of a pair tile its valid frames; padded tokens are (-1, -1)
    for b, (n, F) in enumerate(((12, 49), (9, 39))):
        assert sp[b, 0, 0] == 0 and sp[b, n - 1, 1] == F and torch.equal(sp[b, 1:n, 0], sp[b, :n - 1, 1])
        assert bool((sp[b, :n, 1] > sp[b, :n, 0]).all()) and bool((sp[b, n:] == -1).all())
    assert "matrix" not in _align(m, fx["batch"])


def test_scores_match_oracle(fx):
    err = (fx["res"]["scores"].double().cpu() - fx["s_ref"]).abs().max().item()
    tol = 1.5 * fx["e_old"] + 1e-4
    print(f"align().scores vs float64 oracle: {err:.3e}; last_alignment_scores vs oracle e_old = {fx['e_old']:.3e}; "
          f"tolerance {tol:.3e}")
    assert err <= tol


def _head_operands(model, batch):
    """The head's bf16 q / kv recomputed from the hidden states encode_* return."""
    from speech_transcript_embeddings_amd import ops
    s = model.store
    with torch.no_grad():
        _, ah = model.encode_audio(batch["input_values"], batch["attention_mask_audio"])
        _, th = model.encode_text(batch["input_ids_pos"], batch["attention_mask_pos"])
    B, L, Ht = th.shape
    T, Ha = ah.shape[1:]
    P = model.projection_dim
    thb = ops.cast_bf16(th.reshape(B * L, Ht).contiguous(), torch.empty(B * L, Ht, device=DEV, dtype=BF16))
    ahb = ops.cast_bf16(ah.reshape(B * T, Ha).contiguous(), torch.empty(B * T, Ha, device=DEV, dtype=BF16))
    W, bW = s.w(PRE + "alignment_attention.in_proj_weight"), s.p(PRE + "alignment_attention.in_proj_bias")
    tp = ops.linear(thb, s.w(PRE + "text_projection.weight"), s.p(PRE + "text_projection.bias"), out_bf16=True)
    ap = ops.linear(ahb, s.w(PRE + "audio_projection.weight"), s.p(PRE + "audio_projection.bias"), out_bf16=True)
    q = ops.linear(tp, W[:P], bW[:P], out_bf16=True)
    kv = ops.linear(ap, W[P:], bW[P:], out_bf16=True)
    return q, kv, B, L, T, P


def test_matrix_against_both_yardsticks(fx):
    from speech_transcript_embeddings_amd import ops
    model, batch = fx["model"], fx["batch"]
    q, kv, B, L, T, P = _head_operands(model, batch)
    nh = model.word_level_alignment.num_heads
    km = batch["attention_mask_audio"].to(torch.int32).reshape(-1).contiguous()
    mref, _ = align_matrix_ref(q, kv, km, B, L, T, P, nh)
    probs = torch.empty(B * nh * L * T, device=DEV)
    ops.align_attn_fwd(q, kv, km, B, L, T, nh, probs, torch.empty(B * L, P, device=DEV, dtype=BF16))
    d_old = (probs.view(B, nh, L, T).double().cpu().mean(1) - mref).abs().max().item()
    got = fx["res"]["matrix"]
    d_new = (got.double().cpu() - mref).abs().max().item()
    print(f"matrix vs float64: new kernel {d_new:.3e}, head mean of align_attn_fwd's probs {d_old:.3e}, "
          f"bound {1.5 * d_old + 1e-6:.3e}")
    assert d_new <= 1.5 * d_old + 1e-6
    direct = torch.empty(B, L, T, device=DEV)
    ops.align_matrix_fwd(q, kv, km, B, L, T, nh, matrix=direct)
    assert torch.equal(direct, got)                       # align() ran the head on exactly these operands
    assert float(got[1, :, 39:].abs().max()) == 0.0 and float((got.sum(-1) - 1).abs().max()) <= 1e-5
    # the spans are the decode of this matrix
    emit = got.double().cpu().clamp_min(float(np.finfo(np.float32).tiny)).log().float().transpose(1, 2).numpy()
    rs, _ = viterbi_batch_ref(emit, [12, 9], [49, 39], L)
    agree = float((torch.from_numpy(rs) == fx["res"]["token_spans"].cpu()).float().mean())
    print(f"spans vs numpy decode of the float64 log of the returned matrix: {agree:.3f} agree")


def _planted_model(meta):
    """The mini model with the head's projections set to pass its inputs through: q = text hidden,
    k = audio hidden (first P columns), biases zero."""
    model = mini_model(meta)
    model.eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    P = model.projection_dim
    for name in ("text_projection", "audio_projection"):
        w = sd[PRE + name + ".weight"]                     # [P, hidden]: the rectangular identity
        w.copy_(torch.eye(P, w.shape[1]))
        sd[PRE + name + ".bias"].zero_()
    sd[PRE + "alignment_attention.in_proj_weight"].copy_(torch.eye(P).repeat(3, 1))
    sd[PRE + "alignment_attention.in_proj_bias"].zero_()
    model.load_state_dict(sd)
    return model


def test_planted_alignment_comes_back_exactly(fx):
    """Token l's query is 8·e_l and the keys of its frames [b_l, b_{l+1}) are 8·e_l: head 0 scores
    64/sqrt(32) on the planted cells and 0 elsewhere, the other heads are uniform, so every frame's
    best token is its planted one and the monotone path through them is the planted path."""
    model = _planted_model(fx["meta"])
    batch = fx["batch"]
    B, L, T = 2, 12, 49
    Ht, Ha = model.text_hidden_dim, model.audio_hidden_dim
    assert min(Ht, Ha, model.projection_dim) >= L
    bounds = [[0, 3, 4, 9, 15, 16, 22, 30, 31, 35, 40, 44, 49], [0, 1, 6, 7, 13, 20, 21, 29, 33, 39]]
    th, ah = torch.zeros(B, L, Ht), torch.zeros(B, T, Ha)
    for b, bd in enumerate(bounds):
        for tok in range(len(bd) - 1):
            th[b, tok, tok] = 8.0
            ah[b, bd[tok]:bd[tok + 1], tok] = 8.0
    word_ids = torch.tensor([[-1, 0, 0, 1, 2, 2, 2, 4, 4, 5, 6, -1], [-1, 0, 1, 1, 1, 2, 3, 3, -1, -1, -1, -1]])
    r = model.align(batch["input_values"], batch["attention_mask_audio"], batch["input_ids_pos"],
                    batch["attention_mask_pos"], word_ids=word_ids.to(DEV), audio_encoded=(None, ah.to(DEV)),
                    text_encoded=(None, th.to(DEV)))
    sp = r["token_spans"].cpu()
    for b, bd in enumerate(bounds):
        n = len(bd) - 1
        assert sp[b, :n].tolist() == [[bd[i], bd[i + 1]] for i in range(n)], b
        assert bool((sp[b, n:] == -1).all())
    ws = r["word_spans"].cpu()
    assert ws.shape == (2, 7, 2) and r["word_scores"].shape == (2, 7) and r["word_seconds"].shape == (2, 7, 2)
    assert ws[0].tolist() == [[3, 9], [9, 15], [15, 30], [-1, -1], [30, 35], [35, 40], [40, 44]]   # word 3: a gap
    assert ws[1].tolist() == [[1, 6], [6, 20], [20, 21], [21, 33], [-1, -1], [-1, -1], [-1, -1]]
    sc = r["scores"].cpu()
    assert abs(float(r["word_scores"][0, 2]) - float(sc[0, 4:7].mean())) < 1e-6
    assert torch.equal(r["word_seconds"].cpu(), torch.where(ws < 0, -1.0, ws.float() * 0.02))


def test_ragged_batch_equals_each_pair_alone(fx):
    """3 clips of 49, 39 and 25 valid frames against transcripts of 1, 4 and 10 tokens: spans and
    path_score of each pair are the bits of the same pair run alone; padded rows are (-1, -1)."""
    model, b0 = fx["model"], fx["batch"]
    pick = [0, 1, 0]
    iv = b0["input_values"][pick].contiguous()
    am = b0["attention_mask_audio"][pick].clone()
    am[2, 25:] = 0
    ids = b0["input_ids_pos"][[0, 0, 0]].contiguous()
    tm = torch.zeros_like(b0["attention_mask_pos"][[0, 0, 0]])
    ntok = [1, 4, 10]
    for b, n in enumerate(ntok):
        tm[b, :n] = 1
    full = model.align(iv, am, ids, tm)
    sp = full["token_spans"].cpu()
    for b, (n, F) in enumerate(zip(ntok, (49, 39, 25))):
        assert sp[b, 0, 0] == 0 and sp[b, n - 1, 1] == F and bool((sp[b, n:] == -1).all())
        one = model.align(iv[b:b + 1], am[b:b + 1], ids[b:b + 1], tm[b:b + 1])
        same = torch.equal(one["token_spans"][0], full["token_spans"][b])
        print(f"pair {b} (n = {n}, F = {F}): path_score alone {float(one['path_score'][0])!r}, "
              f"in the batch {float(full['path_score'][b])!r}, spans equal: {same}")
        assert same and torch.equal(one["path_score"][0], full["path_score"][b])


def test_encoded_reuse_is_bitwise(fx):
    model, b = fx["model"], fx["batch"]
    with torch.no_grad():
        a_enc = model.encode_audio(b["input_values"], b["attention_mask_audio"])
        t_enc = model.encode_text(b["input_ids_pos"], b["attention_mask_pos"])
    r = _align(model, b, return_matrix=True, audio_encoded=a_enc, text_encoded=t_enc)
    for k, v in fx["res"].items():
        assert torch.equal(r[k], v), k


def test_errors_and_side_effects(fx):
    model, b = fx["model"], fx["batch"]
    meta, _ = load("noalign")
    with pytest.raises(ValueError, match="use_word_alignment"):
        _align(mini_model(meta), b)
    holed = b["attention_mask_pos"].clone()
    holed[0, 3] = 0
    with pytest.raises(ValueError, match="prefix"):
        model.align(b["input_values"], b["attention_mask_audio"], b["input_ids_pos"], holed)
    holed = b["attention_mask_audio"].clone()
    holed[1, 0] = 0
    with pytest.raises(ValueError, match="prefix"):
        model.align(b["input_values"], holed, b["input_ids_pos"], b["attention_mask_pos"])
    model.train()
    try:
        r = _align(model, b)
        assert model.training
    finally:
        model.eval()
    assert torch.equal(r["token_spans"], fx["res"]["token_spans"]) and torch.equal(r["scores"], fx["res"]["scores"])


def test_no_probs_sized_allocation(fx):
    """The head call at (B, L, T) = (2, 64, 2048): align_infer's peak memory stays below the training
    path's head forward, which allocates the [B, nh, L, T] probabilities (4 MiB here)."""
    from speech_transcript_embeddings_amd.align import align_forward, align_infer
    model = fx["model"]
    eng = model.engine
    B, L, T = 2, 64, 2048
    torch.manual_seed(0)
    th = torch.randn(B * L, model.text_hidden_dim, device=DEV)
    thb = th.bfloat16()
    ahb = torch.randn(B * T, model.audio_hidden_dim, device=DEV).bfloat16()
    ctx = {"a_mask32": torch.ones(B * T, dtype=torch.int32, device=DEV),
           "_tmask_i64": torch.ones(B, L, dtype=torch.int64, device=DEV)}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    model.store.sync_shadow()
    new, (s_new, m_new, e_new) = peak(lambda: align_infer(eng, th, thb, ahb, B, L, T, ctx, want_matrix=True,
                                                          want_emit=True))
    old, s_old = peak(lambda: align_forward(eng, th, thb, ahb, B, L, T, ctx, False, 0, {}))
    print(f"peak bytes of the head call: align_infer {new}, align_forward {old}, probs {B * 4 * L * T * 4}")
    assert new < old
    assert torch.equal(s_new, s_old)          # the same attention output, so the same confidence
    assert m_new.shape == (B, L, T) and e_new.shape == (B, T, L)
