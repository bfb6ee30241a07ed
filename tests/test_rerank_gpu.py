"""The fused pair score for reranking (Engine.score_pairs / model.score_candidates / retrieval.rerank,
DESIGN §15) on the mini model of the golden fixtures: P = 128, 8 heads, B = 2 clips of T = 49 frames
(one ragged), L = 12.

The tolerance against the float64 oracle is taken from the existing forward's own distance to the
same oracle: e_old = max |(s_pos, s_neg) of model(batch) - oracle|, and the new scores must stay
within 1.5·e_old + 1e-4 (the margin of 1.5 is for the one extra bf16 rounding of the probabilities in
the text->audio attention).

Measured on an MI355X: e_old = 7.24e-4; score_candidates against the oracle 9.15e-4 (tolerance
1.19e-3); audio_context=0 against model(batch) 6.3e-5 and against the oracle 7.87e-4.  Each test
prints its figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as R
from test_model_gpu import batch_of, load, mini_model, oracle_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")


@pytest.fixture(scope="module")
def fx():
    """The model, the batch, the U = 4 distinct transcripts (clean 0, 1 then corrupted 2, 3), the
    training forward's (s_pos, s_neg) and the float64 oracle's pieces, computed once."""
    meta, z = load("noalign")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]])
    mask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]])
    with torch.no_grad():
        tpn, tnn, an = model(batch)
        s_old = torch.stack([(an * tpn).sum(1), (an * tnn).sum(1)], 1).double().cpu()      # [B, 2]
    cfg = R.mini_cfg(meta)
    p = {n: v.detach().double() for n, v in oracle_params(meta).items()}
    cb = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items()}
    with torch.no_grad():
        otp, otn, oan, _ = R.compute_pos_neg_embeddings(p, cb, cfg)
        s_ref = torch.stack([(oan * otp).sum(1), (oan * otn).sum(1)], 1)
        tp, th = R.encode_text(p, ids.cpu(), mask.cpu(), cfg)
        ap, ah = R.encode_audio(p, cb["input_values"], cb["attention_mask_audio"], cfg)

    def pair(b, u):
        with torch.no_grad():
            tf, af = R.apply_cross_modal(p, tp[u:u + 1], th[u:u + 1], mask.cpu()[u:u + 1], ap[b:b + 1], ah[b:b + 1],
                                         cb["attention_mask_audio"][b:b + 1], cfg)
        return float((F.normalize(tf, dim=1) * F.normalize(af, dim=1)).sum())

    e_old = (s_old - s_ref).abs().max().item()
    return dict(meta=meta, model=model, batch=batch, ids=ids, mask=mask, s_old=s_old, s_ref=s_ref, pair=pair,
                e_old=e_old)


def _scores(fx, cand, **kw):
    b = fx["batch"]
    return fx["model"].score_candidates(b["input_values"], b["attention_mask_audio"], fx["ids"], fx["mask"],
                                        torch.tensor(cand, device=DEV), **kw)


def test_score_candidates_matches_oracle(fx):
    """Pair form against R.encode_* + R.apply_cross_modal per (clip, candidate) pair in float64."""
    cand = [[0, 2, 1, 3], [3, -1, 1, 1]]
    got = _scores(fx, cand)
    assert got.shape == (2, 4) and got.dtype == torch.float32 and not got.requires_grad
    got = got.double().cpu()
    err = 0.0
    for b, row in enumerate(cand):
        for c, u in enumerate(row):
            if u < 0:
                assert got[b, c].item() == NEG
            else:
                err = max(err, abs(got[b, c].item() - fx["pair"](b, u)))
    tol = 1.5 * fx["e_old"] + 1e-4
    print(f"score_candidates vs float64 oracle: max error {err:.3e}; model(batch) vs oracle e_old = "
          f"{fx['e_old']:.3e}; tolerance {tol:.3e}")
    assert err <= tol


def test_audio_context_reproduces_training_forward(fx):
    """candidates [clean, corrupted] with audio_context=0 are the training forward's (s_pos, s_neg)."""
    got = _scores(fx, [[0, 2], [1, 3]], audio_context=0).double().cpu()
    err_old = (got - fx["s_old"]).abs().max().item()
    err_ref = (got - fx["s_ref"]).abs().max().item()
    tol = 1.5 * fx["e_old"] + 1e-4
    print(f"audio_context=0 vs model(batch): {err_old:.3e}; vs float64 oracle: {err_ref:.3e}; tolerance {tol:.3e}")
    assert err_old <= tol and err_ref <= tol
    # in the pair form the clean column is the same pair, the corrupted column is fused differently
    pair = _scores(fx, [[0, 2], [1, 3]]).double().cpu()
    assert torch.equal(pair[:, 0], got[:, 0])


def test_column_permutation_is_bitwise(fx):
    cand = torch.tensor([[0, 2, 1, 3], [3, -1, 1, 1]])
    base = _scores(fx, cand.tolist())
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
        got = _scores(fx, cand[:, perm].tolist())
        assert torch.equal(got, base[:, perm]), perm
    assert base[1, 1].item() == NEG and torch.isfinite(base[0]).all()
    assert torch.equal(base[1, 2], base[1, 3])          # the same transcript twice in a row


def test_without_fusion_is_the_indexed_cosine(fx):
    from speech_transcript_embeddings_amd import embed_audio, embed_texts, ops
    model = mini_model(fx["meta"], use_cross_modal=False)
    model.eval()
    b = fx["batch"]
    cand = [[0, 2, 1, 3], [3, -1, 1, 1]]
    got = model.score_candidates(b["input_values"], b["attention_mask_audio"], fx["ids"], fx["mask"],
                                 torch.tensor(cand, device=DEV))
    A = embed_audio(model, b["input_values"], b["attention_mask_audio"])
    T = embed_texts(model, fx["ids"], fx["mask"])
    S = torch.empty(A.shape[0], T.shape[0], device=DEV)
    ops.similarity(A, T, S)
    for r, row in enumerate(cand):
        for c, u in enumerate(row):
            assert got[r, c].item() == (S[r, u].item() if u >= 0 else NEG), (r, c)


def test_candidates_out_of_range_raise(fx):
    with pytest.raises(ValueError):
        _scores(fx, [[0, 4], [1, 3]])
    with pytest.raises(ValueError):
        _scores(fx, [[0, -2], [1, 3]])


def _two_batches(fx):
    b1 = fx["batch"]
    # the batches of the end-to-end retrieval test: the corrupted transcripts as clean ones, clips reversed
    b2 = dict(b1, input_ids_pos=b1["input_ids_neg"], attention_mask_pos=b1["attention_mask_neg"],
              input_values=b1["input_values"].flip(0).contiguous(),
              attention_mask_audio=b1["attention_mask_audio"].flip(0).contiguous())
    cpu = lambda b: {k: v.cpu() for k, v in b.items()}                                 # noqa: E731
    return b1, b2, cpu(b1), cpu(b2)


def test_evaluate_retrieval_rerank(fx):
    from speech_transcript_embeddings_amd import EmbeddingIndex, embed_audio, embed_texts, evaluate_retrieval, \
        retrieval_metrics
    model = fx["model"]
    b1, b2, c1, c2 = _two_batches(fx)
    k = 4
    out = evaluate_retrieval(model, [c1, None, c2], DEV, ks=(1, 2), return_ranks=True, rerank_k=k)
    assert set(out) == {"a2t", "t2a", "a2t_ranks", "t2a_ranks", "a2t_rerank", "a2t_rerank_ranks"}
    # the reference: search, score_candidates and numpy ordering
    index = None
    for b in (b1, b2):
        t = embed_texts(model, b["input_ids_pos"], b["attention_mask_pos"])
        if index is None:
            index = EmbeddingIndex(t.shape[1], device=DEV)
        index.add(t)
    ids = torch.cat([b1["input_ids_pos"], b2["input_ids_pos"]])
    mask = torch.cat([b1["attention_mask_pos"], b2["attention_mask_pos"]])
    first = out["a2t_ranks"].cpu().numpy()
    want, at = [], 0
    for b in (b1, b2):
        a = embed_audio(model, b["input_values"], b["attention_mask_audio"])
        idx = index.search(a, k)[1].cpu().numpy()
        uniq = np.unique(idx[idx >= 0])
        slots = np.where(idx >= 0, np.searchsorted(uniq, np.maximum(idx, 0)), -1)
        rows = torch.from_numpy(uniq).to(DEV, torch.int64)
        sc = model.score_candidates(b["input_values"], b["attention_mask_audio"], ids[rows], mask[rows],
                                    torch.from_numpy(slots).to(DEV)).cpu().numpy()
        for r in range(idx.shape[0]):
            live = sorted((p for p in range(k) if idx[r, p] >= 0), key=lambda p: (-sc[r, p], p))
            order = [int(idx[r, p]) for p in live]
            want.append(order.index(at + r) if at + r in order else int(first[at + r]))
        at += idx.shape[0]
    assert out["a2t_rerank_ranks"].cpu().tolist() == want
    assert out["a2t_rerank"] == retrieval_metrics(torch.tensor(want), ks=(1, 2)) and out["a2t_rerank"]["n"] == 4
    print("a2t ranks", first.tolist(), "-> reranked", want)
    # k = 1 permutes nothing; k = 0 is the unchanged result
    one = evaluate_retrieval(model, [c1, c2], DEV, ks=(1, 2), return_ranks=True, rerank_k=1)
    assert torch.equal(one["a2t_rerank_ranks"], one["a2t_ranks"]) and torch.equal(one["a2t_ranks"], out["a2t_ranks"])
    assert set(evaluate_retrieval(model, [c1, c2], DEV, rerank_k=0)) == {"a2t", "t2a"}


def test_evaluate_retrieval_rerank_needs_the_same_order(fx):
    from speech_transcript_embeddings_amd import evaluate_retrieval
    _, _, c1, c2 = _two_batches(fx)

    class Reordering:
        """A loader whose second pass yields its batches in the other order."""
        def __init__(self):
            self.passes = 0

        def __iter__(self):
            self.passes += 1
            return iter([c1, c2] if self.passes == 1 else [c2, c1])

    class Shorter(Reordering):
        def __iter__(self):
            self.passes += 1
            return iter([c1, c2] if self.passes == 1 else [c1])

    with pytest.raises(ValueError, match="same items in the same order"):
        evaluate_retrieval(fx["model"], Reordering(), DEV, rerank_k=2)
    with pytest.raises(ValueError, match="yielded 2 items"):
        evaluate_retrieval(fx["model"], Shorter(), DEV, rerank_k=2)
