"""Text -> clip reranking (retrieval.AudioStateStore / Engine.score_clips / model.score_clips /
retrieval.rerank_clips) on the mini model of the golden fixtures: P = 128, 8 heads,
2 clips of T = 49 frames (one ragged), 4 transcripts of L = 12.

The tolerance against the float64 oracle is test_rerank_gpu.py's: e_old = max |(s_pos, s_neg) of
model(batch) - oracle|, and the scores must stay within 1.5·e_old + 1e-4 (the margin covers the
same single bf16 rounding of the probabilities in the text->audio attention).

Measured on an MI355X: e_old = 7.24e-4; score_clips against the oracle 9.15e-4 (tolerance 1.19e-3);
score_clips against score_candidates transposed 0 (bitwise), also on the wav2vec2 route; one add of
two clips against two adds of one 0 (bitwise).  Each test prints its figures.
"""
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
    """The model, the batch, the 4 distinct transcripts (clean 0, 1 then corrupted 2, 3), the store of
    the 2 clips, the float64 pair score of all 4 x 2 pairs and the tolerance, computed once."""
    from speech_transcript_embeddings_amd import AudioStateStore
    meta, z = load("noalign")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]])
    mask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]])
    with torch.no_grad():
        tpn, tnn, an = model(batch)
        s_old = torch.stack([(an * tpn).sum(1), (an * tnn).sum(1)], 1).double().cpu()
    cfg = R.mini_cfg(meta)
    p = {n: v.detach().double() for n, v in oracle_params(meta).items()}
    cb = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items()}
    with torch.no_grad():
        otp, otn, oan, _ = R.compute_pos_neg_embeddings(p, cb, cfg)
        s_ref = torch.stack([(oan * otp).sum(1), (oan * otn).sum(1)], 1)
        tp, th = R.encode_text(p, ids.cpu(), mask.cpu(), cfg)
        ap, ah = R.encode_audio(p, cb["input_values"], cb["attention_mask_audio"], cfg)
        oracle = torch.zeros(4, 2, dtype=torch.float64)
        for u in range(4):
            for b in range(2):
                tf, af = R.apply_cross_modal(p, tp[u:u + 1], th[u:u + 1], mask.cpu()[u:u + 1], ap[b:b + 1],
                                             ah[b:b + 1], cb["attention_mask_audio"][b:b + 1], cfg)
                oracle[u, b] = (F.normalize(tf, dim=1) * F.normalize(af, dim=1)).sum()
    e_old = (s_old - s_ref).abs().max().item()
    store = AudioStateStore(model, DEV)
    store.add(batch["input_values"], batch["attention_mask_audio"])
    return dict(meta=meta, model=model, batch=batch, ids=ids, mask=mask, oracle=oracle, e_old=e_old,
                tol=1.5 * e_old + 1e-4, store=store)


def _scores(fx, cand, store=None):
    return fx["model"].score_clips(fx["ids"], fx["mask"], store or fx["store"], torch.tensor(cand, device=DEV))


ALL = [[0, 1]] * 4        # every clip for every text


def test_store_holds_the_valid_frames(fx):
    store, am = fx["store"], fx["batch"]["attention_mask_audio"]
    assert len(store) == 2 and store.frames.dtype == torch.int32
    assert store.frames.tolist() == am.sum(1).tolist() and min(store.frames.tolist()) < am.shape[1]   # one ragged
    assert store.seg_row.tolist() == [0, store.frames[0].item()] and store.rows == int(am.sum())
    assert store.kv.dtype == torch.bfloat16 and store.kv.shape[1] == 2 * 128 and store.kv.shape[0] >= store.rows
    assert store.nbytes >= store.rows * 2 * 128 * 2 + 2 * 128 * 4


def test_score_clips_matches_oracle(fx):
    got = _scores(fx, ALL)
    assert got.shape == (4, 2) and got.dtype == torch.float32 and not got.requires_grad
    err = (got.double().cpu() - fx["oracle"]).abs().max().item()
    print(f"score_clips vs float64 oracle: max error {err:.3e}; model(batch) vs oracle e_old = {fx['e_old']:.3e}; "
          f"tolerance {fx['tol']:.3e}")
    assert err <= fx["tol"]


def test_symmetric_to_score_candidates(fx):
    """The same chain on the same rows: score_clips[u][b] has the bits of score_candidates[b][u], the
    ragged clip included (the store's truncated rows against the masked padded ones)."""
    b = fx["batch"]
    a2t = fx["model"].score_candidates(b["input_values"], b["attention_mask_audio"], fx["ids"], fx["mask"],
                                       torch.tensor([[0, 1, 2, 3]] * 2, device=DEV))
    t2a = _scores(fx, ALL)
    print("score_clips - score_candidatesᵀ: max", (t2a - a2t.t()).abs().max().item())
    assert torch.equal(t2a, a2t.t())


def test_independent_of_how_the_corpus_was_added(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    b = fx["batch"]
    st = AudioStateStore(fx["model"], DEV, reserve_frames=7)     # grows on the first and on the second add
    for i in (0, 1):
        st.add(b["input_values"][i:i + 1], b["attention_mask_audio"][i:i + 1])
    assert st.frames.tolist() == fx["store"].frames.tolist() and st.seg_row.tolist() == fx["store"].seg_row.tolist()
    one, two = _scores(fx, ALL), _scores(fx, ALL, st)
    diff = (one - two).abs().max().item()
    print(f"one add of 2 clips vs two adds of 1: max difference {diff:.3e} (bitwise equal: {torch.equal(one, two)})")
    assert diff <= fx["tol"]
    assert (two.double().cpu() - fx["oracle"]).abs().max().item() <= fx["tol"]
    # the same clips behind another one: the segments land at other offsets
    st2 = AudioStateStore(fx["model"], DEV)
    st2.add(b["input_values"][1:2], b["attention_mask_audio"][1:2])
    st2.add(b["input_values"], b["attention_mask_audio"])
    assert st2.seg_row.tolist()[1] == st2.frames[0].item()
    shifted = _scores(fx, [[1, 2]] * 4, st2)
    assert torch.equal(shifted, one)


def test_permutation_empties_and_repeats(fx):
    cand = torch.tensor([[0, 1, 1], [1, -1, 0], [-1, -1, -1], [1, 0, 1]])
    base = _scores(fx, cand.tolist())
    for perm in ([2, 1, 0], [1, 2, 0]):
        assert torch.equal(_scores(fx, cand[:, perm].tolist()), base[:, perm]), perm
    assert base[1, 1].item() == NEG and (base[2] == NEG).all() and torch.isfinite(base[0]).all()
    assert torch.equal(base[0, 1], base[0, 2]) and torch.equal(base[3, 0], base[3, 2])   # the same clip twice
    full = _scores(fx, ALL)
    assert torch.equal(base[0, :2], full[0]) and torch.equal(base[3, 1], full[3, 0])
    assert (_scores(fx, [[-1]] * 4) == NEG).all()


def test_without_fusion_is_the_indexed_cosine(fx):
    from speech_transcript_embeddings_amd import AudioStateStore, embed_audio, embed_texts, ops
    model = mini_model(fx["meta"], use_cross_modal=False)
    model.eval()
    b = fx["batch"]
    store = AudioStateStore(model, DEV)
    store.add(b["input_values"], b["attention_mask_audio"])
    assert store.kv.numel() == 0
    cand = [[0, 1, 1], [1, -1, 0], [-1, 0, -1], [1, 1, 0]]
    got = model.score_clips(fx["ids"], fx["mask"], store, torch.tensor(cand, device=DEV))
    A = embed_audio(model, b["input_values"], b["attention_mask_audio"])
    T = embed_texts(model, fx["ids"], fx["mask"])
    S = torch.empty(T.shape[0], A.shape[0], device=DEV)
    ops.similarity(T, A, S)
    for r, row in enumerate(cand):
        for c, n in enumerate(row):
            assert got[r, c].item() == (S[r, n].item() if n >= 0 else NEG), (r, c)


def test_input_errors(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    b = fx["batch"]
    with pytest.raises(ValueError):
        _scores(fx, [[0, 2]] * 4)
    with pytest.raises(ValueError):
        _scores(fx, [[0, -2]] * 4)
    st = AudioStateStore(fx["model"], DEV)
    holes = b["attention_mask_audio"].clone()
    holes[0, 3] = 0                                  # not a prefix mask
    with pytest.raises(ValueError):
        st.add(b["input_values"], holes)
    none = b["attention_mask_audio"].clone()
    none[1] = 0                                      # a clip with no valid frame
    with pytest.raises(ValueError):
        st.add(b["input_values"], none)
    assert len(st) == 0 and st.rows == 0


def test_a_stale_store_is_refused(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    model = mini_model(fx["meta"])
    model.eval()
    b = fx["batch"]
    st = AudioStateStore(model, DEV)
    st.add(b["input_values"], b["attention_mask_audio"])
    cand = torch.tensor(ALL, device=DEV)
    model.score_clips(fx["ids"], fx["mask"], st, cand)
    with torch.no_grad():
        next(model.text_projection.parameters()).mul_(1.0)      # a write outside the optimizer
    with pytest.raises(RuntimeError, match="other weights"):
        model.score_clips(fx["ids"], fx["mask"], st, cand)
    with pytest.raises(RuntimeError, match="other weights"):
        st.add(b["input_values"], b["attention_mask_audio"])


def test_rerank_clips_and_search(fx):
    from speech_transcript_embeddings_amd import EmbeddingIndex, embed_audio, embed_texts, rerank_clips, rerank_order
    model, b, store = fx["model"], fx["batch"], fx["store"]
    t = embed_texts(model, fx["ids"], fx["mask"])
    index = EmbeddingIndex(t.shape[1], device=DEV)
    index.add(embed_audio(model, b["input_values"], b["attention_mask_audio"]))
    for k in (1, 2, 3):
        got, want = store.search(t, k), index.search(t, k)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    idx = store.search(t, 3)[1]                                  # the third column is empty
    vals, order = rerank_clips(model, fx["ids"], fx["mask"], store, idx)
    sc = model.score_clips(fx["ids"], fx["mask"], store, idx)
    wv, wo = rerank_order(sc, idx)
    assert torch.equal(vals, wv) and torch.equal(order, wo)
    assert (order[:, 2] == -1).all() and (vals[:, 2] == NEG).all() and (vals[:, 0] >= vals[:, 1]).all()
    enc = model.encode_text(fx["ids"], fx["mask"])
    again = rerank_clips(model, fx["ids"], fx["mask"], store, idx, text_encoded=enc)
    assert torch.equal(again[0], vals) and torch.equal(again[1], order)


def _two_batches(fx):
    b1 = fx["batch"]
    # the batches of test_rerank_gpu.py: the corrupted transcripts as clean ones, clips reversed
    b2 = dict(b1, input_ids_pos=b1["input_ids_neg"], attention_mask_pos=b1["attention_mask_neg"],
              input_values=b1["input_values"].flip(0).contiguous(),
              attention_mask_audio=b1["attention_mask_audio"].flip(0).contiguous())
    cpu = lambda b: {k: v.cpu() for k, v in b.items()}                                 # noqa: E731
    return b1, b2, cpu(b1), cpu(b2)


def test_evaluate_retrieval_t2a_rerank(fx):
    from speech_transcript_embeddings_amd import AudioStateStore, embed_texts, evaluate_retrieval, rerank_clips, \
        retrieval_metrics
    model = fx["model"]
    b1, b2, c1, c2 = _two_batches(fx)
    k = 3
    old = evaluate_retrieval(model, [c1, None, c2], DEV, ks=(1, 2, 4), return_ranks=True, rerank_k=k)
    out = evaluate_retrieval(model, [c1, None, c2], DEV, ks=(1, 2, 4), return_ranks=True, rerank_k=k, rerank_t2a=True)
    assert set(out) == set(old) | {"t2a_rerank", "t2a_rerank_ranks"}
    assert set(evaluate_retrieval(model, [c1, c2], DEV, rerank_k=k, rerank_t2a=True)) == \
        {"a2t", "t2a", "a2t_rerank", "t2a_rerank"}
    # with the flag on, everything the parent reported is unchanged; with it off nothing is added
    for key, v in old.items():
        assert torch.equal(out[key], v) if isinstance(v, torch.Tensor) else out[key] == v, key
    assert set(evaluate_retrieval(model, [c1, c2], DEV, rerank_k=0, rerank_t2a=True)) == {"a2t", "t2a"}
    # by hand: store -> search -> rerank_clips
    store = AudioStateStore(model, DEV)
    for b in (b1, b2):
        store.add(b["input_values"], b["attention_mask_audio"])
    first = out["t2a_ranks"].cpu().tolist()
    want, at = [], 0
    for b in (b1, b2):
        t = embed_texts(model, b["input_ids_pos"], b["attention_mask_pos"])
        idx = store.search(t, k)[1]
        order = rerank_clips(model, b["input_ids_pos"], b["attention_mask_pos"], store, idx)[1].cpu().tolist()
        for r, row in enumerate(order):
            want.append(row.index(at + r) if at + r in row else first[at + r])
        at += len(order)
    assert out["t2a_rerank_ranks"].cpu().tolist() == want
    # (the metrics of the same ranks on the same device: a float64 mean is not bitwise portable)
    assert out["t2a_rerank"] == retrieval_metrics(torch.tensor(want, device=DEV), ks=(1, 2, 4))
    assert out["t2a_rerank"]["n"] == 4
    print("t2a ranks", first, "-> reranked", want)
    # reranking permutes the first k places only
    for m in (4,):
        assert out["t2a_rerank"][f"recall@{m}"] == out["t2a"][f"recall@{m}"]
    one = evaluate_retrieval(model, [c1, c2], DEV, ks=(1, 2), return_ranks=True, rerank_k=1, rerank_t2a=True)
    assert torch.equal(one["t2a_rerank_ranks"], one["t2a_ranks"])


def test_wav2vec2_route(fx):
    """Raw waveforms with a ragged SAMPLE mask: the store turns it into the frame mask
    (wav2vec2.frame_mask) as score_pairs does, and score_clips agrees with score_candidates."""
    import numpy as np
    from conftest import GOLDEN
    from speech_transcript_embeddings_amd import AudioStateStore
    from test_w2v2_gpu import _mini, _model
    golden = np.load(GOLDEN / "w2v2_golden.npz")
    m = _model(_mini())
    sd = {k[len("param/"):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("param/")}
    m.audio_encoder.load_state_dict(sd, strict=True)
    m.eval()
    wave = torch.from_numpy(golden["mask/wave"]).cuda()
    smask = torch.from_numpy(golden["mask/mask"]).cuda()
    B = wave.shape[0]
    assert smask.shape == wave.shape and not bool(smask.all())               # a ragged sample mask
    g = torch.Generator().manual_seed(0)
    U, L = 3, 9
    ids = torch.randint(3, 500, (U, L), generator=g).cuda()
    tmask = torch.ones(U, L, dtype=torch.int64)
    tmask[1, 6:] = 0
    tmask = tmask.cuda()
    store = AudioStateStore(m, DEV)
    store.add(wave, smask)
    with torch.no_grad():
        T = m.encode_audio(wave, smask)[1].shape[1]
    assert len(store) == B and max(store.frames.tolist()) <= T and min(store.frames.tolist()) < T
    t2a = m.score_clips(ids, tmask, store, torch.tensor([list(range(B))] * U, device=DEV))
    a2t = m.score_candidates(wave, smask, ids, tmask, torch.tensor([list(range(U))] * B, device=DEV))
    diff = (t2a - a2t.t()).abs().max().item()
    print(f"wav2vec2: score_clips vs score_candidatesᵀ max difference {diff:.3e} (tolerance {fx['tol']:.3e})")
    assert torch.isfinite(t2a).all() and diff <= fx["tol"]
