"""AudioStateStore(kv_dtype="mx8") and Engine.score_clips on it, on the mini models of
test_clip_rerank_gpu.py: P = 128, 8 heads, 2 clips of T = 49 frames (one ragged), 4 transcripts of
L = 12; and the wav2vec2 mini model (P = 64) with a ragged sample mask.

What is exact is checked exactly: the stored bytes are ops.mx8_quant of the bf16 store's rows,
kv_rows says what they mean, and score_clips on the mx8 store has the bits of score_clips on a bf16
store holding those dequantised rows (every other op of the chain is shared).  What quantisation
does to the scores is measured, not bounded a priori: QUANT_EFFECT below.

Measured on an MI355X: max |score(mx8 store) − score(bf16 store)| = 1.120e-3 over the 8 pairs; one add
of two clips and two adds of one give the same bf16 rows, hence the same bytes, for both clips.
"""
import types

import pytest
import torch

from test_clip_rerank_gpu import ALL, _two_batches
from test_model_gpu import batch_of, load, mini_model

pytestmark = pytest.mark.gpu
DEV = "cuda"

# max |score_clips(mx8 store) − score_clips(bf16 store)| over the 8 (text, clip) pairs of the fixture,
# measured on an MI355X.  The input quantisation is deterministic; the test allows 3x for a toolchain
# that reorders the fp32 head chain, not for a wrong kernel (the exact tests catch that).  The scores
# themselves lie in [-0.241, -0.104] there.
QUANT_EFFECT = 1.120e-3


@pytest.fixture(scope="module")
def fx():
    """The model, the batch, the 4 transcripts, a bf16 and an mx8 store of the 2 clips, computed once."""
    from speech_transcript_embeddings_amd import AudioStateStore
    meta, z = load("noalign")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]])
    mask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]])
    stores = {}
    for kd in ("bf16", "mx8"):
        stores[kd] = AudioStateStore(model, DEV, kv_dtype=kd)
        stores[kd].add(batch["input_values"], batch["attention_mask_audio"])
    return dict(meta=meta, model=model, batch=batch, ids=ids, mask=mask, **stores)


def _scores(fx, store, cand=ALL):
    return fx["model"].score_clips(fx["ids"], fx["mask"], store, torch.tensor(cand, device=DEV))


def _bytes(store, n):
    a = store.seg_row[n].item()
    b = a + store.frames[n].item()
    return store.kv[a:b], store.kv_scales[a:b]


def _same_clip(s1, n1, s2, n2):
    return all(torch.equal(x, y) for x, y in zip(_bytes(s1, n1), _bytes(s2, n2)))


def test_store_layout(fx):
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.retrieval import kv_bytes_per_frame
    bf, mx = fx["bf16"], fx["mx8"]
    P = 128
    assert bf.kv_dtype == "bf16" and bf.kv.dtype == torch.bfloat16 and bf.kv_scales is None
    assert mx.kv_dtype == "mx8" and mx.kv.dtype == torch.uint8 and mx.kv_scales.dtype == torch.uint8
    assert mx.kv.shape[1] == 2 * P and mx.kv_scales.shape[1] == 2 * P // 32 and mx.kv.shape[0] == mx.kv_scales.shape[0]
    assert mx.kv.shape[0] >= mx.rows == bf.rows
    assert mx.frames.tolist() == bf.frames.tolist() and mx.seg_row.tolist() == bf.seg_row.tolist()
    assert min(mx.frames.tolist()) < fx["batch"]["attention_mask_audio"].shape[1]            # one ragged clip
    n = len(mx)
    per_clip = P * 4 + P * 4 + 12                                   # aproj, the fp32 unit row, the segment table
    assert mx.nbytes == mx.rows * (2 * P + 2 * P // 32) + n * per_clip
    assert bf.nbytes == bf.rows * 4 * P + n * per_clip
    assert kv_bytes_per_frame(P, "mx8") == 2 * P + 2 * P // 32 and kv_bytes_per_frame(P) == 4 * P
    for c in range(n):
        rows = bf.kv_rows(c)
        assert rows.dtype == torch.bfloat16 and rows.shape == (bf.frames[c].item(), 2 * P)
        assert torch.equal(rows, bf.kv[bf.seg_row[c].item():bf.seg_row[c].item() + rows.shape[0]])
        qb, sc = ops.mx8_quant(rows.contiguous())
        got = _bytes(mx, c)
        assert torch.equal(got[0], qb) and torch.equal(got[1], sc)
        assert torch.equal(mx.kv_rows(c), ops.mx8_dequant(qb, sc)) and mx.kv_rows(c).dtype == torch.bfloat16
        assert not torch.equal(mx.kv_rows(c), rows), "the rows really are quantised"


def test_bytes_do_not_depend_on_how_the_corpus_was_added(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    b = fx["batch"]
    one = {}
    for kd in ("bf16", "mx8"):
        one[kd] = AudioStateStore(fx["model"], DEV, reserve_frames=7, kv_dtype=kd)   # grows on both adds
        for i in (0, 1):
            one[kd].add(b["input_values"][i:i + 1], b["attention_mask_audio"][i:i + 1])
            if i == 0 and kd == "mx8":
                first = [t.clone() for t in _bytes(one[kd], 0)]
    mx = one["mx8"]
    assert mx.kv.shape[0] == mx.kv_scales.shape[0] >= mx.rows and mx.frames.tolist() == fx["mx8"].frames.tolist()
    assert all(torch.equal(x, y) for x, y in zip(first, _bytes(mx, 0))), "growth keeps the earlier clips' bytes"
    same = 0
    for c in range(2):
        if torch.equal(one["bf16"].kv_rows(c), fx["bf16"].kv_rows(c)):      # wherever the bf16 rows have the same bits
            assert _same_clip(mx, c, fx["mx8"], c), c
            same += 1
    print(f"two adds of one clip vs one add of two: {same} of 2 clips with the same bf16 rows")
    # the same clips behind another one: the segments land at other offsets, the bytes do not change
    st2 = AudioStateStore(fx["model"], DEV, kv_dtype="mx8")
    st2.add(b["input_values"][1:2], b["attention_mask_audio"][1:2])
    st2.add(b["input_values"], b["attention_mask_audio"])
    assert st2.seg_row.tolist()[1] == st2.frames[0].item()
    assert _same_clip(st2, 1, fx["mx8"], 0) and _same_clip(st2, 2, fx["mx8"], 1)
    assert torch.equal(_scores(fx, st2, [[1, 2]] * 4), _scores(fx, fx["mx8"]))


def test_scores_have_the_bits_of_a_bf16_store_of_the_dequantised_rows(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    b = fx["batch"]
    st = AudioStateStore(fx["model"], DEV)
    st.add(b["input_values"], b["attention_mask_audio"])
    for c in range(len(st)):
        st.kv_rows(c).copy_(fx["mx8"].kv_rows(c))
    cands = (ALL, [[0, 1, 1], [1, -1, 0], [-1, -1, -1], [1, 0, 1]])
    for cand in cands:
        got, want = _scores(fx, fx["mx8"], cand), _scores(fx, st, cand)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.isfinite(_scores(fx, fx["mx8"])).all()


def test_effect_of_quantisation_on_the_scores(fx):
    a, b = _scores(fx, fx["mx8"]), _scores(fx, fx["bf16"])
    d = (a - b).abs().max().item()
    print(f"max |score(mx8 store) - score(bf16 store)| over {a.numel()} pairs: {d:.3e}; scores in "
          f"[{b.min().item():.4f}, {b.max().item():.4f}]; QUANT_EFFECT = {QUANT_EFFECT}")
    assert d > 0, "the rows really are quantised"
    assert d <= 3 * QUANT_EFFECT


def test_error_paths(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    with pytest.raises(ValueError):
        AudioStateStore(fx["model"], DEV, kv_dtype="fp8")
    with pytest.raises(ValueError):
        AudioStateStore(fx["model"], DEV, kv_dtype=torch.bfloat16)
    stub = types.SimpleNamespace(projection_dim=96, use_cross_modal=True)
    with pytest.raises(ValueError, match="64"):
        AudioStateStore(stub, DEV, kv_dtype="mx8")
    model = mini_model(fx["meta"])
    model.eval()
    b = fx["batch"]
    st = AudioStateStore(model, DEV, kv_dtype="mx8")
    st.add(b["input_values"], b["attention_mask_audio"])
    cand = torch.tensor(ALL, device=DEV)
    model.score_clips(fx["ids"], fx["mask"], st, cand)
    with torch.no_grad():
        next(model.text_projection.parameters()).mul_(1.0)      # a write outside the optimizer
    with pytest.raises(RuntimeError, match="other weights"):
        model.score_clips(fx["ids"], fx["mask"], st, cand)
    with pytest.raises(RuntimeError, match="other weights"):
        st.add(b["input_values"], b["attention_mask_audio"])


def test_without_fusion_the_argument_has_no_effect(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    model = mini_model(fx["meta"], use_cross_modal=False)
    model.eval()
    b = fx["batch"]
    cand = torch.tensor([[0, 1, 1], [1, -1, 0], [-1, 0, -1], [1, 1, 0]], device=DEV)
    got = []
    for kd in ("bf16", "mx8"):
        st = AudioStateStore(model, DEV, kv_dtype=kd)
        st.add(b["input_values"], b["attention_mask_audio"])
        assert st.kv.numel() == 0
        got.append(model.score_clips(fx["ids"], fx["mask"], st, cand))
    assert torch.equal(got[0], got[1])


def test_evaluate_retrieval_with_an_mx8_store(fx):
    from speech_transcript_embeddings_amd import evaluate_retrieval
    _, _, c1, c2 = _two_batches(fx)
    k = 3
    base = evaluate_retrieval(fx["model"], [c1, None, c2], DEV, ks=(1, 2, 4), return_ranks=True, rerank_k=k,
                              rerank_t2a=True)
    out = evaluate_retrieval(fx["model"], [c1, None, c2], DEV, ks=(1, 2, 4), return_ranks=True, rerank_k=k,
                             rerank_t2a=True, store_kv_dtype="mx8")
    assert set(out) == set(base) and out["t2a_rerank"]["n"] == base["t2a_rerank"]["n"] == 4
    # stage 1 and the other direction do not read the K/V rows
    for key in ("a2t", "t2a", "a2t_rerank"):
        assert out[key] == base[key], key
    assert torch.equal(out["t2a_ranks"], base["t2a_ranks"])
    assert out["t2a_rerank"]["recall@4"] == out["t2a"]["recall@4"]       # reranking permutes the first k places only
    print("t2a reranked ranks: bf16 store", base["t2a_rerank_ranks"].tolist(), "mx8 store", out["t2a_rerank_ranks"].tolist())
    with pytest.raises(ValueError):
        evaluate_retrieval(fx["model"], [c1, c2], DEV, rerank_k=k, rerank_t2a=True, store_kv_dtype="int8")


def test_wav2vec2_route(fx):
    """Raw waveforms with a ragged SAMPLE mask at P = 64 (dh = 8: four heads share a scale byte): the same
    frames as the bf16 store, the bytes of its rows, the score identity."""
    import numpy as np
    from conftest import GOLDEN
    from speech_transcript_embeddings_amd import AudioStateStore, ops
    from test_w2v2_gpu import _mini, _model
    golden = np.load(GOLDEN / "w2v2_golden.npz")
    m = _model(_mini())
    sd = {k[len("param/"):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("param/")}
    m.audio_encoder.load_state_dict(sd, strict=True)
    m.eval()
    wave = torch.from_numpy(golden["mask/wave"]).cuda()
    smask = torch.from_numpy(golden["mask/mask"]).cuda()
    B = wave.shape[0]
    g = torch.Generator().manual_seed(0)
    U, L = 3, 9
    ids = torch.randint(3, 500, (U, L), generator=g).cuda()
    tmask = torch.ones(U, L, dtype=torch.int64)
    tmask[1, 6:] = 0
    tmask = tmask.cuda()
    bf, mx = AudioStateStore(m, DEV), AudioStateStore(m, DEV, kv_dtype="mx8")
    bf.add(wave, smask)
    mx.add(wave, smask)
    with torch.no_grad():
        T = m.encode_audio(wave, smask)[1].shape[1]
    assert mx.frames.tolist() == bf.frames.tolist() and min(mx.frames.tolist()) < T             # ragged
    for c in range(B):
        qb, sc = ops.mx8_quant(bf.kv_rows(c).contiguous())
        assert torch.equal(_bytes(mx, c)[0], qb) and torch.equal(_bytes(mx, c)[1], sc)
        bf.kv_rows(c).copy_(mx.kv_rows(c))
    cand = torch.tensor([list(range(B))] * U, device=DEV)
    got, want = m.score_clips(ids, tmask, mx, cand), m.score_clips(ids, tmask, bf, cand)
    assert torch.isfinite(got).all() and torch.equal(got, want)
