"""MX-fp8 alignment rows end to end (AudioStateStore(align_rows=True, align_dtype="mx8") /
Engine.locate_clips / retrieval.search_clips) on §20's mini models: the Conformer alignment
model of the golden fixtures (P = 128, 4 alignment heads, 2 clips of 49 and 39 valid frames, 4
transcripts of L = 12) and a wav2vec2 mini model (P = 64) with a ragged sample mask.

Strict: the stored bytes are ops.mx8_quant of the bf16-align store's rows, clip by clip, however the
clips were added; align_kv_rows is their dequantisation; every tensor locate_clips returns on the
mx8-align store is torch.equal to locate_clips on a bf16-align store whose akv rows were overwritten
with those dequantised rows (the kernels share every instruction after the load), for pair_batch 1, 3
and 8 and under either kv_dtype; spans and path scores are the numpy decode of the route's own
emissions; the default store takes no new path.

Toleranced, one figure: max |matrix(mx8-align store) - matrix(bf16-align store)| over the fixture's 8
pairs is > 0 (quantisation happened) and <= 3 x the figure measured on an MI355X when this test was
written, QUANT_EFFECT below.  That is DESIGN §19's rule and reason: room for a toolchain that reorders
the fp32 chain of the head's projections, while a wrong kernel is caught by the exact tests.  How many
token spans differ from the bf16-align store's is printed, not asserted.

Measured on an MI355X: the matrix differs by at most 1.662e-3 (the bound is 4.99e-3), the confidences by
at most 4.44e-3, and 9 of the 96 token spans differ from the bf16-align store's (random mini weights:
the alignment is nearly flat, so small changes move a boundary).
"""
import functools
import types

import numpy as np
import pytest
import torch

from kref_align import viterbi_batch_ref
from test_locate_gpu import ALL, WORD_IDS
from test_model_gpu import batch_of, load, mini_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")
QUANT_EFFECT = 1.662448e-3   # max |matrix(mx8) - matrix(bf16)| on the 8 pairs, measured on an MI355X


def _store(model, wave, amask, **kw):
    from speech_transcript_embeddings_amd import AudioStateStore
    st = AudioStateStore(model, DEV, align_rows=True, **kw)
    st.add(wave, amask)
    return st


def _reference_store(model, wave, amask, mx, **kw):
    """A bf16-align store of the same clips whose akv rows are what the mx8-align store's bytes mean."""
    ref = _store(model, wave, amask, **kw)
    assert ref.akv.dtype == torch.bfloat16 and ref.akv_scales is None
    for n in range(len(ref)):
        ref.align_kv_rows(n).copy_(mx.align_kv_rows(n))
    return ref


@functools.lru_cache(maxsize=None)
def _fx():
    meta, z = load("align")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]])
    mask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]])
    wave, amask = batch["input_values"], batch["attention_mask_audio"]
    bf = _store(model, wave, amask)
    mx = _store(model, wave, amask, align_dtype="mx8")
    wid = torch.tensor(WORD_IDS, device=DEV)
    kw = dict(word_ids=wid, return_matrix=True, return_emit=True)
    cand = torch.tensor(ALL, device=DEV)
    return dict(meta=meta, model=model, ids=ids, mask=mask, wave=wave, amask=amask, bf=bf, mx=mx, kw=kw, cand=cand,
                res=model.locate_clips(ids, mask, mx, cand, **kw), res_bf=model.locate_clips(ids, mask, bf, cand, **kw),
                ntok=mask.sum(1).tolist(), frames=mx.frames.tolist())


@pytest.fixture(scope="module")
def fx():
    return _fx()


def _same_bytes(a, b):
    n = a.rows
    return (a.rows == b.rows and a.seg_row.tolist() == b.seg_row.tolist()
            and torch.equal(a.akv[:n], b.akv[:n]) and torch.equal(a.akv_scales[:n], b.akv_scales[:n]))


def test_layout_is_the_quantised_bf16_rows(fx):
    from speech_transcript_embeddings_amd import ops
    bf, mx = fx["bf"], fx["mx"]
    assert mx.align_dtype == "mx8" and bf.align_dtype == "bf16"
    assert mx.frames.tolist() == [49, 39] and mx.rows == 88
    assert mx.akv.dtype == torch.uint8 and mx.akv.shape[1] == 256 and mx.akv.shape[0] >= 88
    assert mx.akv_scales.dtype == torch.uint8 and mx.akv_scales.shape == (mx.akv.shape[0], 8)
    assert mx.kv.dtype == torch.bfloat16 and torch.equal(mx.kv[:88], bf.kv[:88])       # kv_dtype is independent
    for n in range(2):
        a, f = mx._seg_row[n], mx._seg_len[n]
        q, s = ops.mx8_quant(bf.align_kv_rows(n).contiguous())
        assert torch.equal(mx.akv[a:a + f], q) and torch.equal(mx.akv_scales[a:a + f], s), n
        rows = mx.align_kv_rows(n)
        assert rows.dtype == torch.bfloat16 and torch.equal(rows, ops.mx8_dequant(q, s)), n
        assert not torch.equal(rows, bf.align_kv_rows(n))                                # quantisation happened


def test_growth_and_order_of_adding(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    model, wave, am, mx = fx["model"], fx["wave"], fx["amask"], fx["mx"]
    st = AudioStateStore(model, DEV, reserve_frames=7, align_rows=True, align_dtype="mx8")   # grows on both adds
    assert st.akv.shape == (7, 256) and st.akv_scales.shape == (7, 8)
    st.add(wave[0:1], am[0:1])
    first = (st.akv[:49].clone(), st.akv_scales[:49].clone())
    st.add(wave[1:2], am[1:2])
    assert st.akv.shape[0] == st.akv_scales.shape[0] >= 88
    assert torch.equal(st.akv[:49], first[0]) and torch.equal(st.akv_scales[:49], first[1])   # earlier bytes kept
    assert _same_bytes(st, mx)                                   # two adds of one clip = one add of two
    st2 = AudioStateStore(model, DEV, align_rows=True, align_dtype="mx8")
    st2.add(wave[1:2], am[1:2])
    st2.add(wave, am)
    assert st2.seg_row.tolist() == [0, 39, 88]
    assert torch.equal(st2.akv[39:127], mx.akv[:88]) and torch.equal(st2.akv_scales[39:127], mx.akv_scales[:88])
    assert torch.equal(st2.akv[:39], mx.akv[49:88]) and torch.equal(st2.akv_scales[:39], mx.akv_scales[49:88])
    shifted = model.locate_clips(fx["ids"], fx["mask"], st2, torch.tensor([[1, 2]] * 4, device=DEV), **fx["kw"])
    for k, v in fx["res"].items():
        assert torch.equal(shifted[k], v), k


def test_nbytes(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame, kv_bytes_per_frame
    model, wave, am = fx["model"], fx["wave"], fx["amask"]
    n, rows, P = 2, 88, 128
    base = n * P * 4 + n * P * 4 + n * 12
    assert fx["bf"].nbytes == rows * kv_bytes_per_frame(P) + base + rows * 4 * P          # the parent's formula
    assert fx["mx"].nbytes == rows * kv_bytes_per_frame(P) + base + rows * (2 * P + 2 * P // 32)
    assert fx["mx"].nbytes == fx["bf"].nbytes - rows * (align_bytes_per_frame(P) - align_bytes_per_frame(P, "mx8"))
    both = AudioStateStore(model, DEV, kv_dtype="mx8", align_rows=True, align_dtype="mx8")
    both.add(wave, am)
    assert both.nbytes == base + 2 * rows * (2 * P + 2 * P // 32)


@pytest.mark.parametrize("kv_dtype", ["bf16", "mx8"])
def test_exact_on_the_dequantised_rows(fx, kv_dtype):
    model, ids, mask, wave, am = fx["model"], fx["ids"], fx["mask"], fx["wave"], fx["amask"]
    mx = fx["mx"] if kv_dtype == "bf16" else _store(model, wave, am, kv_dtype="mx8", align_dtype="mx8")
    assert _same_bytes(mx, fx["mx"])                              # the alignment bytes do not depend on kv_dtype
    ref = _reference_store(model, wave, am, mx, kv_dtype=kv_dtype)
    want = model.locate_clips(ids, mask, ref, fx["cand"], **fx["kw"])
    keys = {"token_spans", "token_seconds", "path_score", "scores", "hit_spans", "hit_seconds", "word_spans",
            "word_seconds", "word_scores", "matrix", "emit"}
    assert set(want) == keys
    for pb in (1, 3, 8, 128):
        got = model.locate_clips(ids, mask, mx, fx["cand"], pair_batch=pb, **fx["kw"])
        assert set(got) == keys
        for k in keys:
            assert torch.equal(got[k], want[k]), (kv_dtype, pb, k)
            assert torch.equal(got[k], fx["res"][k]), (kv_dtype, pb, k)
    assert float(want["matrix"].sum()) > 0 and bool((want["token_spans"][:, :, 0, 0] == 0).all())


def test_spans_are_the_decode_of_the_routes_own_emissions(fx):
    r = fx["res"]
    emit = r["emit"].reshape(8, 49, 12).cpu().numpy()
    ntok = [n for n in fx["ntok"] for _ in range(2)]
    nfrm = fx["frames"] * 4
    rs, rsc = viterbi_batch_ref(emit, ntok, nfrm, 12)
    assert np.array_equal(r["token_spans"].reshape(8, 12, 2).cpu().numpy(), rs)
    assert np.array_equal(r["path_score"].reshape(8).cpu().numpy().view(np.int32), rsc.view(np.int32))
    for c, Fr in enumerate(fx["frames"]):                     # frames past the clip's own: 0 / -inf
        assert float(r["matrix"][:, c, :, Fr:].abs().sum()) == 0.0 and bool((r["emit"][:, c, Fr:] == NEG).all())
    assert float((r["matrix"].sum(-1) - 1).abs().max()) <= 1e-5


def test_empty_and_infeasible_slots(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    model, ids, mask = fx["model"], fx["ids"], fx["mask"]
    cand = [[0, -1, 1], [-1, -1, -1], [1, 1, 0], [-1, 0, -1]]
    r = model.locate_clips(ids, mask, fx["mx"], torch.tensor(cand, device=DEV),
                           word_ids=torch.tensor(WORD_IDS, device=DEV))
    full = fx["res"]
    for u, row in enumerate(cand):
        for c, n in enumerate(row):
            if n < 0:
                assert (r["token_spans"][u, c] == -1).all() and (r["token_seconds"][u, c] == -1).all()
                assert (r["hit_spans"][u, c] == -1).all() and (r["hit_seconds"][u, c] == -1).all()
                assert r["path_score"][u, c].item() == NEG and (r["scores"][u, c] == 0).all()
                assert (r["word_spans"][u, c] == -1).all() and (r["word_scores"][u, c] == 0).all()
            else:
                for k in ("token_spans", "path_score", "hit_spans", "scores"):
                    assert torch.equal(r[k][u, c], full[k][u, n]), k
    none = model.locate_clips(ids, mask, fx["mx"], torch.tensor([[-1]] * 4, device=DEV))
    assert (none["token_spans"] == -1).all() and (none["path_score"] == NEG).all() and (none["hit_spans"] == -1).all()
    am = fx["amask"].clone()
    am[1, 10:] = 0                                            # 10 valid frames: infeasible for 12 tokens
    st = AudioStateStore(model, DEV, align_rows=True, align_dtype="mx8")
    st.add(fx["wave"], am)
    assert st.frames.tolist() == [49, 10]
    r = model.locate_clips(ids, mask, st, fx["cand"])
    for u, n in enumerate(fx["ntok"]):
        if n > 10:
            assert (r["token_spans"][u, 1] == -1).all() and r["path_score"][u, 1].item() == NEG
            assert (r["hit_spans"][u, 1] == -1).all()
        else:
            assert r["token_spans"][u, 1, n - 1, 1].item() == 10 and np.isfinite(r["path_score"][u, 1].item())
        assert torch.equal(r["token_spans"][u, 0], full["token_spans"][u, 0])


def test_effect_of_quantisation(fx):
    a, b = fx["res"], fx["res_bf"]
    eff = (a["matrix"] - b["matrix"]).abs().max().item()
    ds = (a["scores"] - b["scores"]).abs().max().item()
    differ = int((a["token_spans"] != b["token_spans"]).any(-1).sum())
    print(f"max |matrix(mx8-align) - matrix(bf16-align)| over the 8 pairs: {eff:.6e} (recorded {QUANT_EFFECT}); "
          f"confidence max difference {ds:.3e}; token spans that differ: {differ} of {a['token_spans'][..., 0].numel()}")
    assert eff > 0.0
    assert QUANT_EFFECT is not None and eff <= 3 * QUANT_EFFECT


def test_errors_and_the_default_store(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.retrieval import kv_bytes_per_frame
    model, wave, am, ids, mask = fx["model"], fx["wave"], fx["amask"], fx["ids"], fx["mask"]
    with pytest.raises(ValueError, match="align_dtype"):
        AudioStateStore(model, DEV, align_rows=True, align_dtype="fp8")
    with pytest.raises(ValueError, match="align_dtype"):
        AudioStateStore(model, DEV, align_dtype="e4m3")         # checked with align_rows=False too
    odd = types.SimpleNamespace(projection_dim=96, use_cross_modal=False, use_word_alignment=True)
    with pytest.raises(ValueError, match="% 64"):
        AudioStateStore(odd, DEV, align_rows=True, align_dtype="mx8")
    # align_rows=False ignores the argument
    plain = AudioStateStore(model, DEV)
    plain.add(wave, am)
    off = AudioStateStore(model, DEV, align_dtype="mx8")
    off.add(wave, am)
    assert off.align_rows is False and off.akv is None and off.akv_scales is None
    n, rows, P = 2, 88, 128
    assert off.nbytes == plain.nbytes == rows * kv_bytes_per_frame(P) + n * P * 4 + n * P * 4 + n * 12
    cand = torch.tensor([[0, 1, -1], [1, 1, 0], [-1, 0, 1], [1, 0, 0]], device=DEV)
    want = model.score_clips(ids, mask, plain, cand)
    assert torch.equal(model.score_clips(ids, mask, off, cand), want)
    assert torch.equal(model.score_clips(ids, mask, fx["mx"], cand), want)
    with pytest.raises(ValueError, match="align_rows"):
        model.locate_clips(ids, mask, off, cand)
    # the default store takes no new path
    assert fx["bf"].akv_scales is None and fx["bf"].akv.dtype == torch.bfloat16


def test_a_stale_store_is_refused(fx):
    model = mini_model(fx["meta"])
    model.eval()
    st = _store(model, fx["wave"], fx["amask"], align_dtype="mx8")
    model.locate_clips(fx["ids"], fx["mask"], st, fx["cand"])
    with torch.no_grad():
        next(model.word_level_alignment.parameters()).mul_(1.0)      # a write outside the optimizer
    with pytest.raises(RuntimeError, match="other weights"):
        model.locate_clips(fx["ids"], fx["mask"], st, fx["cand"])
    with pytest.raises(RuntimeError, match="other weights"):
        st.add(fx["wave"], fx["amask"])


def test_search_clips_is_the_three_calls(fx):
    from speech_transcript_embeddings_amd import embed_texts, rerank_clips, search_clips
    model, store, ids, mask = fx["model"], fx["mx"], fx["ids"], fx["mask"]
    wid = torch.tensor(WORD_IDS, device=DEV)
    vals, idx, where = search_clips(model, store, ids, mask, 3, word_ids=wid)
    first = store.search(embed_texts(model, ids, mask), 3)
    wv, wi = rerank_clips(model, ids, mask, store, first[1])
    want = model.locate_clips(ids, mask, store, wi, word_ids=wid)
    assert torch.equal(vals, wv) and torch.equal(idx, wi) and (idx[:, 2] == -1).all()
    assert set(where) == set(want)
    for k in want:
        assert torch.equal(where[k], want[k]), k
    assert (where["hit_spans"][:, 2] == -1).all() and (where["hit_spans"][:, :2] >= 0).all()


def test_wav2vec2_route():
    """P = 64 (2P = 128: one quantiser tile per row), raw waveforms with a ragged SAMPLE mask."""
    from conftest import GOLDEN
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.modules import TextConfig
    from test_w2v2_gpu import _mini
    golden = np.load(GOLDEN / "w2v2_golden.npz")
    cfg = _mini()
    tc = TextConfig(vocab_size=512, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                    max_position_embeddings=66)
    m = EnhancedAudioTextModel(text_model_name=tc, audio_model_name=cfg, projection_dim=64, text_embedding_dim=64,
                               audio_embedding_dim=cfg.hidden_size, freeze_encoders=False, spec_augment=False,
                               use_word_alignment=True, device="cuda")
    sd = {k[len("param/"):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("param/")}
    m.audio_encoder.load_state_dict(sd, strict=True)
    m.eval()
    wave = torch.from_numpy(golden["mask/wave"]).cuda()
    smask = torch.from_numpy(golden["mask/mask"]).cuda()
    B = wave.shape[0]
    g = torch.Generator().manual_seed(0)
    Uq, L = 3, 9
    ids = torch.randint(3, 500, (Uq, L), generator=g).cuda()
    tmask = torch.ones(Uq, L, dtype=torch.int64)
    tmask[1, 6:] = 0
    tmask = tmask.cuda()
    bf = _store(m, wave, smask)
    mx = _store(m, wave, smask, align_dtype="mx8")
    frames = mx.frames.tolist()
    assert frames == bf.frames.tolist() and len(set(frames)) > 1            # ragged
    for n in range(B):
        a, f = mx._seg_row[n], frames[n]
        q, s = ops.mx8_quant(bf.align_kv_rows(n).contiguous())
        assert torch.equal(mx.akv[a:a + f], q) and torch.equal(mx.akv_scales[a:a + f], s), n
    ref = _reference_store(m, wave, smask, mx)
    cand = torch.tensor([list(range(B))] * Uq, device=DEV)
    got = m.locate_clips(ids, tmask, mx, cand, return_matrix=True, return_emit=True)
    want = m.locate_clips(ids, tmask, ref, cand, return_matrix=True, return_emit=True)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    Tmax = max(frames)
    ntok = [n for n in tmask.sum(1).tolist() for _ in range(B)]
    rs, rsc = viterbi_batch_ref(got["emit"].reshape(Uq * B, Tmax, L).cpu().numpy(), ntok, frames * Uq, L)
    assert np.array_equal(got["token_spans"].reshape(Uq * B, L, 2).cpu().numpy(), rs)
    assert np.array_equal(got["path_score"].reshape(-1).cpu().numpy().view(np.int32), rsc.view(np.int32))
