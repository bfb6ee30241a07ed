"""Timestamped search hits end to end (AudioStateStore(align_rows=True) / Engine.locate_clips /
model.locate_clips / retrieval.search_clips) on the mini alignment model of the golden
fixtures: P = 128, 4 alignment heads (d = 32), 2 clips of T = 49 frames (49 and 39 valid), 4
transcripts of L = 12 (the clean ones, 12 and 9 tokens, then the corrupted ones); and on a wav2vec2
mini model with a ragged sample mask.

Strict: spans and path scores are the numpy decode (kref_align.viterbi_batch_ref) of the route's own
emissions, bit for bit; hit_*, word_* and the seconds follow from the spans by their stated rules;
empty and infeasible slots are (-1, -1) / -inf; where and how the clips were stored does not change a
bit; align_rows=False leaves the store and score_clips as they were.

Toleranced, the rule of tests/test_align_gpu.py and test_clip_rerank_gpu.py: against the float64
oracle (oracle.ref_model.word_level_alignment's expression on the oracle's own hidden states, every
transcript against every clip) the confidences stay within 1.5·e_old + 1e-4 and the matrix within
1.5·old + 1e-6, e_old / old being model.align's errors on the same 8 pairs.  Every test prints its
figures; whether the bits equal model.align's is printed, not asserted (no GEMM batch invariance is
promised).

Measured on an MI355X: confidence error 4.391e-3 for locate_clips and 4.391e-3 for model.align
(tolerance 6.69e-3); matrix error 3.320e-4 for both (bound 4.99e-4); spans, confidences, path scores
and matrix bitwise equal to model.align's on the 8 pairs, and on the wav2vec2 mini model; two adds
of one clip against one add of two: 0 (bitwise).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kref_align import viterbi_batch_ref
from oracle import ref_model as R
from test_model_gpu import batch_of, load, mini_model, oracle_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")
PRE = "word_level_alignment."
ALL = [[0, 1]] * 4        # every clip for every text
WORD_IDS = [[-1, 0, 0, 1, 2, 2, 2, 4, 4, 5, 6, -1], [-1, 0, 1, 1, 1, 2, 3, 3, -1, -1, -1, -1],
            [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1], [-1, 0, 0, 0, 0, 1, 1, 1, -1, -1, -1, -1]]


def _oracle(p, th, ah, tmask, amask, heads):
    """word_level_alignment's expression in float64 -> (confidence [B, L], head-mean matrix [B, L, T])."""
    sc = R.word_level_alignment(p, PRE, th, ah, tmask, amask, heads)
    tp = R._lin(p, PRE + "text_projection", th)
    ap = R._lin(p, PRE + "audio_projection", ah)
    B, L, E = tp.shape
    S = ap.shape[1]
    W, bW = p[PRE + "alignment_attention.in_proj_weight"], p[PRE + "alignment_attention.in_proj_bias"]
    d = E // heads
    q = F.linear(tp, W[:E], bW[:E]).view(B, L, heads, d).transpose(1, 2)
    k = F.linear(ap, W[E:2 * E], bW[E:2 * E]).view(B, S, heads, d).transpose(1, 2)
    s = (q @ k.transpose(-2, -1)) / math.sqrt(d)
    s = s.masked_fill((1.0 - amask).bool()[:, None, None, :], NEG)
    return sc, torch.softmax(s, -1).mean(1)


@pytest.fixture(scope="module")
def fx():
    """The model, the 4 transcripts, the store of the 2 clips, locate_clips of every pair (with matrix
    and emissions), model.align on the same 8 pairs and the float64 oracle's values, computed once."""
    from speech_transcript_embeddings_amd import AudioStateStore
    meta, z = load("align")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]])
    mask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]])
    store = AudioStateStore(model, DEV, align_rows=True)
    store.add(batch["input_values"], batch["attention_mask_audio"])
    res = model.locate_clips(ids, mask, store, torch.tensor(ALL, device=DEV), return_matrix=True, return_emit=True)
    # the same pairs through model.align: pair (u, b) at row 2u + b
    tix, aix = [u for u in range(4) for _ in range(2)], [0, 1] * 4
    old = model.align(batch["input_values"][aix].contiguous(), batch["attention_mask_audio"][aix].contiguous(),
                      ids[tix].contiguous(), mask[tix].contiguous(), return_matrix=True)
    cfg = R.mini_cfg(meta)
    p = {n: v.detach().double() for n, v in oracle_params(meta).items()}
    cb = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in batch.items()}
    with torch.no_grad():
        th = R.encode_text(p, ids.cpu(), mask.cpu(), cfg)[1]
        ah = R.encode_audio(p, cb["input_values"], cb["attention_mask_audio"], cfg)[1]
        o_sc, o_mx = _oracle(p, th[tix], ah[aix], mask.cpu().double()[tix], cb["attention_mask_audio"].double()[aix],
                             cfg.align_heads)
    return dict(meta=meta, model=model, batch=batch, ids=ids, mask=mask, store=store, res=res, old=old,
                o_sc=o_sc, o_mx=o_mx, ntok=mask.sum(1).tolist(), frames=store.frames.tolist())


def _locate(fx, cand, store=None, **kw):
    return fx["model"].locate_clips(fx["ids"], fx["mask"], store or fx["store"], torch.tensor(cand, device=DEV), **kw)


def test_store_keeps_the_alignment_rows(fx):
    from speech_transcript_embeddings_amd import AudioStateStore, ops
    from speech_transcript_embeddings_amd.align import audio_kv
    from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame
    store, model, b = fx["store"], fx["model"], fx["batch"]
    am = b["attention_mask_audio"]
    assert store.frames.tolist() == am.sum(1).tolist() == [49, 39] and store.rows == 88
    assert store.akv.dtype == torch.bfloat16 and store.akv.shape[1] == 256 and store.akv.shape[0] >= 88
    # the rows are align_infer's kv rows of the valid frames
    with torch.no_grad():
        ah = model.encode_audio(b["input_values"], am)[1]
    B, T, Ha = ah.shape
    ahb = ops.cast_bf16(ah.reshape(B * T, Ha).float().contiguous(), torch.empty(B * T, Ha, device=DEV,
                                                                                dtype=torch.bfloat16))
    kv = audio_kv(model.engine, ahb).view(B, T, -1)
    for n, f in enumerate((49, 39)):
        assert torch.equal(store.align_kv_rows(n), kv[n, :f]), n
    plain = AudioStateStore(model, DEV)
    plain.add(b["input_values"], am)
    assert store.nbytes == plain.nbytes + 88 * align_bytes_per_frame(128)
    with pytest.raises(ValueError, match="align_rows"):
        plain.align_kv_rows(0)


def test_result_shapes_and_rules(fx):
    r = fx["res"]
    assert set(r) == {"token_spans", "token_seconds", "scores", "path_score", "hit_spans", "hit_seconds", "matrix",
                      "emit"}
    assert r["token_spans"].shape == (4, 2, 12, 2) and r["token_spans"].dtype == torch.int32
    assert r["token_seconds"].shape == (4, 2, 12, 2) and r["scores"].shape == (4, 2, 12)
    assert r["path_score"].shape == (4, 2) and r["hit_spans"].shape == (4, 2, 2) and r["hit_spans"].dtype == torch.int32
    assert r["hit_seconds"].shape == (4, 2, 2) and r["matrix"].shape == (4, 2, 12, 49) and r["emit"].shape == (4, 2, 49, 12)
    assert not any(v.requires_grad for v in r.values())
    assert set(_locate(fx, ALL)) == set(r) - {"matrix", "emit"}
    sp = r["token_spans"].cpu()
    assert torch.equal(r["token_seconds"].cpu(), torch.where(sp < 0, -1.0, sp.float() * 0.02))
    hs = r["hit_spans"].cpu()
    assert torch.equal(r["hit_seconds"].cpu(), torch.where(hs < 0, -1.0, hs.float() * 0.02))
    for u, n in enumerate(fx["ntok"]):
        for c, Fr in enumerate(fx["frames"]):
            s = sp[u, c]
            # the spans tile the clip's valid frames; padded tokens are (-1, -1)
            assert s[0, 0] == 0 and s[n - 1, 1] == Fr and torch.equal(s[1:n, 0], s[:n - 1, 1])
            assert bool((s[:n, 1] > s[:n, 0]).all()) and bool((s[n:] == -1).all())
            # the hit: the first frame of token 1 to the end of token n - 2
            assert hs[u, c].tolist() == [int(s[1, 0]), int(s[n - 2, 1])]
            # frames past the clip's own: 0 in the matrix, -inf in the emissions
            assert float(r["matrix"][u, c, :, Fr:].abs().sum()) == 0.0
            assert bool((r["emit"][u, c, Fr:] == NEG).all())
    assert float((r["matrix"].sum(-1) - 1).abs().max()) <= 1e-5
    # custom lead / trail
    wide = _locate(fx, ALL, lead=0, trail=0)["hit_spans"].cpu()
    assert wide[..., 0].eq(0).all() and wide[:, 0, 1].eq(49).all() and wide[:, 1, 1].eq(39).all()
    far = _locate(fx, ALL, lead=4, trail=4)["hit_spans"].cpu()          # 9 tokens: exactly token 4 is left
    for u, n in enumerate(fx["ntok"]):
        for c in range(2):
            want = [int(sp[u, c, 4, 0]), int(sp[u, c, n - 5, 1])] if n >= 9 else [-1, -1]
            assert far[u, c].tolist() == want
    assert (_locate(fx, ALL, lead=5, trail=4)["hit_spans"][1] == -1).all()     # 9 < 5 + 4 + 1


def test_spans_are_the_decode_of_the_routes_own_emissions(fx):
    r = fx["res"]
    emit = r["emit"].reshape(8, 49, 12).cpu().numpy()
    ntok = [n for n in fx["ntok"] for _ in range(2)]
    nfrm = fx["frames"] * 4
    rs, rsc = viterbi_batch_ref(emit, ntok, nfrm, 12)
    assert np.array_equal(r["token_spans"].reshape(8, 12, 2).cpu().numpy(), rs)
    assert np.array_equal(r["path_score"].reshape(8).cpu().numpy().view(np.int32), rsc.view(np.int32))
    # and the emissions are the log of the returned matrix
    m = r["matrix"].double().cpu().clamp_min(float(np.finfo(np.float32).tiny)).log().transpose(2, 3)
    for c, Fr in enumerate(fx["frames"]):
        assert float((r["emit"][:, c, :Fr].double().cpu() - m[:, c, :Fr]).abs().max()) <= 2.0 ** -21 * 88


def test_words_follow_from_the_token_spans(fx):
    wid = torch.tensor(WORD_IDS)
    r = _locate(fx, ALL, word_ids=wid.to(DEV))
    assert torch.equal(r["token_spans"], fx["res"]["token_spans"]) and torch.equal(r["scores"], fx["res"]["scores"])
    W = 10
    assert r["word_spans"].shape == (4, 2, W, 2) and r["word_scores"].shape == (4, 2, W)
    sp, sc = r["token_spans"].cpu(), r["scores"].cpu()
    ws, wsc = r["word_spans"].cpu(), r["word_scores"].cpu()
    for u in range(4):
        for c in range(2):
            for w in range(W):
                toks = [l for l in range(12) if WORD_IDS[u][l] == w and sp[u, c, l, 0] >= 0]
                if not toks:
                    assert ws[u, c, w].tolist() == [-1, -1] and wsc[u, c, w] == 0
                    continue
                assert ws[u, c, w].tolist() == [min(int(sp[u, c, l, 0]) for l in toks),
                                                max(int(sp[u, c, l, 1]) for l in toks)]
                assert abs(float(wsc[u, c, w]) - float(sc[u, c, toks].mean())) < 1e-6
    assert torch.equal(r["word_seconds"].cpu(), torch.where(ws < 0, -1.0, ws.float() * 0.02))


def test_against_the_float64_oracle(fx):
    new_s = fx["res"]["scores"].reshape(8, 12).double().cpu()
    old_s = fx["old"]["scores"].double().cpu()
    e_new, e_old = (new_s - fx["o_sc"]).abs().max().item(), (old_s - fx["o_sc"]).abs().max().item()
    new_m = fx["res"]["matrix"].reshape(8, 12, 49).double().cpu()
    old_m = fx["old"]["matrix"].double().cpu()
    d_new, d_old = (new_m - fx["o_mx"]).abs().max().item(), (old_m - fx["o_mx"]).abs().max().item()
    same = {k: torch.equal(fx["res"][k].reshape(fx["old"][k].shape), fx["old"][k])
            for k in ("token_spans", "scores", "path_score", "matrix")}
    print(f"confidence vs float64 oracle: locate_clips {e_new:.3e}, model.align e_old = {e_old:.3e}, "
          f"tolerance {1.5 * e_old + 1e-4:.3e}")
    print(f"matrix vs float64 oracle: locate_clips {d_new:.3e}, model.align {d_old:.3e}, "
          f"bound {1.5 * d_old + 1e-6:.3e}")
    print(f"bitwise equal to model.align on the same 8 pairs: {same}")
    assert e_new <= 1.5 * e_old + 1e-4
    assert d_new <= 1.5 * d_old + 1e-6


def test_empty_and_infeasible_slots(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    cand = [[0, -1, 1], [-1, -1, -1], [1, 1, 0], [-1, 0, -1]]
    r = _locate(fx, cand, word_ids=torch.tensor(WORD_IDS, device=DEV))
    full = fx["res"]
    for u, row in enumerate(cand):
        for c, n in enumerate(row):
            if n < 0:
                assert (r["token_spans"][u, c] == -1).all() and (r["token_seconds"][u, c] == -1).all()
                assert (r["hit_spans"][u, c] == -1).all() and (r["hit_seconds"][u, c] == -1).all()
                assert r["path_score"][u, c].item() == NEG and (r["scores"][u, c] == 0).all()
                assert (r["word_spans"][u, c] == -1).all() and (r["word_scores"][u, c] == 0).all()
            else:                                    # the same pair wherever it sits in the candidate lists
                assert torch.equal(r["token_spans"][u, c], full["token_spans"][u, n])
                assert torch.equal(r["path_score"][u, c], full["path_score"][u, n])
                assert torch.equal(r["hit_spans"][u, c], full["hit_spans"][u, n])
    none = _locate(fx, [[-1]] * 4)
    assert (none["token_spans"] == -1).all() and (none["path_score"] == NEG).all() and (none["hit_spans"] == -1).all()
    # a clip of 10 valid frames: infeasible for the 12-token transcripts, feasible for the 9-token ones
    b = fx["batch"]
    am = b["attention_mask_audio"].clone()
    am[1, 10:] = 0
    st = AudioStateStore(fx["model"], DEV, align_rows=True)
    st.add(b["input_values"], am)
    assert st.frames.tolist() == [49, 10]
    r = _locate(fx, ALL, st)
    for u, n in enumerate(fx["ntok"]):
        if n > 10:
            assert (r["token_spans"][u, 1] == -1).all() and r["path_score"][u, 1].item() == NEG
            assert (r["hit_spans"][u, 1] == -1).all()
        else:
            assert r["token_spans"][u, 1, n - 1, 1].item() == 10 and math.isfinite(r["path_score"][u, 1].item())
        assert torch.equal(r["token_spans"][u, 0], full["token_spans"][u, 0])


def test_independent_of_how_the_corpus_was_added(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    b, one = fx["batch"], fx["res"]
    keys = ("token_spans", "hit_spans", "path_score", "scores")
    st = AudioStateStore(fx["model"], DEV, reserve_frames=7, align_rows=True)   # grows on both adds
    for i in (0, 1):
        st.add(b["input_values"][i:i + 1], b["attention_mask_audio"][i:i + 1])
    assert st.frames.tolist() == fx["frames"] and st.seg_row.tolist() == fx["store"].seg_row.tolist()
    two = _locate(fx, ALL, st)
    print("two adds of one clip vs one add of two:",
          {k: (two[k].float() - one[k].float()).abs().max().item() for k in keys})
    for k in keys:
        assert torch.equal(two[k], one[k]), k
    # the same clips behind another one: the segments land at other offsets
    st2 = AudioStateStore(fx["model"], DEV, align_rows=True)
    st2.add(b["input_values"][1:2], b["attention_mask_audio"][1:2])
    st2.add(b["input_values"], b["attention_mask_audio"])
    assert st2.seg_row.tolist() == [0, 39, 88]
    shifted = _locate(fx, [[1, 2]] * 4, st2)
    for k in keys:
        assert torch.equal(shifted[k], one[k]), k
    # chunks of pairs: every pair_batch gives the same bits
    for pb in (1, 3, 8):
        chunked = _locate(fx, ALL, pair_batch=pb)
        for k in keys:
            assert torch.equal(chunked[k], one[k]), (pb, k)


def test_align_rows_off_leaves_the_store_as_it_was(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.retrieval import kv_bytes_per_frame
    model, b = fx["model"], fx["batch"]
    assert model.use_cross_modal
    plain = AudioStateStore(model, DEV)
    plain.add(b["input_values"], b["attention_mask_audio"])
    assert plain.align_rows is False and plain.akv is None
    n, rows, P = 2, 88, 128
    assert plain.nbytes == rows * kv_bytes_per_frame(P) + n * P * 4 + n * P * 4 + n * 12     # the parent's formula
    assert torch.equal(plain.kv[:rows], fx["store"].kv[:rows])
    cand = torch.tensor([[0, 1, -1], [1, 1, 0], [-1, 0, 1], [1, 0, 0]], device=DEV)
    assert torch.equal(model.score_clips(fx["ids"], fx["mask"], plain, cand),
                       model.score_clips(fx["ids"], fx["mask"], fx["store"], cand))
    with pytest.raises(ValueError, match="align_rows"):
        model.locate_clips(fx["ids"], fx["mask"], plain, cand)


def test_search_clips_is_the_three_calls(fx):
    from speech_transcript_embeddings_amd import embed_texts, rerank_clips, search_clips
    model, store = fx["model"], fx["store"]
    wid = torch.tensor(WORD_IDS, device=DEV)
    vals, idx, where = search_clips(model, store, fx["ids"], fx["mask"], 3, word_ids=wid)
    t = embed_texts(model, fx["ids"], fx["mask"])
    first = store.search(t, 3)
    wv, wi = rerank_clips(model, fx["ids"], fx["mask"], store, first[1])
    want = model.locate_clips(fx["ids"], fx["mask"], store, wi, word_ids=wid)
    assert torch.equal(vals, wv) and torch.equal(idx, wi) and (idx[:, 2] == -1).all()
    assert set(where) == set(want)
    for k in want:
        assert torch.equal(where[k], want[k]), k
    assert (where["hit_spans"][:, 2] == -1).all() and (where["hit_spans"][:, :2] >= 0).all()
    # stage 1 only, and without the location
    v1, i1, w1 = search_clips(model, store, fx["ids"], fx["mask"], 3, rerank=False)
    assert torch.equal(v1, first[0]) and torch.equal(i1, first[1])
    assert torch.equal(w1["hit_spans"], model.locate_clips(fx["ids"], fx["mask"], store, first[1])["hit_spans"])
    assert search_clips(model, store, fx["ids"], fx["mask"], 2, locate=False)[2] is None


def test_errors_and_side_effects(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    model, b = fx["model"], fx["batch"]
    meta, _ = load("noalign")
    noalign = mini_model(meta)
    with pytest.raises(ValueError, match="use_word_alignment"):
        AudioStateStore(noalign, DEV, align_rows=True)
    with pytest.raises(ValueError, match="use_word_alignment"):
        noalign.locate_clips(fx["ids"], fx["mask"], fx["store"], torch.tensor(ALL, device=DEV))
    with pytest.raises(ValueError, match="lie in"):
        _locate(fx, [[0, 2]] * 4)
    with pytest.raises(ValueError, match="lie in"):
        _locate(fx, [[0, -2]] * 4)
    holed = fx["mask"].clone()
    holed[0, 3] = 0
    with pytest.raises(ValueError, match="prefix"):
        model.locate_clips(fx["ids"], holed, fx["store"], torch.tensor(ALL, device=DEV))
    model.train()
    try:
        r = _locate(fx, ALL)
        assert model.training
    finally:
        model.eval()
    assert torch.equal(r["token_spans"], fx["res"]["token_spans"]) and torch.equal(r["scores"], fx["res"]["scores"])
    # a clip over 2048 valid frames is refused by add; the store is left as it was
    st = AudioStateStore(model, DEV, align_rows=True)
    T, Ha = 2049, model.audio_hidden_dim
    enc = (torch.zeros(1, model.projection_dim, device=DEV), torch.zeros(1, T, Ha, device=DEV))
    with pytest.raises(ValueError, match="2048"):
        st.add(None, torch.ones(1, T, dtype=torch.int64, device=DEV), audio_encoded=enc)
    assert len(st) == 0 and st.rows == 0


def test_a_stale_store_is_refused(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    model = mini_model(fx["meta"])
    model.eval()
    b = fx["batch"]
    st = AudioStateStore(model, DEV, align_rows=True)
    st.add(b["input_values"], b["attention_mask_audio"])
    cand = torch.tensor(ALL, device=DEV)
    model.locate_clips(fx["ids"], fx["mask"], st, cand)
    with torch.no_grad():
        next(model.word_level_alignment.parameters()).mul_(1.0)      # a write outside the optimizer
    with pytest.raises(RuntimeError, match="other weights"):
        model.locate_clips(fx["ids"], fx["mask"], st, cand)
    with pytest.raises(RuntimeError, match="other weights"):
        st.add(b["input_values"], b["attention_mask_audio"])


def test_wav2vec2_route():
    """Raw waveforms with a ragged SAMPLE mask: the store turns it into the frame mask
    (wav2vec2.frame_mask) as align_pairs does, and every pair's spans tile its clip's valid frames
    and are the numpy decode of the route's emissions."""
    from conftest import GOLDEN
    from speech_transcript_embeddings_amd import AudioStateStore
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
    assert smask.shape == wave.shape and not bool(smask.all())               # a ragged sample mask
    g = torch.Generator().manual_seed(0)
    U, L = 3, 9
    ids = torch.randint(3, 500, (U, L), generator=g).cuda()
    tmask = torch.ones(U, L, dtype=torch.int64)
    tmask[1, 6:] = 0
    tmask = tmask.cuda()
    store = AudioStateStore(m, DEV, align_rows=True)
    store.add(wave, smask)
    with torch.no_grad():
        T = m.encode_audio(wave, smask)[1].shape[1]
    frames = store.frames.tolist()
    assert len(store) == B and max(frames) <= T and min(frames) < T
    cand = torch.tensor([list(range(B))] * U, device=DEV)
    r = m.locate_clips(ids, tmask, store, cand, return_emit=True)
    Tmax = max(frames)
    assert r["emit"].shape == (U, B, Tmax, L)
    ntok = [n for n in tmask.sum(1).tolist() for _ in range(B)]
    rs, rsc = viterbi_batch_ref(r["emit"].reshape(U * B, Tmax, L).cpu().numpy(), ntok, frames * U, L)
    assert np.array_equal(r["token_spans"].reshape(U * B, L, 2).cpu().numpy(), rs)
    assert np.array_equal(r["path_score"].reshape(-1).cpu().numpy().view(np.int32), rsc.view(np.int32))
    sp = r["token_spans"].cpu()
    for u, n in enumerate(tmask.sum(1).tolist()):
        for c, Fr in enumerate(frames):
            if Fr >= n:
                assert sp[u, c, 0, 0] == 0 and sp[u, c, n - 1, 1] == Fr
    # the same pairs through model.align (clip c with transcript u), reported
    tix, aix = [u for u in range(U) for _ in range(B)], list(range(B)) * U
    old = m.align(wave[aix].contiguous(), smask[aix].contiguous(), ids[tix].contiguous(), tmask[tix].contiguous())
    same = torch.equal(old["token_spans"], r["token_spans"].reshape(U * B, L, 2))
    ds = (old["scores"] - r["scores"].reshape(U * B, L)).abs().max().item()
    print(f"wav2vec2: spans equal model.align's: {same}; confidence max difference {ds:.3e}")
    # seconds per frame: the mini conv stack's total stride in samples at 16 kHz
    fs = math.prod(cfg.conv_stride) / 16000
    assert m.engine.frame_seconds == fs
    assert torch.equal(r["token_seconds"].cpu(), torch.where(sp < 0, -1.0, sp.float() * fs))
