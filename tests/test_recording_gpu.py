"""Long recordings in the AudioStateStore end to end (AudioStateStore.add_recording,
retrieval.search_recordings) on the mini alignment model of tests/test_locate_gpu.py (P = 128,
4 alignment heads), with align_rows=True, once with bf16 and once with MX-fp8 rows in both banks.

Strict, all of it (torch.equal): a recording short enough for one chunk and one window is the clip
store.add makes of the same features; a long recording's rows are stored once and are the rows of the
same engine calls made by hand on the same batch shapes; every window's projection is the DENSE pooling
of a copy of its rows; search_recordings is its stages composed by hand."""
import pytest
import torch

from test_locate_gpu import WORD_IDS
from test_model_gpu import batch_of, load, mini_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
LONG = dict(window_frames=40, hop_frames=20, chunk_frames=48, context_frames=8, chunk_batch=2)
DTYPES = [pytest.param("bf16", id="bf16"), pytest.param("mx8", id="mx8")]


@pytest.fixture(scope="module")
def fx():
    meta, z = load("align")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    g = torch.Generator(device="cpu").manual_seed(23)
    return dict(model=model, batch=batch, wid=torch.tensor(WORD_IDS, device=DEV),
                ids=torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]]),
                mask=torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]]),
                rec130=torch.randn(130, 160, generator=g).to(DEV), rec90=torch.randn(90, 160, generator=g).to(DEV))


def _store(fx, dtype, **kw):
    from speech_transcript_embeddings_amd import AudioStateStore
    return AudioStateStore(fx["model"], DEV, kv_dtype=dtype, align_rows=True, align_dtype=dtype, **kw)


def _unit(store, n):
    assert len(store.index.chunks) >= 1
    return torch.cat([rows for _, rows in store.index.chunks])[n]


def _bank_rows(bank_dtype, rows_bf16):
    """What a bank of this dtype says it holds after writing these bf16 rows."""
    from speech_transcript_embeddings_amd import ops
    return rows_bf16 if bank_dtype == "bf16" else ops.mx8_dequant(*ops.mx8_quant(rows_bf16))


# ------------------------------------------------------------------ a short recording is a clip
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_short_recording_is_the_clip_add_makes(fx, dtype):
    x = fx["batch"]["input_values"][:1].contiguous()                     # clip 0: 49 frames, all valid
    clip, rec = _store(fx, dtype), _store(fx, dtype)
    clip.add(x, torch.ones(1, 49, dtype=torch.int64, device=DEV))
    assert rec.add_recording(x[0]) == 0                                  # one chunk, no context, one window
    assert len(rec) == 1 and rec.rows == 49 and rec.recordings == 1 and rec.nbytes == clip.nbytes
    assert rec.seg_row.tolist() == [0] and rec.frames.tolist() == [49]
    assert rec.recording_of.tolist() == [0] and rec.offset_of.tolist() == [0]
    assert torch.equal(rec.kv_rows(0), clip.kv_rows(0))
    assert torch.equal(rec.align_kv_rows(0), clip.align_kv_rows(0))
    assert torch.equal(rec.aproj[0], clip.aproj[0])
    assert torch.equal(_unit(rec, 0), _unit(clip, 0))
    again = _store(fx, dtype)
    assert again.add_recording(x) == 0                                   # [1, F, 160] is accepted too
    assert torch.equal(again.aproj, rec.aproj) and torch.equal(again.kv_rows(0), rec.kv_rows(0))


# ------------------------------------------------------------------ a long recording
def _by_hand(fx, x, plan, chunk_batch):
    """The kept frames' fp32 states and split image from engine.audio_forward on the batches
    add_recording forms, then the rows and the scorer activations over all of them at once."""
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd._lib import ACT_TANH
    from speech_transcript_embeddings_amd.align import audio_kv
    model = fx["model"]
    eng, s = model.engine, model.store
    s.sync_shadow()
    F = x.shape[0]
    D = eng.acfg.hidden_size
    h = torch.empty(F, D, device=DEV)
    hs = torch.empty(F, 2 * D, device=DEV, dtype=BF16)
    chunks = list(zip(plan["keep"], plan["input"]))
    for c0 in range(0, len(chunks), chunk_batch):
        part = chunks[c0:c0 + chunk_batch]
        T = max(b - a for _, (a, b) in part)
        feats = torch.zeros(len(part), T, 160, device=DEV)
        mask = torch.zeros(len(part), T, dtype=torch.int64, device=DEV)
        for j, (_, (a, b)) in enumerate(part):
            feats[j, :b - a] = x[a:b]
            mask[j, :b - a] = 1
        ctx = {}
        hc, _ = eng.audio_forward(feats, mask, False, 0, ctx, save=False)
        for j, ((ka, kb), (a, _)) in enumerate(part):
            h[ka:kb] = hc[j * T + ka - a:j * T + kb - a]
            hs[ka:kb] = ctx["a_hs"][j * T + ka - a:j * T + kb - a]
    hb = ops.cast_bf16(h, torch.empty(F, D, device=DEV, dtype=BF16))
    kv = eng._kv("text_to_audio_attention", "audio_seq_to_projection", hb)[0]
    akv = audio_kv(eng, hb)
    t = ops.linear(hs, s.w2("audio_pooling.attention.0.weight"), s.p("audio_pooling.attention.0.bias"), act=ACT_TANH)
    return h, kv, akv, t


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_long_recording_is_stored_once_and_windowed_in_place(fx, dtype):
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame, kv_bytes_per_frame, plan_recording
    model, x = fx["model"], fx["rec130"]
    eng, s = model.engine, model.store
    plan = plan_recording(130, 40, 20, 48, 8)
    assert plan["keep"] == [(0, 48), (48, 96), (96, 130)] and plan["input"] == [(0, 56), (40, 104), (88, 130)]
    starts, lens = plan["window_start"], plan["window_len"]
    assert starts == [0, 20, 40, 60, 80, 100] and lens == [40] * 5 + [30]
    store = _store(fx, dtype, reserve_frames=50)                          # grows inside add_recording
    assert store.add_recording(x, **LONG) == 0
    W, P = 6, 128
    assert store.rows == 130 and len(store) == W and store.recordings == 1
    assert store.nbytes == (130 * (kv_bytes_per_frame(P, dtype) + align_bytes_per_frame(P, dtype))
                            + W * P * 4 + W * P * 4 + W * 12)
    assert store.recording_of.tolist() == [0] * W and store.recording_of.dtype == I32
    assert store.offset_of.tolist() == starts and store.offset_of.dtype == I32
    assert store.seg_row.tolist() == starts and store.frames.tolist() == lens
    # the rows: stored once, the same engine calls made by hand on the same batch shapes
    h, kv, akv, t = _by_hand(fx, x, plan, 2)
    assert torch.equal(store.kv_bank.rows(0, 130), _bank_rows(dtype, kv))
    assert torch.equal(store.align_bank.rows(0, 130), _bank_rows(dtype, akv))
    for n, (a, ln) in enumerate(zip(starts, lens)):                      # windows are slices of those 130 rows
        assert torch.equal(store.kv_rows(n), store.kv_bank.rows(a, a + ln))
        assert torch.equal(store.align_kv_rows(n), store.align_bank.rows(a, a + ln))
    if dtype == "bf16":                                                  # views of one buffer, overlapping by 20 rows
        assert store.kv_rows(1).data_ptr() == store.kv.data_ptr() + 20 * 2 * P * 2
        assert store.kv_rows(0)[20:].data_ptr() == store.kv_rows(1).data_ptr()
    # every window's projection: the DENSE pooling (B = 1) of a copy of its rows, through _proj_fwd on [W, H]
    w2, b2 = s.p("audio_pooling.attention.2.weight").view(-1), s.p("audio_pooling.attention.2.bias")
    pooled = torch.empty(W, h.shape[1], device=DEV)
    for n, (a, ln) in enumerate(zip(starts, lens)):
        ops.attn_pool_fwd_f32(t[a:a + ln].clone(), w2, b2, h[a:a + ln].clone(), None, 1, ln,
                              torch.empty(ln, device=DEV), pooled[n:n + 1])
    aproj = eng._proj_fwd("audio_projection", pooled, W, False, 0, {})
    assert torch.equal(store.aproj, aproj)
    from speech_transcript_embeddings_amd.retrieval import _unit_rows
    assert torch.equal(torch.cat([r for _, r in store.index.chunks]), _unit_rows(aproj))
    assert not torch.equal(store.aproj[0], store.aproj[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_store_keeps_clips_and_ids(fx, dtype):
    b = fx["batch"]
    clips = _store(fx, dtype)
    clips.add(b["input_values"], b["attention_mask_audio"])              # 49 and 39 valid frames
    alone = _store(fx, dtype)
    alone.add_recording(fx["rec130"], **LONG)
    mixed = _store(fx, dtype)
    mixed.add(b["input_values"], b["attention_mask_audio"])
    assert mixed.add_recording(fx["rec130"], **LONG) == 2
    mixed.add(b["input_values"], b["attention_mask_audio"])
    assert len(mixed) == 10 and mixed.recordings == 5 and mixed.rows == 88 + 130 + 88
    assert mixed.recording_of.tolist() == [0, 1] + [2] * 6 + [3, 4]
    assert mixed.offset_of.tolist() == [0, 0, 0, 20, 40, 60, 80, 100, 0, 0]
    assert mixed.seg_row.tolist() == [0, 49] + [88 + o for o in (0, 20, 40, 60, 80, 100)] + [218, 267]
    assert mixed.frames.tolist() == [49, 39] + [40] * 5 + [30] + [49, 39]
    for n, (st, m) in enumerate([(clips, 0), (clips, 1)] + [(alone, i) for i in range(6)] + [(clips, 0), (clips, 1)]):
        assert torch.equal(mixed.kv_rows(n), st.kv_rows(m)), n
        assert torch.equal(mixed.align_kv_rows(n), st.align_kv_rows(m)), n
        assert torch.equal(mixed.aproj[n], st.aproj[m]), n
        assert torch.equal(_unit(mixed, n), _unit(st, m)), n


# ------------------------------------------------------------------ search_recordings
@pytest.fixture(scope="module")
def archive(fx):
    """Clips, a 6-window and a 4-window recording, clips again: 14 windows of 6 recordings."""
    b = fx["batch"]
    st = _store(fx, "bf16")
    st.add(b["input_values"], b["attention_mask_audio"])
    st.add_recording(fx["rec130"], **LONG)
    st.add_recording(fx["rec90"], **LONG)
    st.add(b["input_values"], b["attention_mask_audio"])
    assert len(st) == 14 and st.recordings == 6
    assert st.recording_of.tolist() == [0, 1] + [2] * 6 + [3] * 4 + [4, 5]
    return st


def _stages(fx, store, k, m):
    from speech_transcript_embeddings_amd.retrieval import _unit_rows, best_per_recording, rerank_clips
    model = fx["model"]
    with model._eval_arithmetic():
        enc = model.encode_text(fx["ids"], fx["mask"])
    vals, idx = store.search(_unit_rows(enc[0]), m)
    vals, idx = rerank_clips(model, fx["ids"], fx["mask"], store, idx, text_encoded=enc)
    return best_per_recording(vals, idx, store.recording_of, k)


def _check_recording_time(store, wins, where):
    off = torch.where(wins >= 0, store.offset_of[wins.clamp(min=0).long()], 0)
    for name, o in (("hit", off[..., None]), ("token", off[..., None, None])):
        sp, sec = where[name + "_spans"], where[name + "_seconds"]
        assert torch.equal(where[f"recording_{name}_spans"], torch.where(sp < 0, sp, sp + o))
        assert torch.equal(where[f"recording_{name}_seconds"], torch.where(sp < 0, sec, sec + o.float() * 0.02))
        assert bool(((sp < 0) == (where[f"recording_{name}_spans"] < 0)).all())


@pytest.mark.parametrize("k", [3, 8])
def test_search_recordings_is_its_stages_composed_by_hand(fx, archive, k):
    from speech_transcript_embeddings_amd.retrieval import search_recordings
    model, store = fx["model"], archive
    m = min(4 * k, 128, 14)
    vals, recs, wins = _stages(fx, store, k, m)
    got = search_recordings(model, store, fx["ids"], fx["mask"], k, neighbours=False, word_ids=fx["wid"])
    assert torch.equal(got[0], vals) and torch.equal(got[1], recs) and torch.equal(got[2], wins)
    want = model.locate_clips(fx["ids"], fx["mask"], store, wins, word_ids=fx["wid"], free_ends=True)
    extra = {"recording_hit_spans", "recording_hit_seconds", "recording_token_spans", "recording_token_seconds"}
    assert set(got[3]) == set(want) | extra
    for key in want:
        assert torch.equal(got[3][key], want[key]), key
    _check_recording_time(store, wins, got[3])
    for row, wrow in zip(recs.tolist(), wins.tolist()):
        live = [r for r in row if r >= 0]
        assert len(live) == len(set(live))                               # no recording twice
        assert all(store.recording_of[w].item() == r for r, w in zip(row, wrow) if r >= 0)
    if k == 8:                                                           # 6 recordings: the tail is empty
        assert (recs[:, 6:] == -1).all() and (wins[:, 6:] == -1).all() and torch.isneginf(vals[:, 6:]).all()
        assert (recs[:, :6] >= 0).all()
        assert (got[3]["recording_hit_spans"][:, 6:] == -1).all() and (got[3]["path_score"][:, 6:] == NEG).all()
    else:
        assert (recs >= 0).all()
    assert (got[3]["recording_hit_spans"][:, :3] >= 0).all()
    print("windows:", wins.tolist(), "offsets:", store.offset_of[wins.clamp(min=0).long()].tolist())


def test_neighbours_keep_the_best_of_three_windows(fx, archive):
    from speech_transcript_embeddings_amd.retrieval import search_recordings
    model, store, k = fx["model"], archive, 3
    vals, recs, centre = _stages(fx, store, k, 12)
    rec_of = store.recording_of.tolist()

    def same(w, o):
        return o if w >= 0 and 0 <= o < 14 and rec_of[o] == rec_of[w] else -1

    left = [[same(w, w - 1) for w in row] for row in centre.tolist()]
    right = [[same(w, w + 1) for w in row] for row in centre.tolist()]
    cand = torch.cat([centre, torch.tensor(left, device=DEV, dtype=I32), torch.tensor(right, device=DEV, dtype=I32)], 1)
    three = model.locate_clips(fx["ids"], fx["mask"], store, cand, word_ids=fx["wid"], free_ends=True)
    got = search_recordings(model, store, fx["ids"], fx["mask"], k, word_ids=fx["wid"])
    assert torch.equal(got[0], vals) and torch.equal(got[1], recs)
    path = three["path_score"].view(4, 3, k)
    n_moved = 0
    for q in range(4):
        for c in range(k):
            p = path[q, :, c].tolist()
            j = p.index(max(p))                                          # the first maximum: centre, left, right
            assert got[2][q, c].item() == cand.view(4, 3, k)[q, j, c].item()
            assert got[3]["path_score"][q, c].item() == max(p)
            for key in three:
                assert torch.equal(got[3][key][q, c], three[key].view(4, 3, k, *three[key].shape[2:])[q, j, c]), key
            n_moved += j != 0
    print("neighbour windows kept:", n_moved, "of", 4 * k)
    _check_recording_time(store, got[2], got[3])
    gw = got[2]                                                          # the window kept is one of the hit's recording
    assert torch.equal(torch.where(gw >= 0, store.recording_of[gw.clamp(min=0).long()], -1), recs)


def test_the_other_switches_pass_through(fx, archive):
    from speech_transcript_embeddings_amd.retrieval import _unit_rows, best_per_recording, search_recordings
    model, store, k = fx["model"], archive, 3
    vals, recs, wins = _stages(fx, store, k, 12)
    # free_ends=False: the forced decode of the chosen windows, and no neighbours whatever the switch says
    got = search_recordings(model, store, fx["ids"], fx["mask"], k, free_ends=False, neighbours=True)
    want = model.locate_clips(fx["ids"], fx["mask"], store, wins)
    assert torch.equal(got[2], wins)
    for key in want:
        assert torch.equal(got[3][key], want[key]), key
    _check_recording_time(store, wins, got[3])
    # spot_bias reaches the decode
    got = search_recordings(model, store, fx["ids"], fx["mask"], k, neighbours=False, spot_bias=0.5)
    want = model.locate_clips(fx["ids"], fx["mask"], store, wins, free_ends=True, spot_bias=0.5)
    assert torch.equal(got[3]["path_score"], want["path_score"]) and torch.equal(got[3]["hit_spans"], want["hit_spans"])
    # locate=False
    got = search_recordings(model, store, fx["ids"], fx["mask"], k, locate=False)
    assert got[3] is None and torch.equal(got[0], vals) and torch.equal(got[2], wins)
    # rerank=False: stage 1's order; window_k: fewer windows searched
    with model._eval_arithmetic():
        enc = model.encode_text(fx["ids"], fx["mask"])
    for m in (12, 5):
        v1, i1 = store.search(_unit_rows(enc[0]), m)
        want = best_per_recording(v1, i1, store.recording_of, k)
        got = search_recordings(model, store, fx["ids"], fx["mask"], k, rerank=False, locate=False,
                                window_k=None if m == 12 else m)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], want))
    # attention_mask=None means every token valid
    full = torch.ones_like(fx["mask"])
    a = search_recordings(model, store, fx["ids"], None, k, locate=False)
    b = search_recordings(model, store, fx["ids"], full, k, locate=False)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------ refusals
def test_refusals(fx, monkeypatch):
    from speech_transcript_embeddings_amd import AudioStateStore
    meta, _ = load("align")
    model = mini_model(meta)                                             # its own model: a weight is touched below
    model.eval()
    x = fx["rec130"]
    store = AudioStateStore(model, DEV, align_rows=True)

    def untouched():
        return len(store) == 0 and store.rows == 0 and store.recordings == 0 and store._token is None

    with pytest.raises(ValueError, match="2048"):
        store.add_recording(x, window_frames=2049)
    with pytest.raises(ValueError):
        store.add_recording(x, window_frames=40, hop_frames=41)
    with pytest.raises(ValueError):
        store.add_recording(x, chunk_frames=0)
    with pytest.raises(ValueError):
        store.add_recording(x, chunk_batch=0)
    with pytest.raises(ValueError, match="ONE recording"):
        store.add_recording(torch.stack([x, x]))
    assert untouched()
    with monkeypatch.context() as mp:                                    # mean pooling
        mp.setattr(model, "use_attentive_pooling", False)
        with pytest.raises(ValueError, match="use_attentive_pooling"):
            store.add_recording(x, **LONG)
    with monkeypatch.context() as mp:                                    # a raw-waveform encoder
        mp.setattr(type(model.engine), "raw_audio", property(lambda self: True))
        with pytest.raises(ValueError, match="raw-waveform"):
            store.add_recording(x, **LONG)
    assert untouched()
    # without align_rows the window may be as long as the pooling kernel's segments
    plain = AudioStateStore(model, DEV)
    plain.add_recording(x, window_frames=2049, hop_frames=2049, chunk_frames=48, context_frames=8)
    assert len(plain) == 1 and plain.frames.tolist() == [130]
    with pytest.raises(ValueError, match="8192"):
        plain.add_recording(x, window_frames=8193)
    # a stale store
    store.add_recording(x, **LONG)
    with torch.no_grad():
        next(iter(model.parameters())).add_(0.0)                         # moves the version counter, not the value
    with pytest.raises(RuntimeError, match="other weights"):
        store.add_recording(x, **LONG)
    from speech_transcript_embeddings_amd.retrieval import search_recordings
    with pytest.raises(RuntimeError, match="other weights"):
        search_recordings(model, store, fx["ids"], fx["mask"], 2)
    assert len(store) == 6 and store.rows == 130
