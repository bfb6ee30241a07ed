"""Free-endpoint phrase spotting end to end (Engine.locate_clips / align_pairs with free_ends=True,
model.locate_clips / model.align, retrieval.search_clips) on the mini alignment model and
store of tests/test_locate_gpu.py: P = 128, 4 alignment heads, 2 clips of T = 49 frames (49 and 39
valid), 4 transcripts of L = 12 (12, 9, 12 and 9 tokens).

Strict, all of it: the token spans, the hit and the score are the numpy decode (kref_spot.spot_batch_ref)
of the route's own emissions against bg = -log(nfrm) + spot_bias evaluated in fp32 on the device, bit
for bit; scores, matrix and emit are the default mode's bits; free_ends=False is the call without the
argument, key by key; model.align(free_ends=True) and the segmented route give one result; empty and
infeasible slots are (-1, -1) / -inf."""
import numpy as np
import pytest
import torch

from kref_spot import spot_batch_ref
from test_locate_gpu import ALL, WORD_IDS
from test_model_gpu import batch_of, load, mini_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")
L, T = 12, 49


@pytest.fixture(scope="module")
def fx():
    """The model, the 4 transcripts, the store of the 2 clips, and locate_clips of every pair with the
    matrix and the emissions, in the default mode and with free ends; computed once."""
    from speech_transcript_embeddings_amd import AudioStateStore
    meta, z = load("align")
    model = mini_model(meta)
    model.eval()
    batch = batch_of(z)
    ids = torch.cat([batch["input_ids_pos"], batch["input_ids_neg"]])
    mask = torch.cat([batch["attention_mask_pos"], batch["attention_mask_neg"]])
    store = AudioStateStore(model, DEV, align_rows=True)
    store.add(batch["input_values"], batch["attention_mask_audio"])
    cand = torch.tensor(ALL, device=DEV)
    wid = torch.tensor(WORD_IDS, device=DEV)
    kw = dict(word_ids=wid, return_matrix=True, return_emit=True)
    return dict(model=model, batch=batch, ids=ids, mask=mask, store=store, cand=cand, wid=wid,
                forced=model.locate_clips(ids, mask, store, cand, **kw),
                free=model.locate_clips(ids, mask, store, cand, free_ends=True, **kw),
                ntok=mask.sum(1).tolist(), frames=store.frames.tolist())


def _locate(fx, cand=ALL, store=None, **kw):
    return fx["model"].locate_clips(fx["ids"], fx["mask"], store or fx["store"], torch.tensor(cand, device=DEV), **kw)


def _background(nfrm, bias=0.0):
    """-log(nfrm) + bias in fp32 on the device, the expression of Engine._spot."""
    f = torch.tensor(nfrm, dtype=torch.int32, device=DEV)
    return (-torch.log(f.clamp(min=1).to(torch.float32)) + float(bias)).cpu().numpy()


def _assert_is_the_reference(r, ntok, nfrm, lead=1, trail=1, bias=0.0):
    """r: a locate_clips dict with emit over len(ntok) x len(nfrm) pairs."""
    R = len(ntok) * len(nfrm)
    emit = r["emit"].reshape(R, -1, L).cpu().numpy()
    m = [max(n - lead - trail, 0) for n in ntok for _ in nfrm]
    F = list(nfrm) * len(ntok)
    rs, rh, rsc = spot_batch_ref(emit, m, F, _background(F, bias), lead, L)
    assert np.array_equal(r["token_spans"].reshape(R, L, 2).cpu().numpy(), rs)
    assert np.array_equal(r["hit_spans"].reshape(R, 2).cpu().numpy(), rh)
    assert np.array_equal(r["path_score"].reshape(R).cpu().numpy().view(np.int32), rsc.view(np.int32))
    return rs, rh, rsc


def test_free_ends_is_the_reference_decode_of_the_routes_emissions(fx):
    r = fx["free"]
    assert set(r) == set(fx["forced"])
    assert r["token_spans"].shape == (4, 2, L, 2) and r["token_spans"].dtype == torch.int32
    assert r["hit_spans"].shape == (4, 2, 2) and r["hit_spans"].dtype == torch.int32 and r["path_score"].shape == (4, 2)
    rs, rh, rsc = _assert_is_the_reference(r, fx["ntok"], fx["frames"])
    print("free-end hits:", rh.tolist(), "scores:", rsc.tolist(), "forced hits:",
          fx["forced"]["hit_spans"].reshape(8, 2).tolist())
    hs, sp = r["hit_spans"].cpu(), r["token_spans"].cpu()
    for u, n in enumerate(fx["ntok"]):
        for c, Fr in enumerate(fx["frames"]):
            assert 0 <= hs[u, c, 0] < hs[u, c, 1] <= Fr                          # inside the clip's own frames
            s = sp[u, c]
            assert bool((s[0] == -1).all()) and bool((s[n - 1:] == -1).all())    # <s>, </s> and the padding
            assert hs[u, c].tolist() == [int(s[1, 0]), int(s[n - 2, 1])]
            assert bool((s[1:n - 1, 1] > s[1:n - 1, 0]).all()) and torch.equal(s[2:n - 1, 0], s[1:n - 2, 1])
    assert torch.equal(r["token_seconds"].cpu(), torch.where(sp < 0, -1.0, sp.float() * 0.02))
    assert torch.equal(r["hit_seconds"].cpu(), torch.where(hs < 0, -1.0, hs.float() * 0.02))


def test_everything_but_the_decode_is_the_default_modes(fx):
    for k in ("scores", "emit", "matrix"):
        assert torch.equal(fx["free"][k], fx["forced"][k]), k


def test_spot_bias_shifts_the_background_and_nothing_else(fx):
    for bias in (0.75, -1.5):
        r = _locate(fx, spot_bias=bias, free_ends=True, return_emit=True)
        _assert_is_the_reference(r, fx["ntok"], fx["frames"], bias=bias)
        assert torch.equal(r["emit"], fx["free"]["emit"]) and torch.equal(r["scores"], fx["free"]["scores"])
    # a higher bar never lengthens the hit's score: the gain of every frame falls by the same amount
    hi = _locate(fx, spot_bias=0.75, free_ends=True)["path_score"]
    assert bool((hi <= fx["free"]["path_score"]).all())
    # the default mode does not read it
    a, b = _locate(fx, spot_bias=3.0), _locate(fx)
    for k in b:
        assert torch.equal(a[k], b[k]), k


def test_lead_and_trail_choose_the_phrase(fx):
    for lead, trail in ((0, 0), (2, 3), (4, 4)):
        r = _locate(fx, lead=lead, trail=trail, free_ends=True, return_emit=True)
        _assert_is_the_reference(r, fx["ntok"], fx["frames"], lead, trail)
    # 9 tokens, lead + trail = 9: no phrase token is left
    r = _locate(fx, lead=5, trail=4, free_ends=True)
    for u, n in enumerate(fx["ntok"]):
        if n == 9:
            assert (r["token_spans"][u] == -1).all() and (r["hit_spans"][u] == -1).all()
            assert (r["path_score"][u] == NEG).all()
        else:
            assert (r["hit_spans"][u] >= 0).all()
    r = _locate(fx, lead=12, trail=0, free_ends=True)                           # beyond the last column
    assert (r["token_spans"] == -1).all() and (r["hit_spans"] == -1).all() and (r["path_score"] == NEG).all()
    with pytest.raises(ValueError, match="lead and trail"):
        _locate(fx, lead=-1, free_ends=True)


def test_empty_and_infeasible_slots(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    cand = [[0, -1, 1], [-1, -1, -1], [1, 1, 0], [-1, 0, -1]]
    r = _locate(fx, cand, word_ids=fx["wid"], free_ends=True)
    full = fx["free"]
    for u, row in enumerate(cand):
        for c, n in enumerate(row):
            if n < 0:
                assert (r["token_spans"][u, c] == -1).all() and (r["token_seconds"][u, c] == -1).all()
                assert (r["hit_spans"][u, c] == -1).all() and (r["hit_seconds"][u, c] == -1).all()
                assert r["path_score"][u, c].item() == NEG and (r["scores"][u, c] == 0).all()
                assert (r["word_spans"][u, c] == -1).all() and (r["word_scores"][u, c] == 0).all()
            else:                                    # the same pair wherever it sits in the candidate lists
                for k in ("token_spans", "path_score", "hit_spans", "word_spans"):
                    assert torch.equal(r[k][u, c], full[k][u, n]), k
    none = _locate(fx, [[-1]] * 4, free_ends=True)
    assert (none["token_spans"] == -1).all() and (none["path_score"] == NEG).all() and (none["hit_spans"] == -1).all()
    # a clip of 10 valid frames: with lead = trail = 0 infeasible for the 12-token phrases, feasible for the
    # 9-token ones; without <s> / </s> the 10 tokens of the long phrases just fit
    b = fx["batch"]
    am = b["attention_mask_audio"].clone()
    am[1, 10:] = 0
    st = AudioStateStore(fx["model"], DEV, align_rows=True)
    st.add(b["input_values"], am)
    assert st.frames.tolist() == [49, 10]
    r = _locate(fx, ALL, st, lead=0, trail=0, free_ends=True, return_emit=True)
    _assert_is_the_reference(r, fx["ntok"], [49, 10], 0, 0)
    for u, n in enumerate(fx["ntok"]):
        if n > 10:
            assert (r["token_spans"][u, 1] == -1).all() and r["path_score"][u, 1].item() == NEG
            assert (r["hit_spans"][u, 1] == -1).all()
        else:
            assert (r["hit_spans"][u, 1] >= 0).all() and r["hit_spans"][u, 1, 1].item() <= 10
    r = _locate(fx, ALL, st, free_ends=True, return_emit=True)
    _assert_is_the_reference(r, fx["ntok"], [49, 10])
    assert r["hit_spans"][0, 1].tolist() == [0, 10]


def test_free_ends_false_is_the_call_without_it(fx):
    model, b = fx["model"], fx["batch"]
    kw = dict(word_ids=fx["wid"], return_matrix=True, return_emit=True)
    off = model.locate_clips(fx["ids"], fx["mask"], fx["store"], fx["cand"], free_ends=False, **kw)
    assert set(off) == set(fx["forced"])
    for k in off:
        assert torch.equal(off[k], fx["forced"][k]), k
    args = (b["input_values"], b["attention_mask_audio"], fx["ids"][:2], fx["mask"][:2])
    akw = dict(word_ids=fx["wid"][:2], return_matrix=True)
    plain, off = model.align(*args, **akw), model.align(*args, free_ends=False, lead=3, trail=2, spot_bias=1.0, **akw)
    assert set(plain) == set(off) and "hit_spans" not in plain
    for k in plain:
        assert torch.equal(plain[k], off[k]), k


def test_dense_and_segmented_routes_agree(fx):
    """model.align(free_ends=True) on the 8 pairs (pair (u, b) at row 2u + b) against the store's route."""
    model, b = fx["model"], fx["batch"]
    tix, aix = [u for u in range(4) for _ in range(2)], [0, 1] * 4
    wid = fx["wid"][tix].contiguous()
    args = (b["input_values"][aix].contiguous(), b["attention_mask_audio"][aix].contiguous(),
            fx["ids"][tix].contiguous(), fx["mask"][tix].contiguous())
    dense = model.align(*args, word_ids=wid, return_matrix=True, free_ends=True)
    forced = model.align(*args, word_ids=wid, return_matrix=True)
    assert set(dense) == set(forced) | {"hit_spans", "hit_seconds"}
    assert torch.equal(dense["scores"], forced["scores"]) and torch.equal(dense["matrix"], forced["matrix"])
    seg = fx["free"]
    for k in ("token_spans", "hit_spans", "path_score", "token_seconds", "hit_seconds", "word_spans"):
        assert torch.equal(dense[k], seg[k].reshape(dense[k].shape)), k
    # other arguments reach the dense route as they reach the segmented one
    d2 = model.align(*args, free_ends=True, lead=2, trail=3, spot_bias=-0.5)
    s2 = _locate(fx, free_ends=True, lead=2, trail=3, spot_bias=-0.5)
    for k in ("token_spans", "hit_spans", "path_score"):
        assert torch.equal(d2[k], s2[k].reshape(d2[k].shape)), k


def test_mx8_store(fx):
    from speech_transcript_embeddings_amd import AudioStateStore
    b = fx["batch"]
    st = AudioStateStore(fx["model"], DEV, align_rows=True, align_dtype="mx8")
    st.add(b["input_values"], b["attention_mask_audio"])
    r = _locate(fx, ALL, st, free_ends=True, return_emit=True)
    _assert_is_the_reference(r, fx["ntok"], fx["frames"])
    forced = _locate(fx, ALL, st, return_emit=True)
    assert torch.equal(r["emit"], forced["emit"]) and torch.equal(r["scores"], forced["scores"])


def test_search_clips_passes_the_arguments_through(fx):
    from speech_transcript_embeddings_amd import search_clips
    model, store = fx["model"], fx["store"]
    vals, idx, where = search_clips(model, store, fx["ids"], fx["mask"], 3, word_ids=fx["wid"], free_ends=True,
                                    spot_bias=0.25)
    want = model.locate_clips(fx["ids"], fx["mask"], store, idx, word_ids=fx["wid"], free_ends=True, spot_bias=0.25)
    assert set(where) == set(want)
    for k in want:
        assert torch.equal(where[k], want[k]), k
    assert (where["hit_spans"][:, 2] == -1).all() and (where["hit_spans"][:, :2] >= 0).all()
    v0, i0, w0 = search_clips(model, store, fx["ids"], fx["mask"], 3, word_ids=fx["wid"])
    assert torch.equal(v0, vals) and torch.equal(i0, idx)
    assert torch.equal(w0["scores"], where["scores"]) and not torch.equal(w0["token_spans"], where["token_spans"])


def test_words_cover_phrase_tokens_only(fx):
    """word_* come through words_from_tokens unchanged: a token without a span (lead, trail, padding)
    gives its word nothing."""
    lead, trail = 2, 1
    r = _locate(fx, word_ids=fx["wid"], lead=lead, trail=trail, free_ends=True)
    sp, sc = r["token_spans"].cpu(), r["scores"].cpu()
    ws, wsc = r["word_spans"].cpu(), r["word_scores"].cpu()
    W = ws.shape[2]
    for u, n in enumerate(fx["ntok"]):
        for c in range(2):
            for w in range(W):
                toks = [l for l in range(lead, n - trail) if WORD_IDS[u][l] == w]
                assert all(sp[u, c, l, 0] >= 0 for l in toks)
                if not toks:
                    assert ws[u, c, w].tolist() == [-1, -1] and wsc[u, c, w] == 0
                    continue
                assert ws[u, c, w].tolist() == [min(int(sp[u, c, l, 0]) for l in toks),
                                                max(int(sp[u, c, l, 1]) for l in toks)]
                assert abs(float(wsc[u, c, w]) - float(sc[u, c, toks].mean())) < 1e-6
    # transcript 2's word 0 is token 1 alone, inside lead: no span; transcript 0's word 0 keeps token 2 only
    assert (ws[2, :, 0] == -1).all()
    assert torch.equal(ws[0, :, 0], sp[0, :, 2])
