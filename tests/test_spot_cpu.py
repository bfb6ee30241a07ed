"""Free-endpoint phrase spotting without a GPU: the reference of tests/kref_spot.py pinned
to a brute-force enumeration of every (start, end, monotone path), the planted phrase that the forced
decode misplaces, the tie rules and the infeasible-pair conventions, the ste::align_spot schema and fake
implementation, the C ABI of ste_align_spot (declared, exported, in the ctypes table, contract violations
returned before any launch) and ops.align_spot's argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from kref_align import planted, viterbi_ref
from kref_spot import gain_sum, spot_batch_ref, spot_paths, spot_ref
from speech_transcript_embeddings_amd import torch_ops
from speech_transcript_embeddings_amd.align import hit_spans

ERR_ARG, ERR_SHAPE = 1001, 1002


# ------------------------------------------------------------------ the reference
def test_spot_ref_against_all_hits():
    """F <= 8, m <= 4, lead in {0, 1, 2}, padding columns on both sides, emissions and bg multiples of
    1/4 (every float32 sum exact, many ties): the score is the best over every (start, end, monotone
    path), the returned spans are one such hit and attain it, and the end is the earliest that does."""
    rng = np.random.default_rng(22)
    cases = 0
    for rep in range(8):
        for m in range(1, 5):
            for F in range(m, 9):
                lead = int(rng.integers(0, 3))
                pad = int(rng.integers(0, 3))
                e = (rng.integers(-24, 5, (F + 1, lead + m + pad)) / 4).astype(np.float32)
                e[F] = np.nan                                      # a frame past nfrm
                bg = float(rng.integers(-16, 1)) / 4
                spans, hit, score = spot_ref(e, m, F, bg, lead)
                hits = [(gain_sum(e, b, bg, lead), end) for _, end, b in spot_paths(m, F)]
                top = max(s for s, _ in hits)
                assert score == top, (m, F, lead, bg)
                assert hit[1] == min(end for s, end in hits if s == top)
                assert (spans[:, 1] > spans[:, 0]).all() and np.array_equal(spans[1:, 0], spans[:-1, 1])
                assert hit == (spans[0, 0], spans[-1, 1]) and 0 <= hit[0] and hit[1] <= F
                assert gain_sum(e, np.append(spans[:, 0], spans[-1, 1]), bg, lead) == score
                cases += 1
    assert cases >= 200


@pytest.mark.parametrize("bg", [-1.0, -2.5, -4.0])
def test_planted_phrase_is_found_where_the_forced_decode_misplaces_it(bg):
    """A 6-token, 40-frame path at frames 77..117 of a 200-frame clip, in columns 1..6 of a -5 background
    with flat <s> / </s> columns: the free-endpoint decode reports (77, 117) for every background level
    between the path's 0 and the clip's -5; the forced decode + hit_spans starts the phrase at frame 1."""
    p, want = planted(12, 200, 6, 40, seed=3)
    e = np.full((200, 12), -5.0, dtype=np.float32)
    e[77:117, 1:7] = p[:40, :6]
    spans, hit, score = spot_ref(e, 6, 200, bg, lead=1)
    assert hit == (77, 117) and np.array_equal(spans, want + 77)
    assert score == np.float32(40 * -bg)
    sb, hb, _ = spot_batch_ref(e[None], [6], [200], [bg], 1, 12)
    assert hb.tolist() == [[77, 117]] and np.array_equal(sb[0, 1:7], want + 77)
    assert (sb[0, 0] == -1).all() and (sb[0, 7:] == -1).all()
    forced, _, _ = viterbi_ref(e, 8, 200)
    fh = hit_spans(torch.from_numpy(forced)[None], torch.tensor([8]))[0].tolist()
    print(f"bg {bg}: free ends {hit}, forced decode + hit_spans {fh}")
    assert fh == [1, 117]


def test_ties_stay_and_the_earliest_end_wins():
    """All gains zero: every hit scores 0; token 0 never restarts (0 > 0 is false), every later token
    advances only on a strict improvement, and the first frame that attains the maximum is the end."""
    for m, F, lead in ((1, 1, 0), (3, 6, 0), (4, 4, 2), (2, 9, 1)):
        e = np.full((F, lead + m + 1), -1.5, dtype=np.float32)
        spans, hit, score = spot_ref(e, m, F, -1.5, lead)
        assert hit == (0, m) and score == 0.0
        assert spans.tolist() == [[j, j + 1] for j in range(m)]
    # a background above every emission: the shortest hit loses least, the earliest one wins the tie
    spans, hit, score = spot_ref(np.full((7, 3), -2.0, dtype=np.float32), 3, 7, -1.0)
    assert hit == (0, 3) and score == -3.0


def test_spot_batch_ref_conventions():
    e = np.zeros((6, 6, 5), dtype=np.float32)
    bg = np.full(6, -1.0, dtype=np.float32)
    #             ok  m<1  lead+m>L  F<m  F>T  ok
    ntok, nfrm = [3, 0, 5, 4, 2, 4], [6, 6, 6, 3, 7, 4]
    spans, hit, score = spot_batch_ref(e, ntok, nfrm, bg, 1, 5)
    assert spans[0].tolist() == [[-1, -1], [0, 1], [1, 2], [2, 6], [-1, -1]]
    assert hit[0].tolist() == [0, 6] and score[0] == 6.0
    assert (spans[1:5] == -1).all() and (hit[1:5] == -1).all() and np.isneginf(score[1:5]).all()
    assert hit[5].tolist() == [0, 4] and score[5] == 4.0 and (spans[5, 0] == -1).all()
    # emissions of -inf only: no D_t[m-1] above -inf, no hit
    spans, hit, score = spot_batch_ref(np.full((1, 4, 3), -np.inf, dtype=np.float32), [2], [4], [-1.0], 0, 3)
    assert (spans == -1).all() and (hit == -1).all() and np.isneginf(score).all()


# ------------------------------------------------------------------ torch op
def test_op_schema_and_fake():
    assert "align_spot" in torch_ops.OPS
    s = str(torch.ops.ste.align_spot.default._schema)
    assert s == ("ste::align_spot(Tensor emit, Tensor ntok, Tensor nfrm, Tensor bg, SymInt lead=0) -> "
                 "(Tensor, Tensor, Tensor)"), s
    with FakeTensorMode():
        B, L, T = 3, 12, 49
        e, n = torch.empty(B, T, L), torch.empty(B, dtype=torch.int32)
        for kw in ({}, {"lead": 1}):
            spans, hit, score = torch.ops.ste.align_spot(e, n, n, torch.empty(B), **kw)
            assert spans.shape == (B, L, 2) and spans.dtype == torch.int32
            assert hit.shape == (B, 2) and hit.dtype == torch.int32
            assert score.shape == (B,) and score.dtype == torch.float32


# ------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_bound():
    from pathlib import Path

    from speech_transcript_embeddings_amd import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "ste.h").read_text()
    assert "int ste_align_spot(" in header
    assert "ste_align_spot" in _lib.SYMBOLS and len(_lib._SIGS["ste_align_spot"][1]) == 13
    assert _lib._SIGS["ste_align_spot"][0] is C.c_int
    assert _lib.fn("ste_align_spot") is not None                 # exported by libste.so


def test_argument_errors_return_status_without_launch():
    """No GPU here: a launch would fail differently.  Pointers are never dereferenced."""
    from speech_transcript_embeddings_amd import _lib
    spot = _lib.fn("ste_align_spot")
    A = 1 << 20

    def call(emit=A, lde=None, ntok=A, nfrm=A, bg=A, lead=1, B=2, L=9, T=17, spans=A, hit=A, score=A):
        return spot(emit, L if lde is None else lde, ntok, nfrm, bg, lead, B, L, T, spans, hit, score, None)

    for name in ("emit", "ntok", "nfrm", "bg", "spans", "hit", "score"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(L=257) == ERR_SHAPE and call(T=2049) == ERR_SHAPE and call(lde=8) == ERR_SHAPE
    assert call(B=0) == ERR_SHAPE and call(L=0) == ERR_SHAPE and call(T=0) == ERR_SHAPE
    assert call(lead=-1) == ERR_SHAPE and call(lead=9) == ERR_SHAPE


def test_ops_align_spot_argument_errors():
    from speech_transcript_embeddings_amd import ops
    B, T, L = 2, 5, 4
    e = torch.zeros(B, T, L)
    n, f, bg = torch.ones(B, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32), torch.zeros(B)
    with pytest.raises(ValueError, match=r"\[B, T, L\]"):
        ops.align_spot(e[0], n, f, bg)
    for lead in (-1, L):
        with pytest.raises(ValueError, match="lead"):
            ops.align_spot(e, n, f, bg, lead)
    with pytest.raises(ValueError, match="float32"):
        ops.align_spot(e.double(), n, f, bg)
    with pytest.raises(ValueError, match="float32"):
        ops.align_spot(e, n, f, bg.double())
    with pytest.raises(ValueError, match="int32"):
        ops.align_spot(e, n.long(), f, bg)
    with pytest.raises(ValueError, match="one entry per pair"):
        ops.align_spot(e, n, f, bg[:1])
    with pytest.raises(ValueError, match="one entry per pair"):
        ops.align_spot(e, n[:1], f, bg)
