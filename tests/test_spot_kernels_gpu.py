"""Kernel parity of the free-endpoint decode (csrc/align_spot.hip): ste_align_spot alone
against tests/kref_spot.py.

BIT-exact: both sides do the same fp32 subtract and add per cell and the same two strict comparisons,
so spans, hit and score are compared with array_equal.  Which shape reaches which branch: L <= 64 is
the one-token-per-lane kernel, L > 64 the four-token one (64 | 65); there lde % 4 == 0 with
lead % 4 == 0 takes the 16-byte row loads (L = 256 with every lane live, L = 65 in lde = 68 with a
lane straddling L and lanes past it), any other lde or lead the scalar loads.  m puts token m - 1 on
lane 0 (m = 1, and 4 of the four-token kernel), on lane 63 (m = 64, 253..256), on a lane's first slot
(m = 5, 65, 253) and its last (m = 4, 64, 256).  F = m and m + 1 are the shortest feasible clips;
1, 7, 8, 9, 16, 17 (and m + 7, m + 9, m + 16) run the 8-row pipeline's tail alone, one and two whole
chunks and the tails after them; F = 2048 with L > 64 is the LDS limit (64 KiB of advance bits).
Every pair's rows from nfrm on are NaN, and every call checks a guard region after each output."""
import numpy as np
import pytest
import torch

from kref_align import planted
from kref_spot import spot_batch_ref
from test_w2v2_kernels_gpu import DEV, ERR_SHAPE, F32, _p, _s

pytestmark = pytest.mark.gpu
I32 = torch.int32
ERR_ARG = 1001
GUARD = 64
LOG_FLT_MIN = float(np.log(np.float32(np.finfo(np.float32).tiny)))


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops
    return ops


def _spot(lib, emit, L, ntok, nfrm, bg, lead):
    """ste_align_spot on emit (numpy float32 [B, T, lde]) -> (spans [B, L, 2], hit [B, 2], score [B]) as
    numpy; the GUARD elements after each output must come back untouched."""
    B, T, lde = emit.shape
    e = torch.from_numpy(np.ascontiguousarray(emit)).to(DEV)
    nt = torch.tensor(list(ntok), dtype=I32, device=DEV)
    nf = torch.tensor(list(nfrm), dtype=I32, device=DEV)
    g = torch.tensor(list(bg), dtype=F32, device=DEV)
    spans = torch.full((B * L * 2 + GUARD,), 77, dtype=I32, device=DEV)
    hit = torch.full((B * 2 + GUARD,), 77, dtype=I32, device=DEV)
    score = torch.full((B + GUARD,), 7.0, dtype=F32, device=DEV)
    rc = lib.fn("ste_align_spot")(_p(e), lde, _p(nt), _p(nf), _p(g), lead, B, L, T, _p(spans), _p(hit), _p(score),
                                  _s(lib))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((spans[B * L * 2:] == 77).all()) and bool((hit[B * 2:] == 77).all()) and bool((score[B:] == 7.0).all())
    return (spans[:B * L * 2].view(B, L, 2).cpu().numpy(), hit[:B * 2].view(B, 2).cpu().numpy(),
            score[:B].cpu().numpy())


def _check(lib, emit, L, ntok, nfrm, bg, lead):
    bg = np.asarray(bg, dtype=np.float32)
    spans, hit, score = _spot(lib, emit, L, ntok, nfrm, bg, lead)
    rs, rh, rsc = spot_batch_ref(emit, ntok, nfrm, bg, lead, L)
    assert np.array_equal(spans, rs), np.argwhere(spans != rs)[:5]
    assert np.array_equal(hit, rh), (hit, rh)
    assert np.array_equal(score.view(np.int32), rsc.view(np.int32)), (score, rsc)     # the same bits
    return spans, hit, score


def _emissions(kind, B, T, lde, nfrm, seed):
    """[B, T, lde] with NaN in every row from the pair's nfrm on.  "normal": N(0, 1); "logsm": the log of a
    sharp softmax over the pair's frames per column, clamped at FLT_MIN as the matrix kernels clamp."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((B, T, lde)).astype(np.float32)
    for b, F in enumerate(nfrm):
        F = min(max(F, 0), T)
        if kind == "logsm" and F:
            z = (e[b, :F] * 40.0).astype(np.float64)
            p = np.exp(z - z.max(0)) / np.exp(z - z.max(0)).sum(0)
            e[b, :F] = np.log(np.maximum(p, np.finfo(np.float32).tiny)).astype(np.float32)
        e[b, F:] = np.nan
    return e


def _background(kind, nfrm):
    return [-0.3 if kind == "normal" else -float(np.log(np.float32(max(F, 1)))) for F in nfrm]


# (L, lde - L, lead, m): see the module docstring
SHAPES = [(5, 0, 0, 1), (5, 3, 1, 4), (5, 0, 0, 5), (5, 3, 4, 1), (5, 0, 3, 2),
          (64, 0, 0, 64), (64, 3, 1, 5), (64, 0, 3, 61), (64, 3, 4, 60), (64, 0, 1, 63), (64, 0, 0, 4),
          (65, 0, 0, 65), (65, 3, 0, 65), (65, 3, 1, 64), (65, 0, 4, 5), (65, 3, 3, 4), (65, 3, 4, 61), (65, 3, 4, 1),
          (256, 0, 0, 256), (256, 0, 4, 252), (256, 0, 1, 255), (256, 3, 3, 253), (256, 0, 0, 65), (256, 0, 4, 64),
          (256, 0, 0, 1), (256, 3, 0, 4), (256, 0, 0, 5)]


@pytest.mark.parametrize("kind", ["normal", "logsm"])
@pytest.mark.parametrize("L,pad,lead,m", SHAPES)
def test_spot_matches_reference_bitwise(lib, L, pad, lead, m, kind):
    nfrm = sorted({m, m + 1, 1, 7, 8, 9, 16, 17, m + 7, m + 9, m + 16})
    B, T = len(nfrm), max(nfrm) + 1
    e = _emissions(kind, B, T, L + pad, nfrm, seed=L * 31 + lead * 7 + m)
    if kind == "logsm":
        assert abs(float(np.nanmin(e)) - LOG_FLT_MIN) < 1e-4           # the clamp is reached
    spans, hit, score = _check(lib, e, L, [m] * B, nfrm, _background(kind, nfrm), lead)
    for b, F in enumerate(nfrm):
        s = spans[b, lead:lead + m]
        if F < m:
            assert (spans[b] == -1).all() and (hit[b] == -1).all() and np.isneginf(score[b])
            continue
        assert (spans[b, :lead] == -1).all() and (spans[b, lead + m:] == -1).all()
        assert (s[:, 1] > s[:, 0]).all() and np.array_equal(s[1:, 0], s[:-1, 1])      # contiguous, non-empty
        assert hit[b].tolist() == [s[0, 0], s[-1, 1]] and 0 <= hit[b, 0] and hit[b, 1] <= F
        if F == m:
            assert hit[b].tolist() == [0, m]                                      # only the diagonal exists


def test_spot_at_the_frame_limit(lib):
    """T = 2048 with L = 256: 64 KiB of advance bits, 256 whole chunks of the pipeline (F = 2048) and a
    7-frame tail after 255 (F = 2047)."""
    L, T, lead = 256, 2048, 4
    nfrm, ntok = [2048, 2047], [252, 5]
    e = _emissions("normal", 2, T, L, nfrm, seed=9)
    _, hit, score = _check(lib, e, L, ntok, nfrm, [-0.3, 0.4], lead)
    assert (hit >= 0).all() and np.isfinite(score).all()


def _pattern_cases():
    return [(5, 0, 1, 3, 40), (64, 3, 0, 64, 150), (130, 2, 4, 100, 300), (200, 0, 3, 70, 170)]


@pytest.mark.parametrize("L,pad,lead,m,F", _pattern_cases())
def test_spot_patterns_by_construction(lib, L, pad, lead, m, F):
    """Five gain patterns in one batch (bg = -1; emissions are multiples of 1/2, every sum exact):
    0 the maximum at frame m - 1: +3 on the diagonal, -4 everywhere else -> (0, m);
    1 the maximum at the last frame: +1 everywhere -> (0, F);
    2 a hit from frame 0: a planted path over the first m + 9 frames, -4 off it -> (0, m + 9);
    3 a late fresh start: -60 for s frames, then a planted path over m + 5 frames, -4 after -> (s, s+m+5);
    4 all gains equal to zero -> (0, m) by the two strict rules."""
    T, bg = F + 2, -1.0
    s = F - (m + 5) - 3
    e = np.full((5, T, L + pad), np.nan, dtype=np.float32)
    cols = slice(lead, lead + m)
    e[0, :F, :L] = -5.0
    e[0, np.arange(m), lead + np.arange(m)] = 2.0
    e[1, :F, :L] = 0.0
    p2, w2 = planted(m, m + 9, m, m + 9, seed=L)
    e[2, :F, :L] = -5.0
    e[2, :m + 9, cols] = np.where(p2 == 0.0, 1.0, -5.0)
    p3, w3 = planted(m, m + 5, m, m + 5, seed=L + 1)
    e[3, :F, :L] = -5.0
    e[3, :s, :L] = -61.0
    e[3, s:s + m + 5, cols] = np.where(p3 == 0.0, 1.0, -5.0)
    e[4, :F, :L] = -1.0
    spans, hit, score = _check(lib, e, L, [m] * 5, [F] * 5, [bg] * 5, lead)
    assert hit.tolist() == [[0, m], [0, F], [0, m + 9], [s, s + m + 5], [0, m]]
    assert score.tolist() == [3.0 * m, 1.0 * F, 2.0 * (m + 9), 2.0 * (m + 5), 0.0]
    assert np.array_equal(spans[2, cols], w2) and np.array_equal(spans[3, cols], w3 + s)
    assert spans[0, cols].tolist() == spans[4, cols].tolist() == [[j, j + 1] for j in range(m)]


def test_planted_phrase_through_the_kernel(lib):
    """The case of tests/test_spot_cpu.py: a 6-token, 40-frame path at frames 77..117 of 200, columns 1..6,
    in a -5 background; every background level between the two finds (77, 117)."""
    p, want = planted(12, 200, 6, 40, seed=3)
    e = np.full((200, 12), -5.0, dtype=np.float32)
    e[77:117, 1:7] = p[:40, :6]
    bgs = [-1.0, -2.5, -4.0]
    spans, hit, score = _check(lib, np.stack([e] * 3), 12, [6] * 3, [200] * 3, bgs, 1)
    assert hit.tolist() == [[77, 117]] * 3 and score.tolist() == [40.0, 100.0, 160.0]
    for b in range(3):
        assert np.array_equal(spans[b, 1:7], want + 77)


@pytest.mark.parametrize("L,lead", [(9, 1), (70, 4), (70, 2)])
def test_spot_ragged_batch_with_infeasible_pairs(lib, L, lead):
    """Feasible pairs of several lengths between infeasible ones, each for another reason: no token, a
    negative count, more tokens than columns from lead, fewer frames than tokens, more frames than rows,
    no frame."""
    T = 90
    ntok = [4, 0, L - lead, -3, L - lead + 1, 6, 1, 5, 3, 2]
    nfrm = [40, 20, T, 10, T, 5, 13, T + 1, 3, 0]
    e = _emissions("normal", len(ntok), T, L, nfrm, seed=L)
    spans, hit, score = _check(lib, e, L, ntok, nfrm, [-0.2] * len(ntok), lead)
    for b in (1, 3, 4, 5, 7, 9):
        assert (spans[b] == -1).all() and (hit[b] == -1).all() and np.isneginf(score[b])
    for b in (0, 2, 6, 8):
        assert (hit[b] >= 0).all() and np.isfinite(score[b])
    assert hit[8].tolist() == [0, 3]


@pytest.mark.parametrize("L,pad,lead,m", [(40, 3, 2, 30), (64, 0, 1, 62), (130, 2, 4, 100), (130, 3, 3, 90)])
def test_spot_ignores_the_other_columns(lib, L, pad, lead, m):
    """Columns outside lead .. lead+m-1 (the lead / trail tokens, the padding tokens and the row's padding)
    hold NaN, or a sentinel that would win every comparison if it were a token."""
    T, F = 50 + m, 47 + m
    rng = np.random.default_rng(L + lead)
    core = rng.standard_normal((2, T, m)).astype(np.float32)
    out = []
    for fill in (0.0, np.nan, 1e30):
        e = np.full((2, T, L + pad), fill, dtype=np.float32)
        e[:, :, lead:lead + m] = core
        out.append(_spot(lib, e, L, [m, m - 1], [F, T], [-0.3, 0.1], lead))
    rs, rh, rsc = spot_batch_ref(np.ascontiguousarray(np.pad(core, ((0, 0), (0, 0), (lead, L - lead - m)))),
                                 [m, m - 1], [F, T], np.float32([-0.3, 0.1]), lead, L)
    # pair 1 has m - 1 tokens: column lead+m-1 holds real emissions and is not one of its tokens either
    for spans, hit, score in out:
        assert np.array_equal(spans, rs) and np.array_equal(hit, rh) and score.tobytes() == rsc.tobytes()


@pytest.mark.parametrize("L,lead", [(40, 1), (130, 4), (130, 1)])
def test_spot_pair_is_independent_of_the_batch(lib, L, lead):
    T = 90
    n = L - lead
    ntok, nfrm = [n, 7, n - 9, 1, 30], [T, 50, 77, 3, 64]
    e = _emissions("normal", 5, T, L, nfrm, seed=L + lead)
    bg = [-0.3, 0.0, -1.0, 0.5, -0.1]
    spans, hit, score = _check(lib, e, L, ntok, nfrm, bg, lead)
    for b in (0, 2):
        one = _spot(lib, e[b:b + 1], L, [ntok[b]], [nfrm[b]], [bg[b]], lead)
        assert np.array_equal(one[0][0], spans[b]) and np.array_equal(one[1][0], hit[b])
        assert one[2][0].tobytes() == score[b].tobytes()
    perm = [4, 2, 0, 3, 1]
    ps, ph, psc = _spot(lib, e[perm], L, [ntok[i] for i in perm], [nfrm[i] for i in perm], [bg[i] for i in perm], lead)
    assert np.array_equal(ps, spans[perm]) and np.array_equal(ph, hit[perm]) and psc.tobytes() == score[perm].tobytes()


def test_ops_wrapper_and_custom_op(ops):
    L, T, lead = 12, 33, 1
    e = np.random.default_rng(2).standard_normal((3, T, L + 4)).astype(np.float32)
    ntok, nfrm, bg = [10, 4, 9], [33, 20, 9], np.float32([-0.3, 0.2, -1.0])
    rs, rh, rsc = spot_batch_ref(e, ntok, nfrm, bg, lead, L)
    ed = torch.from_numpy(e).to(DEV)
    nt, nf = torch.tensor(ntok, dtype=I32, device=DEV), torch.tensor(nfrm, dtype=I32, device=DEV)
    g = torch.from_numpy(bg).to(DEV)
    spans, hit, score = ops.align_spot(ed[:, :, :L], nt, nf, g, lead)             # a column view: lde = L + 4
    assert spans.dtype == I32 and hit.dtype == I32 and score.dtype == F32
    assert np.array_equal(spans.cpu().numpy(), rs) and np.array_equal(hit.cpu().numpy(), rh)
    assert np.array_equal(score.cpu().numpy(), rsc)
    s2, h2, c2 = torch.ops.ste.align_spot(ed[:, :, :L], nt.long(), nf.long(), g, lead)
    assert s2.dtype == I32 and torch.equal(s2, spans) and torch.equal(h2, hit) and torch.equal(c2, score)
    s0, h0, c0 = ops.align_spot(ed[:, :, :L], nt, nf, g)                          # lead defaults to 0
    r0 = spot_batch_ref(e, ntok, nfrm, bg, 0, L)
    assert np.array_equal(s0.cpu().numpy(), r0[0]) and np.array_equal(h0.cpu().numpy(), r0[1])
    assert torch.equal(torch.ops.ste.align_spot(ed[:, :, :L], nt, nf, g)[1], h0)


def test_spot_limits_and_argument_errors(lib, ops):
    """Status codes and exceptions only: none of these launches a kernel, and the buffers stay untouched."""
    t = torch.zeros(1 << 12, device=DEV)
    n = torch.ones(4, dtype=I32, device=DEV)
    f = lib.fn("ste_align_spot")

    def call(emit=t, lde=8, ntok=n, nfrm=n, bg=t, lead=0, B=1, L=8, T=4, spans=t, hit=t, score=t):
        return f(_p(emit), lde, _p(ntok), _p(nfrm), _p(bg), lead, B, L, T, _p(spans), _p(hit), _p(score), _s(lib))

    assert call(lde=257, L=257) == ERR_SHAPE and call(T=2049) == ERR_SHAPE and call(lde=7) == ERR_SHAPE
    assert call(B=0) == ERR_SHAPE and call(lead=-1) == ERR_SHAPE and call(lead=8) == ERR_SHAPE
    for name in ("emit", "ntok", "nfrm", "bg", "spans", "hit", "score"):
        assert call(**{name: None}) == ERR_ARG, name
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
    e = torch.zeros(2, 5, 4, device=DEV)
    two, bg = torch.ones(2, dtype=I32, device=DEV), torch.zeros(2, device=DEV)
    with pytest.raises(ValueError, match="lead"):
        ops.align_spot(e, two, two, bg, 4)
    with pytest.raises(ValueError, match="int32"):
        ops.align_spot(e, two.long(), two, bg)
    with pytest.raises(ValueError, match="one entry per pair"):
        ops.align_spot(e, two, two, bg[:1])
