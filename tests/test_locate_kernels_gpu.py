"""Kernel contract of ste_align_matrix_seg_fwd (csrc/align_infer.hip): the segmented form of
ste_align_matrix_fwd, (query block, segment) pairs over runs of rows of one K|V buffer.

Everything here is EXACT (torch.equal / array_equal), no tolerance: a pair with F frames must give
the bits of ste_align_matrix_fwd(B = 1, T = F, no mask) on copies of its rows, whatever else is in
the launch.  The segment lengths 1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025 and 2048 are the edges of the
VU = 8 value rows in flight, the 64-lane softmax stride and the NT = 1024 threads of a block;
(L, P, nh) = (1, 64, 8), (9, 128, 4), (12, 768, 4), (70, 256, 1) are the edges of the QB = 8 query groups
and d = 8, 32, 192, 256.  The segments lie out of order in one buffer between NaN rows, every leading
dimension carries padding, and every output is filled with NaN beforehand, so a read outside a
segment or a write outside a pair's rows shows.

The planted-path test is independent of the reference arithmetic: one-hot queries and keys whose
off-path weights underflow to 0, so kernel -> ste_align_decode must return the planted spans.
"""
import functools

import numpy as np
import pytest
import torch

from kref_align import planted, viterbi_batch_ref
from test_w2v2_kernels_gpu import BF16, DEV, ERR_SHAPE, F32, _p, _s

pytestmark = pytest.mark.gpu
I32, I64 = torch.int32, torch.int64
ERR_ARG = 1001
NAN = float("nan")
FS = (1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2048)
GAP = 3                                   # NaN rows before, between and after the segments
SHAPES = [(1, 64, 8), (9, 128, 4), (12, 768, 4), (70, 256, 1)]
U = 3                                     # query blocks


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops
    return ops


def _layout(lengths, order, P, pad, gen):
    """Segments of the given lengths laid in `order` into one NaN-filled bf16 buffer [rows, 2P + pad],
    GAP NaN rows around each -> (buffer on the device, its [:, :2P] view, seg_row list, the segments'
    own rows as contiguous device tensors)."""
    rows = GAP + sum(n + GAP for n in lengths)
    buf = torch.full((rows, 2 * P + pad), NAN, dtype=BF16)
    seg_row, own = [0] * len(lengths), [None] * len(lengths)
    at = GAP
    for g in order:
        n = lengths[g]
        own[g] = torch.randn(n, 2 * P, generator=gen).to(BF16)
        buf[at:at + n, :2 * P] = own[g]
        seg_row[g] = at
        at += n + GAP
    buf = buf.to(DEV)
    return buf, buf[:, :2 * P], seg_row, [o.to(DEV) for o in own]


def _alone(ops, qu, rows, L, nh):
    """ste_align_matrix_fwd(B = 1, T = F, no mask) on contiguous copies -> (matrix [L, F], emit [F, L], out [L, P])."""
    F, P = rows.shape[0], rows.shape[1] // 2
    m = torch.empty(1, L, F, device=DEV)
    e = torch.empty(1, F, L, device=DEV)
    o = torch.empty(L, P, device=DEV, dtype=BF16)
    ops.align_matrix_fwd(qu.contiguous(), rows.contiguous(), None, 1, L, F, nh, matrix=m, emit=e, out=o)
    return m[0], e[0], o


@functools.lru_cache(maxsize=None)
def _big(L, P, nh):
    """The one big launch of a shape and everything the tests compare it with, computed once."""
    from speech_transcript_embeddings_amd import ops
    gen = torch.Generator().manual_seed(1000 * L + P + nh)
    G = len(FS)
    order = [int(i) for i in torch.randperm(G, generator=gen)]
    buf, kv, seg_row, own = _layout(FS, order, P, 8, gen)
    ldq = P + 8
    qbuf = torch.full((U * L, ldq), NAN, dtype=BF16)
    qbuf[:, :P] = torch.randn(U * L, P, generator=gen).to(BF16)
    qbuf = qbuf.to(DEV)
    # two pairs per segment with different queries, one empty pair, in a shuffled order
    pairs = [(g % U, g) for g in range(G)] + [((g + 1) % U, g) for g in range(G)] + [(-1, 0), (0, -1)]
    pairs = [pairs[int(i)] for i in torch.randperm(len(pairs), generator=gen)]
    R, Tmax = len(pairs), max(FS)
    qblk = torch.tensor([p[0] for p in pairs], dtype=I32, device=DEV)
    pseg = torch.tensor([p[1] for p in pairs], dtype=I32, device=DEV)
    srow = torch.tensor(seg_row, dtype=I64, device=DEV)
    slen = torch.tensor(FS, dtype=I32, device=DEV)
    lde, ldo = L + 5, P + 8
    matrix = torch.full((R, L, Tmax), NAN, device=DEV)
    emit = torch.full((R, Tmax, lde), NAN, device=DEV)
    out = torch.full((R * L, ldo), NAN, device=DEV, dtype=BF16)
    ops.align_matrix_seg_fwd(qbuf[:, :P], qblk, pseg, kv, srow, slen, L, Tmax, nh, matrix=matrix,
                             emit=emit[:, :, :L], out=out[:, :P])
    torch.cuda.synchronize()
    return dict(pairs=pairs, q=qbuf, own=own, seg_row=seg_row, matrix=matrix, emit=emit, out=out, buf=buf,
                qblk=qblk, pseg=pseg, srow=srow, slen=slen, kv=kv)


@pytest.mark.parametrize("L,P,nh", SHAPES)
def test_equal_to_the_dense_kernel(ops, L, P, nh):
    b = _big(L, P, nh)
    q = b["q"][:, :P]
    for r, (u, g) in enumerate(b["pairs"]):
        o = b["out"][r * L:(r + 1) * L]
        assert bool(o[:, P:].isnan().all()), (r, "out padding written")
        if u < 0 or g < 0:                                   # an empty pair: zero out rows, sentinels intact
            assert float(o[:, :P].float().abs().max()) == 0.0
            assert bool(b["matrix"][r].isnan().all()) and bool(b["emit"][r].isnan().all())
            continue
        F = FS[g]
        m, e, oo = _alone(ops, q[u * L:(u + 1) * L], b["own"][g], L, nh)
        what = f"pair {r}: query {u}, segment {g} (F = {F})"
        assert torch.equal(b["matrix"][r, :, :F], m), what
        assert torch.equal(b["emit"][r, :F, :L], e), what
        assert torch.equal(o[:, :P], oo), what
        assert bool(b["matrix"][r, :, F:].isnan().all()), what + ": matrix frames >= F written"
        assert bool(b["emit"][r, F:].isnan().all()), what + ": emit frames >= F written"
        assert bool(b["emit"][r, :, L:].isnan().all()), what + ": emit columns >= L written"
    assert bool(b["buf"][:GAP].isnan().all())                # (the operands are read-only)


@pytest.mark.parametrize("L,P,nh", SHAPES)
def test_equal_to_the_masked_dense_kernel_at_tmax(ops, L, P, nh):
    """One dense call at T = Tmax with prefix masks over finite random padding rows: a masked key's
    weight is exactly 0, so rows [:F] carry the same bits."""
    b = _big(L, P, nh)
    G, Tmax = len(FS), max(FS)
    gen = torch.Generator().manual_seed(5)
    kvd = torch.randn(G, Tmax, 2 * P, generator=gen).to(BF16).to(DEV)
    km = torch.zeros(G, Tmax, dtype=I32, device=DEV)
    qd = torch.empty(G * L, P, dtype=BF16, device=DEV)
    for g in range(G):
        kvd[g, :FS[g]] = b["own"][g]
        km[g, :FS[g]] = 1
        qd[g * L:(g + 1) * L] = b["q"][(g % U) * L:(g % U + 1) * L, :P]
    m = torch.empty(G, L, Tmax, device=DEV)
    e = torch.empty(G, Tmax, L, device=DEV)
    o = torch.empty(G * L, P, device=DEV, dtype=BF16)
    ops.align_matrix_fwd(qd, kvd.view(G * Tmax, 2 * P), km.view(-1), G, L, Tmax, nh, matrix=m, emit=e, out=o)
    for g in range(G):
        r = b["pairs"].index((g % U, g))
        F = FS[g]
        assert torch.equal(b["matrix"][r, :, :F], m[g, :, :F]), g
        assert torch.equal(b["emit"][r, :F, :L], e[g, :F]), g
        assert torch.equal(b["out"][r * L:(r + 1) * L, :P], o[g * L:(g + 1) * L]), g
        assert float(m[g, :, F:].abs().max() if F < Tmax else 0.0) == 0.0


def test_a_pair_does_not_depend_on_its_launch(ops):
    """The same pair alone (R = G = 1, Tmax = F, its segment at row 0 of another buffer), at another
    position with other neighbours, and with each output requested on its own."""
    L, P, nh = 9, 128, 4
    b = _big(L, P, nh)
    for g in (FS.index(65), FS.index(1025)):
        u, F = g % U, FS[g]
        r = b["pairs"].index((u, g))
        want = (b["matrix"][r, :, :F], b["emit"][r, :F, :L], b["out"][r * L:(r + 1) * L, :P])
        kv1 = b["own"][g].clone()                            # another buffer: contiguous, ldkv = 2P, no gap
        q1 = b["q"][:, :P].contiguous()
        one = lambda v, dt=I32: torch.tensor([v], dtype=dt, device=DEV)     # noqa: E731
        for which in ("all", "matrix", "emit", "out"):
            m = torch.full((1, L, F), NAN, device=DEV) if which in ("all", "matrix") else None
            e = torch.full((1, F, L), NAN, device=DEV) if which in ("all", "emit") else None
            o = torch.full((L, P), NAN, device=DEV, dtype=BF16) if which in ("all", "out") else None
            ops.align_matrix_seg_fwd(q1, one(u), one(0), kv1, one(0, I64), one(F), L, F, nh, matrix=m, emit=e, out=o)
            for got, ref in zip((m, e, o), want):
                if got is not None:
                    assert torch.equal(got.view(ref.shape), ref), (g, which)
        # last of five pairs, behind an empty pair and pairs of other segments, Tmax between F and 2048
        Tmax = F + 11
        qb = torch.tensor([2, -1, 0, 1, u], dtype=I32, device=DEV)
        ps = torch.tensor([1, g, 2, 0, g], dtype=I32, device=DEV)
        m = torch.full((5, L, Tmax), NAN, device=DEV)
        e = torch.full((5, Tmax, L), NAN, device=DEV)
        o = torch.full((5 * L, P), NAN, device=DEV, dtype=BF16)
        ops.align_matrix_seg_fwd(b["q"][:, :P], qb, ps, b["kv"], b["srow"], b["slen"], L, Tmax, nh, matrix=m, emit=e,
                                 out=o)
        assert torch.equal(m[4, :, :F], want[0]) and torch.equal(e[4, :F], want[1]) and torch.equal(o[4 * L:], want[2])
        assert bool(m[4, :, F:].isnan().all()) and bool(e[4, F:].isnan().all())


def test_empty_pairs(ops):
    """qblk = -1, pseg = -1, pseg >= G, seg_len = 0 and seg_len > Tmax: zero out rows, sentinels intact,
    no error; the live pair beside them is unaffected."""
    L, P, nh, Tmax = 9, 64, 4, 16
    gen = torch.Generator().manual_seed(2)
    lengths = (5, 0, 40, 16)
    buf, kv, seg_row, own = _layout(lengths, [2, 0, 3, 1], P, 8, gen)
    q = torch.randn(2 * L, P, generator=gen).to(BF16).to(DEV)
    pairs = [(-1, 0), (0, -1), (1, 1), (0, 2), (1, 4), (1, 0), (0, 3)]     # the last two are live
    qb = torch.tensor([p[0] for p in pairs], dtype=I32, device=DEV)
    ps = torch.tensor([p[1] for p in pairs], dtype=I32, device=DEV)
    R = len(pairs)
    m = torch.full((R, L, Tmax), NAN, device=DEV)
    e = torch.full((R, Tmax, L), NAN, device=DEV)
    o = torch.full((R * L, P), NAN, device=DEV, dtype=BF16)
    ops.align_matrix_seg_fwd(q, qb, ps, kv, torch.tensor(seg_row, dtype=I64, device=DEV),
                             torch.tensor(lengths, dtype=I32, device=DEV), L, Tmax, nh, matrix=m, emit=e, out=o)
    for r in range(5):
        assert float(o[r * L:(r + 1) * L].float().abs().max()) == 0.0, r
        assert bool(m[r].isnan().all()) and bool(e[r].isnan().all()), r
    for r, (u, g) in ((5, (1, 0)), (6, (0, 3))):
        F = lengths[g]
        wm, we, wo = _alone(ops, q[u * L:(u + 1) * L], own[g], L, nh)
        assert torch.equal(m[r, :, :F], wm) and torch.equal(e[r, :F], we) and torch.equal(o[r * L:(r + 1) * L], wo)
        assert bool(m[r, :, F:].isnan().all()) and bool(e[r, F:].isnan().all())
    # without out nothing at all is written for an empty pair
    m2 = torch.full((R, L, Tmax), NAN, device=DEV)
    ops.align_matrix_seg_fwd(q, qb, ps, kv, torch.tensor(seg_row, dtype=I64, device=DEV),
                             torch.tensor(lengths, dtype=I32, device=DEV), L, Tmax, nh, matrix=m2)
    assert bool(m2[:5].isnan().all()) and torch.equal(m2[5, :, :5], m[5, :, :5])


def test_rejected_before_a_launch(lib):
    t = torch.zeros(1 << 16, device=DEV)
    z = torch.zeros(64, dtype=I64, device=DEV)               # qblk / pseg / seg_row / seg_len: all zeros
    f = lib.fn("ste_align_matrix_seg_fwd")

    def call(R=1, G=1, L=3, Tmax=16, P=64, nh=8, matrix=True, emit=True, out=True, ldq=None, ldkv=None):
        return f(_p(t), ldq or P, _p(z), _p(z), _p(t), ldkv or 2 * P, _p(z), _p(z), R, G, L, Tmax, P, nh,
                 _p(t) if matrix else None, _p(t) if emit else None, L, _p(t) if out else None, P, _s(lib))

    assert call(Tmax=2049) == ERR_SHAPE
    assert call(P=1040, nh=4) == ERR_SHAPE                   # d = 260
    assert call(P=80, nh=8) == ERR_SHAPE                     # d = 10, not a multiple of 8
    assert call(R=0) == ERR_SHAPE and call(G=0) == ERR_SHAPE
    assert call(matrix=False, emit=False, out=False) == ERR_ARG
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_more_pairs_than_a_grid_dimension(ops):
    """R = 65535 + 4 pairs of one-frame segments: the entry point splits the launch.  One key gives
    probability 1 in every head, so matrix is exactly 1 and out is the segment's value row."""
    L, P, nh, R = 1, 64, 8, 65535 + 4
    gen = torch.Generator().manual_seed(4)
    kv = torch.randn(2, 2 * P, generator=gen).to(BF16).to(DEV)
    q = torch.randn(L, P, generator=gen).to(BF16).to(DEV)
    ps = (torch.arange(R, device=DEV) % 2).to(I32)
    m = torch.full((R, L, 1), NAN, device=DEV)
    o = torch.full((R * L, P), NAN, device=DEV, dtype=BF16)
    ops.align_matrix_seg_fwd(q, torch.zeros(R, dtype=I32, device=DEV), ps, kv, torch.tensor([0, 1], dtype=I64, device=DEV),
                             torch.tensor([1, 1], dtype=I32, device=DEV), L, 1, nh, matrix=m, out=o)
    assert bool((m == 1.0).all())
    assert torch.equal(o, kv[:, P:].index_select(0, ps.long()))


def test_planted_paths_come_back(ops):
    """nh = 1, q_l = s·e_l, k_t = s·e_token(t) with s = 32: a planted cell scores s²/√d = 128 and any
    other 0, so an off-path weight is at most e^-128 < FLT_MIN and flushes to 0 while token l's frames
    share weight 1 equally.  Every other monotone path crosses a cell of log FLT_MIN, so the decode of
    the kernel's emissions is the planted segmentation, whatever the segment's length and place."""
    L, P, nh, s = 12, 64, 1, 32.0
    ntoks = (12, 7)
    frames = ((12, 37, 300), (7, 64, 129))
    lengths, spans_of, pairs = [], [], []
    for u, n in enumerate(ntoks):
        for F in frames[u]:
            pairs.append((u, len(lengths)))
            lengths.append(F)
            spans_of.append(planted(L, F, n, F, seed=10 * F + n)[1])
    gen = torch.Generator().manual_seed(6)
    order = [3, 0, 5, 2, 4, 1]
    rows = GAP + sum(n + GAP for n in lengths)
    buf = torch.full((rows, 2 * P + 8), NAN, dtype=BF16)
    seg_row = [0] * len(lengths)
    at = GAP
    for g in order:
        F = lengths[g]
        k = torch.zeros(F, P)
        for tok, (a, b) in enumerate(spans_of[g]):
            k[a:b, tok] = s
        buf[at:at + F, :P] = k.to(BF16)
        buf[at:at + F, P:2 * P] = torch.randn(F, P, generator=gen).to(BF16)
        seg_row[g] = at
        at += F + GAP
    buf = buf.to(DEV)
    q = torch.zeros(len(ntoks) * L, P)
    for u, n in enumerate(ntoks):
        for l in range(n):
            q[u * L + l, l] = s
    q = q.to(BF16).to(DEV)
    R, Tmax = len(pairs), max(lengths)
    qb = torch.tensor([p[0] for p in pairs], dtype=I32, device=DEV)
    ps = torch.tensor([p[1] for p in pairs], dtype=I32, device=DEV)
    emit = torch.full((R, Tmax, L), NAN, device=DEV)
    ops.align_matrix_seg_fwd(q, qb, ps, buf[:, :2 * P], torch.tensor(seg_row, dtype=I64, device=DEV),
                             torch.tensor(lengths, dtype=I32, device=DEV), L, Tmax, nh, emit=emit)
    ntok = torch.tensor([ntoks[u] for u, _ in pairs], dtype=I32, device=DEV)
    nfrm = torch.tensor([lengths[g] for _, g in pairs], dtype=I32, device=DEV)
    spans, score = ops.align_decode(emit, ntok, nfrm)
    spans, score = spans.cpu().numpy(), score.cpu().numpy()
    for r, (u, g) in enumerate(pairs):
        n = ntoks[u]
        assert np.array_equal(spans[r, :n], spans_of[g]), (r, spans[r, :n], spans_of[g])
        assert (spans[r, n:] == -1).all()
    rs, rsc = viterbi_batch_ref(emit.cpu().numpy(), ntok.tolist(), nfrm.tolist(), L)
    assert np.array_equal(spans, rs)
    assert np.array_equal(score.view(np.int32), rsc.view(np.int32))
