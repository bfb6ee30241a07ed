"""Kernel contract of ste_align_matrix_seg_mx8_fwd (csrc/align_infer.hip): the segmented
alignment matrix on rows stored as MX-fp8 (e4m3 bytes + one E8M0 scale byte per 32 columns).

Everything here is EXACT, no tolerance: for every pair the kernel must give the bits of
ste_align_matrix_seg_fwd on ops.mx8_dequant of the same bytes laid out at the same rows, because the two
kernels share every instruction after the load.  The segment lengths 1, 7, 8, 9, 63, 64, 65, 1023, 1024,
1025 and 2048 are the edges of the value rows in flight (8 in the bf16 kernel, 16 here), the 64-lane
softmax stride and the NT = 1024 threads of a block; (L, P, nh) = (1, 64, 8), (9, 128, 4), (12, 192, 8),
(12, 768, 4), (70, 256, 1) give d = 8 (four heads per scale block), 32, 24 (blocks straddle heads),
192 and 256.  The segments lie out of order between poison rows (e4m3 NaN bytes under scale byte 255),
every leading dimension carries padding and every output is filled with NaN beforehand, so a read
outside a segment or a write outside a pair's rows shows.

The rounding corner of mx8_dequant1 (every finite e4m3 byte under the scale bytes whose products land in
bf16's subnormal range, where the conversion rounds) is compared bit for bit too, and the dequantiser the
reference rows come from is itself held against tests/kref_mx8.py's numpy reading of the raw bytes.

The planted-path test is independent of the bf16 kernel: one-hot rows of a power of two are exact in
e4m3, so kernel -> ste_align_decode must return the planted spans.
"""
import functools

import numpy as np
import pytest
import torch

import kref_mx8
from kref_align import planted, viterbi_batch_ref
from test_w2v2_kernels_gpu import BF16, DEV, ERR_SHAPE, _p, _s

pytestmark = pytest.mark.gpu
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
ERR_ARG = 1001
NAN = float("nan")
FS = (1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2048)
GAP = 3                                   # poison rows before, between and after the segments
SHAPES = [(1, 64, 8), (9, 128, 4), (12, 192, 8), (12, 768, 4), (70, 256, 1)]
U = 3                                     # query blocks
PAD_KV, PAD_SC = 8, 3                     # padding columns of the byte and of the scale buffer


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops
    return ops


def _bits(t):
    """The raw bits of an fp32 / bf16 tensor: equality that no NaN sentinel escapes."""
    return t.view(I32 if t.dtype == torch.float32 else torch.int16)


def _layout(own_q, own_s, order, P):
    """Segments (bytes [n, 2P], scales [n, 2P/32]) laid in `order` between GAP poison rows -> (byte
    buffer [rows, 2P + PAD_KV] of 0x7f, scale buffer [rows, 2P/32 + PAD_SC] of 255, the NaN-filled bf16
    buffer [rows, 2P + 8] holding ops.mx8_dequant of the segments at the same rows, seg_row)."""
    from speech_transcript_embeddings_amd import ops
    lengths = [q.shape[0] for q in own_q]
    rows = GAP + sum(n + GAP for n in lengths)
    kvb = torch.full((rows, 2 * P + PAD_KV), 0x7F, dtype=U8, device=DEV)
    scb = torch.full((rows, 2 * P // 32 + PAD_SC), 255, dtype=U8, device=DEV)
    deq = torch.full((rows, 2 * P + 8), NAN, dtype=BF16, device=DEV)
    seg_row = [0] * len(lengths)
    at = GAP
    for g in order:
        n = lengths[g]
        kvb[at:at + n, :2 * P] = own_q[g]
        scb[at:at + n, :2 * P // 32] = own_s[g]
        if n:
            deq[at:at + n, :2 * P] = ops.mx8_dequant(own_q[g], own_s[g])
        seg_row[g] = at
        at += n + GAP
    return kvb, scb, deq, seg_row


def _quantised(lengths, P, gen):
    """ops.mx8_quant of rows drawn in [-0.9, 0.9], one (bytes, scales) per segment."""
    from speech_transcript_embeddings_amd import ops
    own_q, own_s = [], []
    for n in lengths:
        rows = ((torch.rand(max(n, 1), 2 * P, generator=gen) * 1.8 - 0.9).to(BF16).to(DEV))[:n].contiguous()
        if n:
            q, s = ops.mx8_quant(rows)
        else:
            q, s = torch.empty(0, 2 * P, dtype=U8, device=DEV), torch.empty(0, 2 * P // 32, dtype=U8, device=DEV)
        own_q.append(q)
        own_s.append(s)
    return own_q, own_s


def _outputs(R, L, Tmax, P):
    lde, ldo = L + 5, P + 8
    return (torch.full((R, L, Tmax), NAN, device=DEV), torch.full((R, Tmax, lde), NAN, device=DEV),
            torch.full((R * L, ldo), NAN, device=DEV, dtype=BF16))


@functools.lru_cache(maxsize=None)
def _big(L, P, nh):
    """The one big launch of a shape on the bytes and the bf16 kernel's on the dequantised rows, once."""
    from speech_transcript_embeddings_amd import ops
    gen = torch.Generator().manual_seed(2100 * L + P + nh)
    G = len(FS)
    order = [int(i) for i in torch.randperm(G, generator=gen)]
    own_q, own_s = _quantised(FS, P, gen)
    kvb, scb, deq, seg_row = _layout(own_q, own_s, order, P)
    ldq = P + 8
    qbuf = torch.full((U * L, ldq), NAN, dtype=BF16)
    qbuf[:, :P] = torch.randn(U * L, P, generator=gen).to(BF16)
    qbuf = qbuf.to(DEV)
    # two pairs per segment with different query blocks (so a qblk repeats), two empty pairs, shuffled
    pairs = [(g % U, g) for g in range(G)] + [((g + 1) % U, g) for g in range(G)] + [(-1, 0), (0, -1)]
    pairs = [pairs[int(i)] for i in torch.randperm(len(pairs), generator=gen)]
    R, Tmax = len(pairs), max(FS)
    qblk = torch.tensor([p[0] for p in pairs], dtype=I32, device=DEV)
    pseg = torch.tensor([p[1] for p in pairs], dtype=I32, device=DEV)
    srow = torch.tensor(seg_row, dtype=I64, device=DEV)
    slen = torch.tensor(FS, dtype=I32, device=DEV)
    kv, sc = kvb[:, :2 * P], scb[:, :2 * P // 32]
    matrix, emit, out = _outputs(R, L, Tmax, P)
    ops.align_matrix_seg_fwd(qbuf[:, :P], qblk, pseg, kv, srow, slen, L, Tmax, nh, scales=sc, matrix=matrix,
                             emit=emit[:, :, :L], out=out[:, :P])
    wm, we, wo = _outputs(R, L, Tmax, P)
    ops.align_matrix_seg_fwd(qbuf[:, :P], qblk, pseg, deq[:, :2 * P], srow, slen, L, Tmax, nh, matrix=wm,
                             emit=we[:, :, :L], out=wo[:, :P])
    torch.cuda.synchronize()
    return dict(pairs=pairs, q=qbuf, own_q=own_q, own_s=own_s, seg_row=seg_row, matrix=matrix, emit=emit, out=out,
                want=(wm, we, wo), kvb=kvb, scb=scb, kv=kv, sc=sc, qblk=qblk, pseg=pseg, srow=srow, slen=slen)


@pytest.mark.parametrize("L,P,nh", SHAPES)
def test_equal_to_the_bf16_kernel_on_the_dequantised_rows(L, P, nh):
    b = _big(L, P, nh)
    wm, we, wo = b["want"]
    for r, (u, g) in enumerate(b["pairs"]):
        o = b["out"][r * L:(r + 1) * L]
        assert bool(o[:, P:].isnan().all()), (r, "out padding written")
        if u < 0 or g < 0:                                   # an empty pair: zero out rows, sentinels intact
            assert float(o[:, :P].float().abs().max()) == 0.0
            assert bool(b["matrix"][r].isnan().all()) and bool(b["emit"][r].isnan().all())
            continue
        F = FS[g]
        what = f"pair {r}: query {u}, segment {g} (F = {F})"
        assert not bool(wm[r, :, :F].isnan().any()) and not bool(wo[r * L:(r + 1) * L, :P].isnan().any()), what
        assert torch.equal(b["matrix"][r, :, :F], wm[r, :, :F]), what
        assert torch.equal(b["emit"][r, :F, :L], we[r, :F, :L]), what
        assert torch.equal(o[:, :P], wo[r * L:(r + 1) * L, :P]), what
        assert bool(b["matrix"][r, :, F:].isnan().all()), what + ": matrix frames >= F written"
        assert bool(b["emit"][r, F:].isnan().all()), what + ": emit frames >= F written"
        assert bool(b["emit"][r, :, L:].isnan().all()), what + ": emit columns >= L written"
    # and the whole buffers, sentinels included, bit for bit
    for got, want in zip((b["matrix"], b["emit"], b["out"]), b["want"]):
        assert torch.equal(_bits(got), _bits(want))
    assert bool((b["kvb"][:GAP] == 0x7F).all()) and bool((b["scb"][:GAP] == 255).all())     # read-only operands


def test_the_rounding_corner_of_the_value_element(ops):
    """Every finite e4m3 byte in the V columns under the scale bytes 0, 1, 2, 5, 8, 9, 10 (products in
    bf16's subnormal range, where bf16(fp32) rounds), 64, 127 and 254, one per 32-block; 24 rows, so that
    both the 16 rows in flight and the remainder loop see every byte."""
    L, P, nh, F = 5, 320, 2, 24
    scales_v = (0, 1, 2, 5, 8, 9, 10, 64, 127, 254)
    assert len(scales_v) == P // 32
    gen = torch.Generator().manual_seed(21)
    (q8,), (s8,) = _quantised((F,), P, gen)
    q8, s8 = q8.clone(), s8.clone()
    r = torch.arange(F).view(F, 1, 1)
    blk = torch.arange(P // 32).view(1, P // 32, 1)
    j = torch.arange(32).view(1, 1, 32)
    v = ((r * 32 + j + 37 * blk) % 256).to(U8)
    v[(v & 0x7F) == 0x7F] = 0                                   # the two NaN bytes
    vals = v.view(F, P)
    for k in range(P // 32):                                   # every finite byte, in the first 8 and the last 8 rows
        for rows in (slice(0, 8), slice(16, 24)):
            assert len(set(vals[rows, 32 * k:32 * k + 32].reshape(-1).tolist())) == 254
    q8[:, P:] = vals.to(DEV)
    s8[:, P // 32:] = torch.tensor(scales_v, dtype=U8, device=DEV)
    # what the bytes mean: the library's dequantiser against the numpy reading of the raw bytes
    deq = ops.mx8_dequant(q8, s8)
    assert kref_mx8.same_bf16(deq.view(torch.int16).cpu().numpy().view(np.uint16),
                              kref_mx8.mx8_dequant_bits(q8.cpu().numpy(), s8.cpu().numpy()))
    qu = (torch.randn(L, P, generator=gen) * 0.5).to(BF16).to(DEV)
    one = lambda x, dt=I32: torch.tensor([x], dtype=dt, device=DEV)     # noqa: E731
    got = torch.full((L, P), NAN, device=DEV, dtype=BF16)
    want = torch.full((L, P), NAN, device=DEV, dtype=BF16)
    gm, wm = torch.full((1, L, F), NAN, device=DEV), torch.full((1, L, F), NAN, device=DEV)
    ops.align_matrix_seg_fwd(qu, one(0), one(0), q8, one(0, I64), one(F), L, F, nh, scales=s8, matrix=gm, out=got)
    ops.align_matrix_seg_fwd(qu, one(0), one(0), deq, one(0, I64), one(F), L, F, nh, matrix=wm, out=want)
    assert torch.equal(gm, wm) and float(gm.min()) > 0.0       # every frame carries weight in the sums
    assert torch.equal(_bits(got), _bits(want))                # (E = 254 overflows to inf: bits, not values)
    low = got[:, :7 * 32].float()                              # the subnormal blocks: tiny, and not all zero
    assert bool(low.isfinite().all()) and float(low.abs().max()) > 0.0
    mid = got[:, 7 * 32:9 * 32].float()
    assert bool(mid.isfinite().all()) and float(mid.abs().max()) > 0.0


def test_a_pair_does_not_depend_on_its_launch(ops):
    """The same pair alone (R = G = 1, Tmax = F, its segment at row 0 of another buffer), with each output
    requested on its own, and as the last of five pairs behind an empty one with another Tmax."""
    L, P, nh = 9, 128, 4
    b = _big(L, P, nh)
    for g in (FS.index(65), FS.index(1025)):
        u, F = g % U, FS[g]
        r = b["pairs"].index((u, g))
        want = (b["matrix"][r, :, :F], b["emit"][r, :F, :L], b["out"][r * L:(r + 1) * L, :P])
        kv1, sc1 = b["own_q"][g].clone(), b["own_s"][g].clone()  # another buffer: contiguous, no padding, no gap
        q1 = b["q"][:, :P].contiguous()
        one = lambda x, dt=I32: torch.tensor([x], dtype=dt, device=DEV)     # noqa: E731
        for which in ("all", "matrix", "emit", "out"):
            m = torch.full((1, L, F), NAN, device=DEV) if which in ("all", "matrix") else None
            e = torch.full((1, F, L), NAN, device=DEV) if which in ("all", "emit") else None
            o = torch.full((L, P), NAN, device=DEV, dtype=BF16) if which in ("all", "out") else None
            ops.align_matrix_seg_fwd(q1, one(u), one(0), kv1, one(0, I64), one(F), L, F, nh, scales=sc1, matrix=m,
                                     emit=e, out=o)
            for got, ref in zip((m, e, o), want):
                if got is not None:
                    assert torch.equal(got.view(ref.shape), ref), (g, which)
        Tmax = F + 11
        qb = torch.tensor([2, -1, 0, 1, u], dtype=I32, device=DEV)
        ps = torch.tensor([1, g, 2, 0, g], dtype=I32, device=DEV)
        m = torch.full((5, L, Tmax), NAN, device=DEV)
        e = torch.full((5, Tmax, L), NAN, device=DEV)
        o = torch.full((5 * L, P), NAN, device=DEV, dtype=BF16)
        ops.align_matrix_seg_fwd(b["q"][:, :P], qb, ps, b["kv"], b["srow"], b["slen"], L, Tmax, nh, scales=b["sc"],
                                 matrix=m, emit=e, out=o)
        assert torch.equal(m[4, :, :F], want[0]) and torch.equal(e[4, :F], want[1]) and torch.equal(o[4 * L:], want[2])
        assert bool(m[4, :, F:].isnan().all()) and bool(e[4, F:].isnan().all())
        assert bool(m[1].isnan().all()) and float(o[L:2 * L].float().abs().max()) == 0.0


def test_empty_pairs(ops):
    """qblk = -1, pseg = -1, pseg >= G, seg_len = 0 and seg_len > Tmax: zero out rows, sentinels intact,
    no error; the live pairs beside them are unaffected."""
    L, P, nh, Tmax = 9, 64, 4, 16
    gen = torch.Generator().manual_seed(2)
    lengths = (5, 0, 40, 16)
    own_q, own_s = _quantised(lengths, P, gen)
    kvb, scb, deq, seg_row = _layout(own_q, own_s, [2, 0, 3, 1], P)
    q = torch.randn(2 * L, P, generator=gen).to(BF16).to(DEV)
    pairs = [(-1, 0), (0, -1), (1, 1), (0, 2), (1, 4), (1, 0), (0, 3)]     # the last two are live
    qb = torch.tensor([p[0] for p in pairs], dtype=I32, device=DEV)
    ps = torch.tensor([p[1] for p in pairs], dtype=I32, device=DEV)
    R = len(pairs)
    srow = torch.tensor(seg_row, dtype=I64, device=DEV)
    slen = torch.tensor(lengths, dtype=I32, device=DEV)

    def outs():
        return (torch.full((R, L, Tmax), NAN, device=DEV), torch.full((R, Tmax, L), NAN, device=DEV),
                torch.full((R * L, P), NAN, device=DEV, dtype=BF16))

    m, e, o = outs()
    ops.align_matrix_seg_fwd(q, qb, ps, kvb[:, :2 * P], srow, slen, L, Tmax, nh, scales=scb[:, :2 * P // 32], matrix=m,
                             emit=e, out=o)
    wm, we, wo = outs()
    ops.align_matrix_seg_fwd(q, qb, ps, deq[:, :2 * P], srow, slen, L, Tmax, nh, matrix=wm, emit=we, out=wo)
    for r in range(5):
        assert float(o[r * L:(r + 1) * L].float().abs().max()) == 0.0, r
        assert bool(m[r].isnan().all()) and bool(e[r].isnan().all()), r
    for r, F in ((5, 5), (6, 16)):
        assert not bool(m[r, :, :F].isnan().any()) and not bool(o[r * L:(r + 1) * L].isnan().any())
        assert bool(m[r, :, F:].isnan().all()) and bool(e[r, F:].isnan().all())
    for got, want in ((m, wm), (e, we), (o, wo)):
        assert torch.equal(_bits(got), _bits(want))
    # without out nothing at all is written for an empty pair
    m2 = torch.full((R, L, Tmax), NAN, device=DEV)
    ops.align_matrix_seg_fwd(q, qb, ps, kvb[:, :2 * P], srow, slen, L, Tmax, nh, scales=scb[:, :2 * P // 32], matrix=m2)
    assert bool(m2[:5].isnan().all()) and torch.equal(m2[5, :, :5], m[5, :, :5])


def test_rejected_before_a_launch(lib):
    t = torch.zeros(1 << 16, device=DEV)
    z = torch.zeros(64, dtype=I64, device=DEV)               # qblk / pseg / seg_row / seg_len: all zeros
    f = lib.fn("ste_align_matrix_seg_mx8_fwd")

    def call(R=1, G=1, L=3, Tmax=16, P=64, nh=8, matrix=True, emit=True, out=True, ldq=None, ldkv=None, lds=None,
             kv_off=0, scales=True):
        return f(_p(t), ldq or P, _p(z), _p(z), _p(t) + kv_off, ldkv or 2 * P, _p(t) if scales else None,
                 lds or 2 * P // 32, _p(z), _p(z), R, G, L, Tmax, P, nh, _p(t) if matrix else None,
                 _p(t) if emit else None, L, _p(t) if out else None, P, _s(lib))

    assert call(P=48, nh=2) == ERR_SHAPE                     # P % 32 != 0
    assert call(ldkv=132) == ERR_SHAPE                       # ldkv % 8 != 0
    assert call(kv_off=4) == ERR_SHAPE                       # kv not 8-byte aligned
    assert call(lds=3) == ERR_SHAPE                          # lds < 2P/32
    assert call(Tmax=2049) == ERR_SHAPE
    assert call(P=1040, nh=4) == ERR_SHAPE                   # d = 260
    assert call(R=0) == ERR_SHAPE and call(G=0) == ERR_SHAPE
    assert call(scales=False) == ERR_ARG
    assert call(matrix=False, emit=False, out=False) == ERR_ARG
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_planted_paths_come_back(ops):
    """kref_align.planted with nh = 1, q_l = s·e_l, k_t = s·e_token(t), s = 32: a planted cell scores
    s²/√d = 128 and any other 0, so an off-path weight flushes to 0 and every other monotone path crosses
    a cell of log FLT_MIN.  0 and 32 are exact in e4m3 under the row's scale (one non-zero magnitude
    per block, a power of two), so quantising the keys loses nothing."""
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
    own_q, own_s = [], []
    for g, F in enumerate(lengths):
        rows = torch.zeros(F, 2 * P)
        for tok, (a, b) in enumerate(spans_of[g]):
            rows[a:b, tok] = s
        rows[:, P:] = torch.rand(F, P, generator=gen) * 1.8 - 0.9
        rows = rows.to(BF16).to(DEV)
        q8, s8 = ops.mx8_quant(rows)
        assert torch.equal(ops.mx8_dequant(q8, s8)[:, :P], rows[:, :P])       # the keys are exact
        own_q.append(q8)
        own_s.append(s8)
    kvb, scb, _, seg_row = _layout(own_q, own_s, [3, 0, 5, 2, 4, 1], P)
    q = torch.zeros(len(ntoks) * L, P)
    for u, n in enumerate(ntoks):
        for l in range(n):
            q[u * L + l, l] = s
    q = q.to(BF16).to(DEV)
    R, Tmax = len(pairs), max(lengths)
    qb = torch.tensor([p[0] for p in pairs], dtype=I32, device=DEV)
    ps = torch.tensor([p[1] for p in pairs], dtype=I32, device=DEV)
    emit = torch.full((R, Tmax, L), NAN, device=DEV)
    ops.align_matrix_seg_fwd(q, qb, ps, kvb[:, :2 * P], torch.tensor(seg_row, dtype=I64, device=DEV),
                             torch.tensor(lengths, dtype=I32, device=DEV), L, Tmax, nh, scales=scb[:, :2 * P // 32],
                             emit=emit)
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
