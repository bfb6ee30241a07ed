"""ste_xattn_seg_mx8_fwd and ste_mx8_dequant (csrc/xattn_mq.hip, csrc/gemm.hip): the segmented
cross attention of §18 over K/V rows stored as OCP e4m3 bytes with one E8M0 scale per 32 columns.

A stored element means bf16(float(e4m3) · 2^(E − 127)) (tests/kref_mx8.py restates it in numpy from the
raw bytes), which is an exact bf16 number, and from the dequantised fragment on the kernel is the bf16
one.  So the checks need no new tolerance:

  * the MX kernel on the bytes has the BITS of ste_xattn_seg_fwd on the dequantised rows;
  * against float64 attention over the numpy-dequantised values the bound is §15's,
    |out − exact| <= 2^-8 · Σ_s p_s·|v_s,c|, with |q|, |k| <= 1;
  * ops.mx8_dequant has the bits of the numpy restatement;
  * a pair's out row does not depend on where it or its segment is.

The layout is §18's one launch per (P, nh): segment lengths around the 32-key tile and the 4-wave
split plus an empty segment, pair counts around the 16-pair tile, empty pairs, the segments out of
order between poison rows (e4m3 NaN bytes 0x7f under the NaN scale 0xff).
"""
import functools

import numpy as np
import pytest
import torch

import kref_mx8
from speech_transcript_embeddings_amd.retrieval import plan_clip_pairs
from test_clip_rerank_kernels_gpu import BOUND, LENS, ORDER, PAIRS, _ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops as o
    return o


def _bits(t):
    """bf16 tensor -> numpy uint16 bits."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _rows(n, P, g):
    """n bf16 K|V rows [n, 2P] in [-0.9, 0.9]: dequantised |k| <= 1, no block near bf16's subnormals."""
    return ((torch.rand(n, 2 * P, generator=g) * 2 - 1) * 0.9).to(BF16)


def _layout(ops, lens, order, gap, P, g, data=None):
    """Segments of the given lengths laid out in `order` with `gap` poison rows before, between and
    after them, quantised row by row -> (bytes uint8 [rows, 2P], scales uint8 [rows, 2P/32], their
    ops.mx8_dequant bf16 [rows, 2P] (NaN in the poison rows), seg_row list, the bf16 rows per segment)."""
    data = data or [_rows(n, P, g) for n in lens]
    seg_row, at = [0] * len(lens), gap
    for s in order:
        seg_row[s] = at
        at += lens[s] + gap
    buf = torch.zeros(at, 2 * P, dtype=BF16)
    live = torch.zeros(at, dtype=torch.bool)
    for s, n in enumerate(lens):
        buf[seg_row[s]:seg_row[s] + n] = data[s]
        live[seg_row[s]:seg_row[s] + n] = True
    qb, sc = ops.mx8_quant(buf.to(DEV))
    qb[~live.to(DEV)] = 0x7F
    sc[~live.to(DEV)] = 0xFF
    deq = ops.mx8_dequant(qb, sc)
    assert torch.isnan(deq[~live.to(DEV)]).all() and torch.isfinite(deq[live.to(DEV)]).all()
    return qb, sc, deq, seg_row, data


def _run(ops, q, buf, seg_row, seg_len, qsel, psel, nh, sc=None, via_op=False):
    """Pairs (row qsel[r] of q, segment psel[r]) in any order, -1 = empty -> out [R, P] in that order.
    sc None: buf is bf16 rows and the kernel ste_xattn_seg_fwd; else buf / sc are bytes and scales."""
    P = q.shape[1]
    plan = plan_clip_pairs(torch.tensor(psel, dtype=torch.int32).view(-1, 1))
    used = plan["unique"].long()
    qs = torch.tensor(qsel, dtype=torch.int32)
    qrow = torch.where(plan["qrow"] >= 0, qs[plan["qrow"].clamp(min=0).long()], plan["qrow"])
    d = lambda t: t.contiguous().to(DEV)                                           # noqa: E731
    head = (d(q), d(qrow), d(plan["pseg"]), buf[:, :P], buf[:, P:2 * P])
    if sc is not None:
        head += (sc[:, :P // 32], sc[:, P // 32:2 * P // 32])
    tail = (d(torch.tensor(seg_row, dtype=torch.int64)[used]), d(torch.tensor(seg_len, dtype=torch.int32)[used]),
            d(plan["tile_first"]), d(plan["tile_cnt"]))
    if via_op:
        out = (torch.ops.ste.xattn_seg if sc is None else torch.ops.ste.xattn_seg_mx8)(*head, *tail, nh)
    else:
        out = torch.full((len(psel), P), float("nan"), device=DEV)
        ops.xattn_seg_fwd(*head[:5], *tail, nh, out, **dict(zip(("ks", "vs"), head[5:])))
    torch.cuda.synchronize()
    return out.index_select(0, plan["inverse"].view(-1).to(DEV))


SHAPES = [(64, 8), (128, 4), (192, 8), (768, 8), (1024, 4)]     # dh = 8, 32, 24, 96, 256
LENS0 = LENS + [0]                                               # an empty segment as well
PAIRS0 = PAIRS + [2]
ORDER0 = ORDER + [6]


@functools.lru_cache(maxsize=None)
def _case(P, nh):
    """The one launch of (P, nh), both kernels, computed once for the tests below."""
    from speech_transcript_embeddings_amd import ops
    g = torch.Generator().manual_seed(19 * P + nh)
    U = 9
    q = torch.rand(U, P, generator=g) * 2 - 1
    qb, sc, deq, seg_row, _ = _layout(ops, LENS0, ORDER0, 3, P, g)
    psel = [s for s, n in enumerate(PAIRS0) for _ in range(n)] + [-1] * 5
    perm = torch.randperm(len(psel), generator=g).tolist()
    psel = [psel[i] for i in perm]
    qsel = torch.randint(0, U, (len(psel),), generator=g).tolist()
    qsel[3] = -1                                                   # a pair without a query
    mx = _run(ops, q, qb, seg_row, LENS0, qsel, psel, nh, sc=sc)
    bf = _run(ops, q, deq, seg_row, LENS0, qsel, psel, nh)
    return dict(q=q, qb=qb.cpu().numpy(), sc=sc.cpu().numpy(), deq=deq, seg_row=seg_row, qsel=qsel, psel=psel,
                mx=mx, bf=bf)


@pytest.mark.parametrize("P,nh", SHAPES)
def test_bits_of_the_bf16_kernel_on_the_dequantised_rows(P, nh):
    """All four DHMAX instantiations; at dh = 24 the MX blocks straddle heads, at dh = 8 four heads
    share one scale byte."""
    c = _case(P, nh)
    assert torch.isfinite(c["mx"]).all(), "a stray read of a poison row shows as NaN"
    assert torch.equal(c["mx"], c["bf"])
    live = [r for r, (u, s) in enumerate(zip(c["qsel"], c["psel"])) if u >= 0 and s >= 0 and LENS0[s] > 0]
    assert len(live) >= sum(PAIRS) - 1
    assert (c["mx"][live].abs().sum(1) > 0).all()


@pytest.mark.parametrize("P,nh", SHAPES)
def test_bound_against_float64_over_the_numpy_dequantised_bytes(P, nh):
    c = _case(P, nh)
    out = c["mx"].cpu().double()
    rows = torch.from_numpy(kref_mx8.mx8_dequant(c["qb"], c["sc"]))          # float64 [rows, 2P], NaN in the gaps
    refs, worst = {}, 0.0
    for r, (u, s) in enumerate(zip(c["qsel"], c["psel"])):
        if u < 0 or s < 0 or LENS0[s] == 0:
            assert torch.equal(out[r], torch.zeros(P, dtype=torch.float64)), r
            continue
        if (u, s) not in refs:
            seg = rows[c["seg_row"][s]:c["seg_row"][s] + LENS0[s]]
            assert seg[:, :P].abs().max() <= 1.0
            refs[u, s] = _ref(c["q"][u], seg, nh)
        ref, bound = refs[u, s]
        err = (out[r] - ref).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= BOUND * bound).all(), (r, u, s)
    print(f"xattn_seg_mx8 P={P} nh={nh}: max |err| / Σp|v| = {worst:.3e} (bound {BOUND:.3e})")


# ------------------------------------------------------------------ ops.mx8_dequant against numpy
def _dequant_equal(ops, qb, sc):
    got = ops.mx8_dequant(qb, sc)
    torch.cuda.synchronize()
    assert got.dtype == BF16 and got.shape == qb.shape
    return kref_mx8.same_bf16(_bits(got), kref_mx8.mx8_dequant_bits(qb.cpu().numpy(), sc.cpu().numpy()))


@pytest.mark.parametrize("rows,K,ldq", [(1, 128, 128), (5, 128, 136), (37, 384, 384), (300, 1536, 1544)])
def test_mx8_dequant_of_quantised_rows(ops, rows, K, ldq):
    """rows = 1, K = 128 (the smallest the entry accepts), a strided ldq, a zero block, a tail block of threads."""
    g = torch.Generator().manual_seed(rows + K)
    x = (torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, 1), generator=g).float())).to(BF16)
    x[rows // 2, 32:64] = 0                                                    # a zero block: scale byte 0x00
    qb, sc = ops.mx8_quant(x.to(DEV))
    assert sc[rows // 2, 1].item() == 0
    wide = torch.full((rows, ldq), 0x7F, dtype=torch.uint8, device=DEV)
    wide[:, :K] = qb
    assert _dequant_equal(ops, wide[:, :K], sc)
    # the dequantised rows are the quantiser's reading of x: within half an e4m3 step (2^-4 relative) of it
    deq = ops.mx8_dequant(wide[:, :K], sc).float().cpu()
    amax = x.float().view(rows, K // 32, 32).abs().amax(2, keepdim=True).expand(-1, -1, 32).reshape(rows, K)
    assert ((deq - x.float()).abs() <= amax * 2.0 ** -4).all()


@pytest.mark.parametrize("n", [-20, -1, 0, 3, 40])
def test_mx8_dequant_amax_at_448_times_power_of_two(ops, n):
    x = torch.zeros(2, 128)
    x[0, :32] = torch.linspace(-1, 1, 32) * 448 * 2.0 ** n
    x[1, 96:] = 448 * 2.0 ** n
    qb, sc = ops.mx8_quant(x.to(BF16).to(DEV))
    assert sc[0, 0].item() == 127 + n and sc[1, 3].item() == 127 + n
    assert _dequant_equal(ops, qb, sc)
    deq = ops.mx8_dequant(qb, sc).float().cpu()
    assert deq[0, 0].item() == -448 * 2.0 ** n and deq[0, 31].item() == 448 * 2.0 ** n and (deq[1, 96:] == 448 * 2.0 ** n).all()


def test_mx8_dequant_of_every_byte(ops):
    """All 256 e4m3 bytes (both NaNs) under scale bytes over the whole range: the smallest normal scale,
    the scales at which products enter bf16's subnormal range (rounded to nearest even), 2^-127, NaN."""
    scales = [0, 1, 2, 5, 8, 9, 10, 64, 120, 127, 128, 200, 246, 254, 255, 133]
    qb = torch.arange(256, dtype=torch.uint8).repeat(len(scales), 1)                  # [16, 256]
    sc = torch.tensor(scales, dtype=torch.uint8).view(-1, 1).repeat(1, 8)
    assert _dequant_equal(ops, qb.to(DEV), sc.to(DEV))


def test_mx8_dequant_rejects_what_the_quantiser_rejects(ops):
    from speech_transcript_embeddings_amd._lib import SteError
    for rows, K, ldq in ((1, 32, 32), (2, 192, 192), (2, 128, 132)):
        wide = torch.zeros(rows, ldq + 8, dtype=torch.uint8, device=DEV).as_strided((rows, K), (ldq, 1))
        flat = torch.full((rows * K,), 7.0, dtype=BF16, device=DEV)
        with pytest.raises(SteError):
            ops.mx8_dequant(wide, torch.zeros(rows, K // 32, dtype=torch.uint8, device=DEV), flat.view(rows, K))
        torch.cuda.synchronize()
        assert torch.equal(flat, torch.full_like(flat, 7.0))


# ------------------------------------------------------------------ invariance
def test_a_pair_gives_the_same_bits_wherever_it_is(ops):
    P, nh, U = 128, 8, 20
    g = torch.Generator().manual_seed(4)
    q = torch.rand(U, P, generator=g) * 2 - 1
    lens = [129, 40, 77]
    qb, sc, _, seg_row, data = _layout(ops, lens, [2, 0, 1], 2, P, g)
    # inside a 40-pair group of segment 0, at position 23 (tile 1, lane 7)
    qsel = torch.randint(0, U, (40,), generator=g).tolist()
    group = _run(ops, q, qb, seg_row, lens, qsel + [3, 4], [0] * 40 + [1, 2], nh, sc=sc)
    assert torch.isfinite(group).all()
    u = qsel[23]
    alone = _run(ops, q, qb, seg_row, lens, [u], [0], nh, sc=sc)
    assert torch.equal(alone[0], group[23])
    # first pair of another tile, among other pairs and segments
    other = _run(ops, q, qb, seg_row, lens, [1, 2, u, 5, 6], [1, 2, 0, 0, 2], nh, sc=sc)
    assert torch.equal(other[2], group[23])
    # the segment moved to another offset of another buffer, as the only segment: the same bytes, since
    # quantisation is per row
    qb2, sc2, _, row2, _ = _layout(ops, [lens[0]], [0], 7, P, g, data=[data[0]])
    assert row2 == [7] and torch.equal(qb2[7:7 + lens[0]], qb[seg_row[0]:seg_row[0] + lens[0]])
    far = _run(ops, q, qb2, row2, [lens[0]], [0, u], [0, 0], nh, sc=sc2)
    assert torch.equal(far[1], group[23])


def test_torch_op_gives_the_same_bits(ops):
    P, nh, U = 128, 4, 6
    g = torch.Generator().manual_seed(8)
    q = torch.rand(U, P, generator=g) * 2 - 1
    lens = [33, 7, 64]
    qb, sc, _, seg_row, _ = _layout(ops, lens, [1, 2, 0], 2, P, g)
    psel = [0] * 17 + [2, 1, -1, 2]
    qsel = torch.randint(0, U, (len(psel),), generator=g).tolist()
    a = _run(ops, q, qb, seg_row, lens, qsel, psel, nh, sc=sc)
    b = _run(ops, q, qb, seg_row, lens, qsel, psel, nh, sc=sc, via_op=True)
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------ argument checks
def test_shape_errors_launch_nothing(ops):
    """STE_ERR_SHAPE before the memset and the launch: the sentinel-filled out is untouched."""
    from speech_transcript_embeddings_amd._lib import SteError

    def attempt(P=64, nh=8, R=2, G=1, ntile=1, koff=0, pad=0):
        q = torch.zeros(3, P, device=DEV)
        kv = torch.zeros(40, 2 * P + pad, dtype=torch.uint8, device=DEV)
        sc = torch.zeros(40, 2 * (P // 32 + 1), dtype=torch.uint8, device=DEV)
        flat = torch.full((max(R, 1) * P,), 7.0, device=DEV)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)            # noqa: E731
        with pytest.raises(SteError):
            ops.xattn_seg_fwd(q, i32([0] * R), i32([0] * R), kv[:, koff:koff + P], kv[:, koff + P:koff + 2 * P],
                              torch.tensor([0] * G, dtype=torch.int64, device=DEV), i32([8] * G), i32([0] * ntile),
                              i32([R] * ntile), nh, flat[:R * P].view(R, P), ks=sc[:, :P // 32 + 1],
                              vs=sc[:, P // 32 + 1:])
        torch.cuda.synchronize()
        assert torch.equal(flat, torch.full_like(flat, 7.0)), "out is untouched"

    attempt(P=80, nh=10)               # dh = 8 passes the rule of ste_xattn_seg_fwd, but P % 32 != 0
    attempt(P=48, nh=6)
    attempt(koff=4, pad=8)             # k and v 4 bytes off an 8-byte boundary
    attempt(pad=4)                     # ldkv % 8 != 0
    attempt(R=0)
    attempt(G=0)
    attempt(ntile=0)
    attempt(P=64, nh=7)                # the rule of ste_xattn_seg_fwd still holds
