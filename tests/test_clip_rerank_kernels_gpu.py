"""ste_xattn_seg_fwd (csrc/xattn_mq.hip): (query, segment) pairs against runs of rows of
one K/V buffer, planned by retrieval.plan_clip_pairs.

The bound is §15's, derived there and not re-measured: against float64 attention on the same fp32 q
and the widened bf16 K/V, with |q|, |k| <= 1, elementwise

    |out - ref| <= 2^-8 · Σ_s p_s·|v_s,c|        (p the float64 softmax)

The other checks are exact: the same bits as ste_xattn_mq_fwd on uniform segments, the same values as
ste_xattn_mq_fwd with a prefix mask on the truncated rows (the store drops padded frames), and the
same bits for a pair wherever it and its segment are placed.

Measured on an MI355X, worst |err| / Σp|v| of the one-launch case: 1.14e-3 (P = 64), 1.18e-3 (128),
1.33e-3 (768), 1.48e-3 (1024) against the bound 3.91e-3.
"""
import pytest
import torch

from speech_transcript_embeddings_amd.retrieval import plan_clip_pairs

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops as o
    return o


def _rows(n, P, g):
    """n bf16 K|V rows [n, 2P]: |k| <= 1, v normal."""
    return torch.cat([(torch.rand(n, P, generator=g) * 2 - 1), torch.randn(n, P, generator=g)], 1).to(BF16)


def _layout(lens, order, gap, P, g):
    """Segments of the given lengths laid out in `order` with `gap` unused NaN rows before, between and
    after them -> (buffer [rows, 2P] bf16, seg_row list, per-segment rows list)."""
    data = [_rows(n, P, g) for n in lens]
    seg_row, at = [0] * len(lens), gap
    for s in order:
        seg_row[s] = at
        at += lens[s] + gap
    buf = torch.full((at, 2 * P), float("nan"), dtype=BF16)
    for s, n in enumerate(lens):
        buf[seg_row[s]:seg_row[s] + n] = data[s]
    return buf, seg_row, data


def _run(ops, q, buf, seg_row, seg_len, qsel, psel, nh, via_op=False):
    """Pairs (row qsel[r] of q, segment psel[r]) in any order, -1 = empty -> out [R, P] in that order."""
    P = q.shape[1]
    plan = plan_clip_pairs(torch.tensor(psel, dtype=torch.int32).view(-1, 1))
    used = plan["unique"].long()
    qs = torch.tensor(qsel, dtype=torch.int32)
    qrow = torch.where(plan["qrow"] >= 0, qs[plan["qrow"].clamp(min=0).long()], plan["qrow"])
    d = lambda t: t.contiguous().to(DEV)                                           # noqa: E731
    args = (d(q), d(qrow), d(plan["pseg"]), buf[:, :P], buf[:, P:2 * P],
            d(torch.tensor(seg_row, dtype=torch.int64)[used]), d(torch.tensor(seg_len, dtype=torch.int32)[used]),
            d(plan["tile_first"]), d(plan["tile_cnt"]))
    if via_op:
        out = torch.ops.ste.xattn_seg(*args, nh)
    else:
        out = torch.full((len(psel), P), float("nan"), device=DEV)
        ops.xattn_seg_fwd(*args, nh, out)
    torch.cuda.synchronize()
    return out.index_select(0, plan["inverse"].view(-1).to(DEV))


def _ref(qv, rows, nh):
    """float64 attention of one query [P] over rows [S, 2P] -> (out [P], Σ p|v| [P])."""
    S, P = rows.shape[0], qv.shape[0]
    d = P // nh
    k, v = rows[:, :P].double().reshape(S, nh, d), rows[:, P:].double().reshape(S, nh, d)
    p = (torch.einsum("hd,shd->hs", qv.double().reshape(nh, d), k) * d ** -0.5).softmax(-1)
    return torch.einsum("hs,shd->hd", p, v).reshape(P), torch.einsum("hs,shd->hd", p, v.abs()).reshape(P)


LENS = [1, 31, 32, 33, 129, 1500]
PAIRS = [16, 1, 40, 17, 16, 17]          # pairs per segment: {1, 16, 17, 40}
ORDER = [3, 5, 0, 4, 2, 1]               # where the segments lie in the buffer


@pytest.mark.parametrize("P,nh", [(64, 8), (128, 4), (768, 8), (1024, 4)])
def test_xattn_seg_fwd_bound(ops, P, nh):
    """One launch: every segment length around the 32-key tile and the 4-wave split, every pair count
    around the 16-pair tile, empty pairs, the segments out of order between NaN rows."""
    g = torch.Generator().manual_seed(P + nh)
    U = 9
    q = torch.rand(U, P, generator=g) * 2 - 1
    buf, seg_row, data = _layout(LENS, ORDER, 3, P, g)
    psel = [s for s, n in enumerate(PAIRS) for _ in range(n)] + [-1] * 5
    perm = torch.randperm(len(psel), generator=g).tolist()
    psel = [psel[i] for i in perm]
    qsel = torch.randint(0, U, (len(psel),), generator=g).tolist()
    qsel[3] = -1                                                   # a pair without a query
    out = _run(ops, q, buf.to(DEV), seg_row, LENS, qsel, psel, nh).cpu().double()
    assert torch.isfinite(out).all(), "a stray read of a gap row shows as NaN"
    refs, worst = {}, 0.0
    for r, (u, s) in enumerate(zip(qsel, psel)):
        if u < 0 or s < 0:
            assert torch.equal(out[r], torch.zeros(P, dtype=torch.float64)), r
            continue
        if (u, s) not in refs:
            refs[u, s] = _ref(q[u], data[s], nh)
        ref, bound = refs[u, s]
        err = (out[r] - ref).abs()
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= BOUND * bound).all(), (r, u, s)
    print(f"xattn_seg P={P} nh={nh}: max |err| / Σp|v| = {worst:.3e} (bound {BOUND:.3e})")


def test_equal_to_xattn_mq_on_uniform_segments(ops):
    P, nh, B, C, S, U = 128, 8, 3, 5, 77, 7
    g = torch.Generator().manual_seed(1)
    q = (torch.rand(U, P, generator=g) * 2 - 1).to(DEV)
    kv = _rows(B * S, P, g).to(DEV)
    qrow = torch.randint(0, U, (B * C,), generator=g, dtype=torch.int32)
    want = torch.empty(B * C, P, device=DEV)
    ops.xattn_mq_fwd(q, qrow.to(DEV), kv[:, :P], kv[:, P:], None, B, C, S, nh, want)
    psel = [b for b in range(B) for _ in range(C)]
    got = _run(ops, q.cpu(), kv, [b * S for b in range(B)], [S] * B, qrow.tolist(), psel, nh)
    assert torch.equal(got, want)


def test_truncated_rows_equal_the_masked_padded_rows(ops):
    """What lets the store drop padded frames: ste_xattn_mq_fwd over S = 77 padded rows with a prefix
    mask gives the values of the attention over the valid prefix alone (a zero's sign may differ)."""
    P, nh, S, C, U = 128, 8, 77, 3, 7
    valid = [1, 31, 33, 64, 77]
    B = len(valid)
    g = torch.Generator().manual_seed(2)
    q = (torch.rand(U, P, generator=g) * 2 - 1).to(DEV)
    kv = _rows(B * S, P, g).to(DEV)                       # the padded rows are random and finite
    mask = torch.zeros(B, S, dtype=torch.int32)
    for b, n in enumerate(valid):
        mask[b, :n] = 1
    qrow = torch.randint(0, U, (B * C,), generator=g, dtype=torch.int32)
    want = torch.empty(B * C, P, device=DEV)
    ops.xattn_mq_fwd(q, qrow.to(DEV), kv[:, :P], kv[:, P:], mask.reshape(-1).to(DEV), B, C, S, nh, want)
    psel = [b for b in range(B) for _ in range(C)]
    got = _run(ops, q.cpu(), kv, [b * S for b in range(B)], valid, qrow.tolist(), psel, nh)
    assert torch.equal(got, want)


def test_a_pair_gives_the_same_bits_wherever_it_is(ops):
    P, nh, U = 128, 8, 20
    g = torch.Generator().manual_seed(4)
    q = torch.rand(U, P, generator=g) * 2 - 1
    lens = [129, 40, 77]
    buf, seg_row, data = _layout(lens, [2, 0, 1], 2, P, g)
    buf = buf.to(DEV)
    # inside a 40-pair group of segment 0, at position 23 (tile 1, lane 7)
    qsel = torch.randint(0, U, (40,), generator=g).tolist()
    group = _run(ops, q, buf, seg_row, lens, qsel + [3, 4], [0] * 40 + [1, 2], nh)
    u = qsel[23]
    alone = _run(ops, q, buf, seg_row, lens, [u], [0], nh)
    assert torch.equal(alone[0], group[23])
    # another tile position among other pairs and segments: first pair of its segment, 5 pairs in all
    other = _run(ops, q, buf, seg_row, lens, [1, 2, u, 5, 6], [1, 2, 0, 0, 2], nh)
    assert torch.equal(other[2], group[23])
    # the segment moved elsewhere, in another buffer, as the only segment
    moved = torch.full((7 + lens[0] + 1, 2 * P), float("nan"), dtype=BF16)
    moved[7:7 + lens[0]] = data[0]
    far = _run(ops, q, moved.to(DEV), [7], [lens[0]], [0, u], [0, 0], nh)
    assert torch.equal(far[1], group[23])


def test_a_segment_past_2_31_elements(ops):
    """A store passes 2^31 rows·columns quickly: a segment whose first element lies past 2^31 elements
    (and past 2^32 bytes) of the buffer gives the bits of the same rows at the start of a small buffer."""
    P, nh, U, S = 64, 8, 5, 33
    g = torch.Generator().manual_seed(9)
    q = torch.rand(U, P, generator=g) * 2 - 1
    seg = _rows(S, P, g)
    near = _run(ops, q, seg.to(DEV), [0], [S], [1, 4], [0, 0], nh)
    first = 2 ** 24 + 5
    assert first * 2 * P > 2 ** 31
    big = torch.empty(first + S, 2 * P, dtype=BF16, device=DEV)          # 4.3 GB, left uninitialised
    big[:64].zero_()
    big[first:first + S] = seg.to(DEV)
    far = _run(ops, q, big, [0, first], [7, S], [1, 4, 2], [1, 1, 0], nh)
    assert torch.equal(far[:2], near)


def test_empty_pairs_and_empty_segments_are_zero_rows(ops):
    P, nh, U = 64, 8, 4
    g = torch.Generator().manual_seed(6)
    q = torch.rand(U, P, generator=g) * 2 - 1
    lens = [5, 0, 33]
    buf, seg_row, _ = _layout(lens, [0, 1, 2], 1, P, g)
    out = _run(ops, q, buf.to(DEV), seg_row, lens, [0, 1, 2, -1, 3, 1], [0, 1, -1, 2, 2, 1], nh)
    zero = torch.zeros(P, device=DEV)
    for r in (1, 2, 3, 5):                         # empty segment, empty pair, no query, empty segment
        assert torch.equal(out[r], zero), r
    assert torch.isfinite(out).all() and out[0].abs().sum() > 0 and out[4].abs().sum() > 0
    # nothing but empty pairs: no tile at all
    none = _run(ops, q, buf.to(DEV), seg_row, lens, [0, 1], [1, 1], nh)
    assert torch.equal(none, torch.zeros(2, P, device=DEV))


def test_shape_errors_launch_nothing(ops):
    from speech_transcript_embeddings_amd._lib import SteError

    def attempt(P, nh, R=2, misalign=False):
        q = torch.zeros(3, P, device=DEV)
        kv = torch.zeros(40, 2 * P, device=DEV, dtype=BF16)
        flat = torch.full((R * P + 1,), 7.0, device=DEV)
        out = flat[1:].view(R, P) if misalign else flat[:R * P].view(R, P)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)            # noqa: E731
        with pytest.raises(SteError):
            ops.xattn_seg_fwd(q, i32([0] * R), i32([0] * R), kv[:, :P], kv[:, P:],
                              torch.tensor([0], dtype=torch.int64, device=DEV), i32([8]), i32([0]), i32([R]), nh, out)
        torch.cuda.synchronize()
        assert torch.equal(flat, torch.full_like(flat, 7.0)), "out is untouched"

    attempt(80, 8)                     # dh = 10, not a multiple of 8
    attempt(64, 7)                     # P % nh != 0
    attempt(64, 8, misalign=True)      # out 4 bytes off a 16-byte boundary
    attempt(64, 8, R=0)                # no pairs


def test_torch_op_gives_the_same_bits(ops):
    P, nh, U = 128, 4, 6
    g = torch.Generator().manual_seed(8)
    q = torch.rand(U, P, generator=g) * 2 - 1
    lens = [33, 7, 64]
    buf, seg_row, _ = _layout(lens, [1, 2, 0], 2, P, g)
    buf = buf.to(DEV)
    psel = [0] * 17 + [2, 1, -1, 2]
    qsel = torch.randint(0, U, (len(psel),), generator=g).tolist()
    a = _run(ops, q, buf, seg_row, lens, qsel, psel, nh)
    b = _run(ops, q, buf, seg_row, lens, qsel, psel, nh, via_op=True)
    assert torch.equal(a, b)
