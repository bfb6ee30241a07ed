"""ste_attn_pool_seg_fwd[_f32] against its contract: every segment of one row buffer pools
to the BITS of the dense ste_attn_pool_fwd[_f32] (B = 1, L = seg_len, no mask) on a copy of its rows,
whatever the other segments are.  One buffer of 5,400 rows whose rows outside every segment are NaN; the
segment lengths sit on the edges of the kernels' shares (8 row-splitting waves, 64 lanes, POOL_WS_NT =
512, NT = 256 and their multiples); the segments overlap (two pairs by half, one nested, one repeated) and
are passed shuffled.  Strict throughout: torch.equal, no tolerance."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(4, 4), (256, 260), (1024, 1024), (64, 768)]
ROWS = 5400
# (first row, length): 1025 nested in 2048; 1024 / 1023 and 513 / 512 overlapping by half; 64 repeated
SEGS = [(100, 2048), (600, 1025), (2200, 1024), (2712, 1023), (3800, 513), (4056, 512), (4600, 511), (5120, 65),
        (5190, 64), (5190, 64), (5260, 63), (5330, 9), (5342, 8), (5352, 7), (5362, 1)]
ORDER = [7, 2, 14, 0, 9, 5, 11, 3, 13, 1, 8, 12, 4, 10, 6]
assert sorted(n for _, n in set(SEGS)) == [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2048]
assert sorted(ORDER) == list(range(len(SEGS)))
ERR_ARG, ERR_SHAPE = 1001, 1002


def _dense(t, w2, b2, h):
    """The dense pooling of ONE sample given as copies of its rows -> (pooled fp32 [H], pooled bf16 [H])."""
    from speech_transcript_embeddings_amd import ops
    L, H = h.shape
    w = torch.empty(L, device=DEV, dtype=F32)
    pooled = torch.empty(1, H, device=DEV, dtype=F32)
    pb = torch.empty(1, H, device=DEV, dtype=BF16)
    (ops.attn_pool_fwd_f32 if h.dtype == F32 else ops.attn_pool_fwd)(t, w2, b2, h, None, 1, L, w, pooled, pb)
    return pooled[0], pb[0]


def _tables(segs):
    return (torch.tensor([r for r, _ in segs], dtype=torch.int64, device=DEV),
            torch.tensor([n for _, n in segs], dtype=torch.int32, device=DEV))


_CASES = {}


def case(Hh, H, dtype):
    """The buffer, the scorer's second layer and the dense reference of every segment, computed once per
    (Hh, H, dtype) and never written again."""
    key = (Hh, H, dtype)
    if key not in _CASES:
        g = torch.Generator(device="cpu").manual_seed(1000 * Hh + H)
        t = (torch.rand(ROWS, Hh, generator=g) * 2 - 1).to(DEV).to(dtype)
        h = torch.randn(ROWS, H, generator=g).to(DEV).to(dtype)
        w2 = (torch.randn(Hh, generator=g) * (4.0 / Hh ** 0.5)).to(DEV)
        b2 = torch.tensor([0.25], device=DEV)
        inside = torch.zeros(ROWS, dtype=torch.bool, device=DEV)
        for r, n in SEGS:
            inside[r:r + n] = True
        assert int((~inside).sum()) > 100
        t[~inside] = float("nan")
        h[~inside] = float("nan")
        ref = [_dense(t[r:r + n].clone(), w2, b2, h[r:r + n].clone()) for r, n in SEGS]
        assert all(bool(torch.isfinite(p).all()) for p, _ in ref)
        _CASES[key] = dict(t=t, h=h, w2=w2, b2=b2, ref=ref)
    return _CASES[key]


PARAMS = [pytest.param(Hh, H, dt, id=f"{Hh}x{H}-{'f32' if dt == F32 else 'bf16'}") for Hh, H in SHAPES for dt in (F32, BF16)]


@pytest.mark.parametrize("Hh,H,dtype", PARAMS)
def test_every_segment_is_the_dense_pooling_of_its_rows(Hh, H, dtype):
    from speech_transcript_embeddings_amd import ops
    c = case(Hh, H, dtype)
    segs = [SEGS[i] for i in ORDER]
    seg_row, seg_len = _tables(segs)
    pb = torch.empty(len(segs), H, device=DEV, dtype=BF16)
    pooled = ops.attn_pool_seg_fwd(c["t"], c["w2"], c["b2"], c["h"], seg_row, seg_len, pooled_bf16=pb)
    assert pooled.shape == (len(segs), H) and pooled.dtype == F32
    for j, i in enumerate(ORDER):
        assert torch.equal(pooled[j], c["ref"][i][0]), SEGS[i]
        assert torch.equal(pb[j], c["ref"][i][1]), SEGS[i]
    # the repeated segment, wherever its two copies landed
    a, b = ORDER.index(8), ORDER.index(9)
    assert torch.equal(pooled[a], pooled[b])


@pytest.mark.parametrize("Hh,H,dtype", PARAMS)
def test_a_segment_does_not_depend_on_the_others(Hh, H, dtype):
    from speech_transcript_embeddings_amd import ops
    c = case(Hh, H, dtype)
    for i in (0, 3, 5, 7, 14):
        r, n = SEGS[i]
        # alone, at row 0 of another buffer
        tt, hh = c["t"][r:r + n].clone(), c["h"][r:r + n].clone()
        alone = ops.attn_pool_seg_fwd(tt, c["w2"], c["b2"], hh, *_tables([(0, n)]))
        assert torch.equal(alone[0], c["ref"][i][0]), SEGS[i]
        # the last of five, behind an empty one
        five = ops.attn_pool_seg_fwd(c["t"], c["w2"], c["b2"], c["h"],
                                     *_tables([SEGS[1], SEGS[10], SEGS[4], (r, 0), (r, n)]))
        assert torch.equal(five[4], c["ref"][i][0]), SEGS[i]
        assert bool((five[3] == 0).all())


@pytest.mark.parametrize("Hh,H,dtype", PARAMS)
def test_empty_and_infeasible_segments_pool_to_zeros(Hh, H, dtype):
    from speech_transcript_embeddings_amd import ops
    c = case(Hh, H, dtype)
    # (row, len): none, negative, longer than 8192, before the buffer, past its end; NaN rows would show a read
    empty = [(3000, 0), (3000, -3), (0, 8193), (-1, 5), (ROWS - 3, 5), (-2 ** 40, 7), (2 ** 40, 7)]
    real = [SEGS[4], SEGS[12], SEGS[7]]
    segs = [empty[0], real[0], empty[1], empty[2], real[1], empty[3], empty[4], real[2], empty[5], empty[6]]
    G = len(segs)
    big = torch.full((G + 2, H), float("nan"), device=DEV)
    bigb = torch.full((G + 2, H), float("nan"), device=DEV, dtype=BF16)
    out = ops.attn_pool_seg_fwd(c["t"], c["w2"], c["b2"], c["h"], *_tables(segs), big[:G], pooled_bf16=bigb[:G])
    assert out.data_ptr() == big.data_ptr()
    for g, s in enumerate(segs):
        if s in real:
            ref = c["ref"][SEGS.index(s)]
            assert torch.equal(big[g], ref[0]) and torch.equal(bigb[g], ref[1]), s
        else:
            assert bool((big[g] == 0).all()) and bool((bigb[g] == 0).all()), s
    assert bool(torch.isnan(big[G:]).all()) and bool(torch.isnan(bigb[G:]).all())     # the guard rows


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_the_longest_segment_and_one_row_more(dtype):
    """8192 rows is the dense kernels' limit and the segment limit: pooled as the dense kernel does;
    8193 rows inside a 9,000-row buffer is an empty segment."""
    from speech_transcript_embeddings_amd import ops
    g = torch.Generator(device="cpu").manual_seed(8192)
    t = (torch.rand(9000, 4, generator=g) * 2 - 1).to(DEV).to(dtype)
    h = torch.randn(9000, 4, generator=g).to(DEV).to(dtype)
    w2, b2 = torch.tensor([1.5, -2.0, 0.5, 1.0], device=DEV), torch.tensor([-0.5], device=DEV)
    out = ops.attn_pool_seg_fwd(t, w2, b2, h, *_tables([(808, 8192), (0, 8193), (807, 8193)]))
    assert torch.equal(out[0], _dense(t[808:].clone(), w2, b2, h[808:].clone())[0])
    assert bool((out[1:] == 0).all())


def test_seventy_thousand_one_row_segments():
    """G beyond 65,535 (the y and z grid limit): a one-row segment has weight exp(0) · 1/1 = 1 and pools to
    its row; a few of them against the dense kernel."""
    from speech_transcript_embeddings_amd import ops
    G, rows, Hh, H = 70000, 300, 8, 260
    g = torch.Generator(device="cpu").manual_seed(7)
    t = (torch.rand(rows, Hh, generator=g) * 2 - 1).to(DEV)
    h = torch.randn(rows, H, generator=g).to(DEV)
    w2, b2 = torch.randn(Hh, generator=g).to(DEV), torch.tensor([0.1], device=DEV)
    seg_row = torch.randint(0, rows, (G,), generator=g).to(DEV)
    out = ops.attn_pool_seg_fwd(t, w2, b2, h, seg_row, torch.ones(G, dtype=torch.int32, device=DEV))
    assert torch.equal(out, h[seg_row])
    for j in (0, 65535, 65536, G - 1):
        r = int(seg_row[j])
        assert torch.equal(out[j], _dense(t[r:r + 1].clone(), w2, b2, h[r:r + 1].clone())[0])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wrapper_and_custom_op(dtype):
    from speech_transcript_embeddings_amd import ops, torch_ops  # noqa: F401  (registers the op)
    c = case(64, 768, dtype)
    seg_row, seg_len = _tables(SEGS)
    want = torch.stack([p for p, _ in c["ref"]])
    given = torch.full((len(SEGS), 768), float("nan"), device=DEV)
    assert ops.attn_pool_seg_fwd(c["t"], c["w2"], c["b2"], c["h"], seg_row, seg_len, given) is given
    assert torch.equal(given, want)
    # the op takes the tables in any integer dtype and the scorer's weight as the Linear's [1, Hh]
    out = torch.ops.ste.attn_pool_seg(c["t"], c["w2"].view(1, -1), c["b2"], c["h"], seg_row.to(torch.int32),
                                      seg_len.to(torch.int64))
    assert torch.equal(out, want)


def test_refusals_leave_the_buffers_untouched():
    from speech_transcript_embeddings_amd import _lib, ops
    c = case(64, 768, F32)
    seg_row, seg_len = _tables(SEGS[:3])
    score = torch.full((ROWS,), float("nan"), device=DEV)
    stat = torch.full((3, 2), float("nan"), device=DEV)
    pooled = torch.full((3, 768), float("nan"), device=DEV)
    f = _lib.fn("ste_attn_pool_seg_fwd_f32")
    s = _lib.stream_ptr()

    def call(G=3, rows=ROWS, Hh=64, H=768, t=c["t"].data_ptr(), out=pooled.data_ptr()):
        return f(t, c["w2"].data_ptr(), c["b2"].data_ptr(), c["h"].data_ptr(), rows, seg_row.data_ptr(),
                 seg_len.data_ptr(), G, Hh, H, score.data_ptr(), stat.data_ptr(), out, None, s)

    assert call(G=0) == ERR_SHAPE and call(rows=0) == ERR_SHAPE and call(Hh=62) == ERR_SHAPE
    assert call(H=766) == ERR_SHAPE and call(t=None) == ERR_ARG and call(out=None) == ERR_ARG
    with pytest.raises(ValueError):
        ops.attn_pool_seg_fwd(c["t"], c["w2"], c["b2"], c["h"], seg_row, seg_len.long(), pooled)
    with pytest.raises(ValueError):
        ops.attn_pool_seg_fwd(c["t"][:, :62].contiguous(), c["w2"][:62].contiguous(), c["b2"], c["h"], seg_row, seg_len,
                              pooled)
    torch.cuda.synchronize()
    assert bool(torch.isnan(score).all()) and bool(torch.isnan(stat).all()) and bool(torch.isnan(pooled).all())
    assert call() == 0                                                       # and the accepted call writes all three
    torch.cuda.synchronize()
    assert torch.equal(pooled, torch.stack([p for p, _ in c["ref"][:3]]))
    assert bool(torch.isfinite(stat).all()) and bool(torch.isfinite(score[100:2148]).all())
