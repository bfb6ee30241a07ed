"""ste_gemm_f32's split-K plan, asked through its host-only queries (no GPU): ste_gemm_f32_plan,
ste_gemm_f32_plan_slab, ste_gemm_f32_ws_floats, ste_gemm_f32_plan_max_tiles, ste_gemm_f32_plan_tile.

The shapes are the 33 fp32 launches of a c2 step (per-GPU batch 64) and of a --batch 32 step, as
profiles/heads_gemm_probe.py traces them from ops.gemm (M, N, K, a_kc, b_kc, epilogue letters as in
the probe's JSON: B bias, C2 pre-activation, Z activation backward, CS column sums, D dropout,
beta; ws: the caller passes the engine's 80 MB workspace), and the shapes of
tests/test_gemm_f32_split_gpu.py.
"""
import ctypes as C

import pytest

WS_ENGINE = 80 << 20


def _heads(b):
    """The fp32 GEMMs of one training step at per-GPU batch b (rows: b audio clips, 2b transcripts,
    2·b·64 text tokens)."""
    b2, t = 2 * b, 2 * b * 64
    return [
        (t, 384, 768, 1, 1, "B", False),
        (b2, 1536, 768, 1, 1, "B C2 D", False), (b2, 768, 1536, 1, 1, "B", False),
        (b, 1536, 1024, 1, 1, "B C2 D", False), (b, 768, 1536, 1, 1, "B", False),
        (b2, 768, 768, 1, 1, "B", False), (b2, 768, 768, 1, 1, "B", False),
        (b, 768, 768, 1, 1, "B", False), (b, 768, 768, 1, 1, "B", False),
        (b2, 768, 1536, 1, 1, "B", False), (b, 768, 1536, 1, 1, "B", False),
        (b2, 1536, 768, 1, 0, "", False), (768, 1536, b2, 0, 0, "beta", True),
        (b, 1536, 768, 1, 0, "", False), (768, 1536, b, 0, 0, "beta", True),
        (b2, 768, 768, 1, 0, "", False), (768, 768, b2, 0, 0, "beta", True),
        (b2, 768, 768, 1, 0, "beta", False), (768, 768, b2, 0, 0, "beta", True),
        (b, 768, 768, 1, 0, "", False), (768, 768, b, 0, 0, "beta", True),
        (b, 768, 768, 1, 0, "beta", False), (768, 768, b, 0, 0, "beta", True),
        (b2, 1536, 768, 1, 0, "Z CS D", False), (768, 1536, b2, 0, 0, "beta", True),
        (b2, 768, 1536, 1, 0, "beta", False), (1536, 768, b2, 0, 0, "beta", True),
        (b, 1536, 768, 1, 0, "Z CS D", False), (768, 1536, b, 0, 0, "beta", True),
        (b, 1024, 1536, 1, 0, "beta", False), (1536, 1024, b, 0, 0, "beta", True),
        (t, 768, 384, 1, 0, "beta", False), (384, 768, t, 0, 0, "beta", True),
    ]


GPU_TEST_SHAPES = [(M, N, K, a, b, e, False) for (M, N, K) in [(4, 68, 528), (68, 64, 1028), (132, 132, 2048)]
                   for a in (1, 0) for b in (1, 0) for e in ("", "B", "B C2 D", "Z CS beta", "B CS")]
CASES = _heads(64) + _heads(32) + GPU_TEST_SHAPES


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.fail("libste.so not built — run __graft_entry__.build()")
    return _lib


def make_args(lib, case):
    M, N, K, a_kc, b_kc, epi, caller_ws = case
    e = epi.split()
    a = lib.GemmArgs()
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.A, a.lda, a.a_kc = 16, (K if a_kc else M), a_kc
    a.B, a.ldb, a.b_kc = 16, (K if b_kc else N), b_kc
    a.C, a.ldc, a.alpha = 16, N, 1.0
    if "B" in e:
        a.bias = 16
    if "C2" in e:
        a.C2, a.ldc2, a.act = 16, N, lib.ACT_GELU
    if "Z" in e:
        a.Z, a.ldz, a.act = 16, N, lib.ACT_GELU_BWD
    if "CS" in e:
        a.colsum = 16
    if "D" in e:
        a.drop_p, a.seed = 0.1, 5
    if "beta" in e:
        a.beta = 1.0
    return a


def tiles(M, N):
    return ((M + 63) // 64) * ((N + 63) // 64)


def old_plan_slabs(case, ws_bytes):
    """The plain weight-gradient split ste_gemm_f32 had before the few-tile plan (restated)."""
    M, N, K, _, _, epi, _ = case
    if set(epi.split()) - {"beta"} or not ws_bytes or tiles(M, N) >= 256 or K < 1024:
        return 1
    S = min((512 + tiles(M, N) - 1) // tiles(M, N), K // 256)
    while S > 1 and S * M * N * 4 > ws_bytes:
        S -= 1
    if S <= 1:
        return 1
    kc = ((K + S - 1) // S + 15) // 16 * 16
    return (K + kc - 1) // kc


def queries(lib):
    return (lib.fn("ste_gemm_f32_plan"), lib.fn("ste_gemm_f32_plan_slab"), lib.fn("ste_gemm_f32_ws_floats"),
            lib.fn("ste_gemm_f32_plan_max_tiles"))


def with_ws(lib, case):
    """(args, need): the arguments as ops.gemm passes them — the caller's workspace if it is large
    enough for ste_gemm_f32_ws_floats, else one of exactly that size."""
    a = make_args(lib, case)
    need = int(lib.fn("ste_gemm_f32_ws_floats")(C.byref(a)))
    if case[6] and WS_ENGINE >= need * 4:
        a.ws, a.ws_bytes = 16, WS_ENGINE
    elif need:
        a.ws, a.ws_bytes = 16, need * 4
    return a, need


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-%d%d-%s%s" % (*c[:5], c[5].replace(" ", "") or "plain",
                                                                               "-ws" if c[6] else ""))
def test_plan(lib, case):
    """With the split on (threshold 64; the library's default is 0, off)."""
    set_max = lib.fn("ste_gemm_f32_plan_max_tiles")
    before = set_max(64)
    try:
        _check_plan(lib, case)
    finally:
        set_max(before)


def _check_plan(lib, case):
    plan, slab, ws_floats, set_max = queries(lib)
    M, N, K = case[:3]
    cs_rows = 2 * ((M + 63) // 64) if "CS" in case[5].split() else 0
    a, need = with_ws(lib, case)
    S, kc = int(plan(C.byref(a))), int(slab(C.byref(a)))
    few = tiles(M, N) <= 64 and K >= 512          # the least the plan promises to split
    old = old_plan_slabs(case, a.ws_bytes)
    if few:
        assert S >= 2, "a few-tile shape with K >= 512 is split"
    if S > 1:
        # slab z = [z*kc, min(K, (z+1)*kc)): starts at multiples of 16, S slabs cover K exactly
        assert kc % 16 == 0 and (S - 1) * kc < K <= S * kc
    else:
        assert kc == K
    if S > 1 and old == 1:
        assert need == S * M * N + cs_rows * N
        # one float short: fewer slabs, never an error; nothing left at all: one launch
        a.ws_bytes = need * 4 - 4
        S1, kc1 = int(plan(C.byref(a))), int(slab(C.byref(a)))
        assert 1 <= S1 < S
        assert (S1 * M * N if S1 > 1 else 0) + cs_rows * N <= need - 1
        assert kc1 % 16 == 0 and (S1 - 1) * kc1 < K <= S1 * kc1
        a.ws, a.ws_bytes = None, 0
        assert int(plan(C.byref(a))) == 1
    elif old > 1:
        assert S == old, "the plain weight-gradient plan keeps its slabs"
    else:
        assert need == cs_rows * N
    # threshold 0: the plan from before the few-tile split, from the same library
    prev = set_max(0)
    try:
        a0, need0 = with_ws(lib, case)
        assert need0 == cs_rows * N
        assert int(plan(C.byref(a0))) == old_plan_slabs(case, a0.ws_bytes)
        if old_plan_slabs(case, a0.ws_bytes) == 1:
            assert int(slab(C.byref(a0))) == K
    finally:
        assert set_max(prev) == 0
    # the tile of the single launch: 32 with few tiles and no column sums
    tile = int(lib.fn("ste_gemm_f32_plan_tile")(C.byref(make_args(lib, case))))
    assert tile == (32 if tiles(M, N) <= 64 and not cs_rows else 64)


def test_threshold_is_returned_and_bounds_the_tile_count(lib):
    plan, _, ws_floats, set_max = queries(lib)
    default = set_max(0)
    try:
        assert default == 0, "the split changes the summation order: off unless asked for"
        assert set_max(2) == 0
        two = make_args(lib, (64, 128, 768, 1, 1, "B", False))     # 2 tiles
        three = make_args(lib, (64, 192, 768, 1, 1, "B", False))   # 3 tiles
        assert ws_floats(C.byref(two)) > 0 and ws_floats(C.byref(three)) == 0
        two.ws, two.ws_bytes = 16, 4 * int(ws_floats(C.byref(two)))
        three.ws, three.ws_bytes = 16, 1 << 30
        assert plan(C.byref(two)) >= 2 and plan(C.byref(three)) == 1
        short = make_args(lib, (64, 128, 496, 1, 1, "B", False))   # K < 512
        short.ws, short.ws_bytes = 16, 1 << 30
        assert plan(C.byref(short)) == 1
    finally:
        set_max(default)
    assert set_max(default) == default
