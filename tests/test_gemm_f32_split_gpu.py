"""The few-tile split-K plan of ste_gemm_f32 (csrc/gemm_f32.hip): K-slabs of raw accumulators in
the workspace, then gemm_f32_reduce_kernel, which rebuilds each accumulator in slab order and runs
the one epilogue function the single launch runs.

Shapes (M, N, K), the smallest at which the split can go wrong:
  (4, 68, 528)      one ragged row tile, a column tile with 4 valid columns, 33 chunks: uneven slabs
  (68, 64, 1028)    two row tiles, K % 16 = 4: the last slab ends in a ragged chunk
  (132, 132, 2048)  three row tiles, three column tiles
in all four a_kc / b_kc layouts (M, N and K are multiples of 4, so every layout is admissible).

a. integer operands in [-8, 8]: every partial sum is below 2^24, exact in any order, so C, C2, C3
   and the ordered column sums must equal the threshold-0 (single launch, the default) call of the same library
   bit for bit under every epilogue feature; plain and bias also equal fp64 rounded once.
b. normal operands, plain and bias: |C - C64| <= (K + 2)·2^-24·|alpha|·Σ_k |a_k||b_k| element-wise,
   the fp32 summation bound of any order.
c. two calls on the same inputs are bitwise equal, column sums included.
d. a workspace too small for two slabs gives the single launch's result bitwise (C ABI call).
e. the 32x32 tiling (few tiles, no column sums) against the 64x64 tiling of the same library
   (ste_gemm_f32_plan_small_tiles(0)) on normal operands: every output bitwise equal, because an
   output element sees the same MFMAs in the same k order; plus (100, 36, 52), a K below one chunk.
"""
import contextlib
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT_ON = 64   # ste_gemm_f32_plan_max_tiles for the split calls (the library's default is 0: off)
SHAPES = [(4, 68, 528), (68, 64, 1028), (132, 132, 2048)]
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
CASES = [(s, l) for s in SHAPES for l in LAYOUTS]
IDS = ["%dx%dx%d-a%s-b%s" % (*s, "kc" if l[0] else "km", "kc" if l[1] else "km") for s, l in CASES]


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def max_tiles(tiles):
    """The few-tile threshold for the calls inside (None: the library's default)."""
    from speech_transcript_embeddings_amd import _lib
    f = _lib.fn("ste_gemm_f32_plan_max_tiles")
    if tiles is None:
        yield
        return
    prev = f(tiles)
    try:
        yield
    finally:
        f(prev)


def launch(ops, A, B, layout, tiles, **kw):
    """ops.gemm on the logical A [M, K], B [N, K] in the given layout; returns the slab count S the
    library planned for exactly the arguments ops.gemm passed."""
    from speech_transcript_embeddings_amd import _lib
    a = A if layout[0] else A.t().contiguous()
    b = B if layout[1] else B.t().contiguous()
    seen, real = [], ops.call

    def spy(name, *args):
        if name == "ste_gemm_f32":
            seen.append(int(_lib.fn("ste_gemm_f32_plan")(args[0])))
        return real(name, *args)

    ops.call = spy
    try:
        with max_tiles(tiles):
            ops.gemm(a, b, a_kc=layout[0], b_kc=layout[1], M=A.shape[0], N=B.shape[0], K=A.shape[1], **kw)
    finally:
        ops.call = real
    torch.cuda.synchronize()
    assert len(seen) == 1
    return seen[0]


def ints(g, *shape, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g, device=DEV).float()


def epilogues(M, N, g, integer):
    """name -> (kwargs factory, output names).  Fresh output tensors per call; inputs shared."""
    from speech_transcript_embeddings_amd import _lib
    bias = ints(g, N) if integer else torch.randn(N, generator=g, device=DEV)
    z = torch.randn(M, N, generator=g, device=DEV)
    rs = (torch.rand(M, generator=g, device=DEV) > 0.3).float() * 2.0
    r = torch.randn(M, N, generator=g, device=DEV)
    c0 = torch.randn(M, N, generator=g, device=DEV)

    def f32():
        return torch.full((M, N), float("nan"), device=DEV)

    def bf():
        return torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)

    return {
        "plain": lambda: dict(out=f32()),
        "bias": lambda: dict(out=f32(), bias=bias, alpha=0.75),
        "bias_gelu_c2_drop_c3lo": lambda: dict(out=f32(), bias=bias, act=_lib.ACT_GELU, pre_out=f32(), drop_p=0.1,
                                               seed=1234, out_bf16_copy=bf(), copy_lo=True),
        "gelubwd_z_rs_colsum_res_beta": lambda: dict(out=c0.clone(), act=_lib.ACT_GELU_BWD, z=z, row_scale=rs,
                                                     colsum=torch.zeros(N, device=DEV), residual=r, beta=1.0,
                                                     alpha=0.5),
        "bias_tanh_colsum": lambda: dict(out=f32(), bias=bias, act=_lib.ACT_TANH, alpha=2.0 ** -10,
                                         colsum=torch.zeros(N, device=DEV)),
    }


def outputs(kw):
    return {k: kw[k] for k in ("out", "pre_out", "out_bf16_copy", "colsum") if kw.get(k) is not None}


def bits_equal(x, y):
    return x.dtype == y.dtype and torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                              y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("shape,layout", CASES, ids=IDS)
def test_exact_every_epilogue(ops, shape, layout):
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N * 3 + K)
    A, B = ints(g, M, K), ints(g, N, K)
    acc64 = A.double() @ B.double().t()
    assert acc64.abs().max().item() < 2 ** 24
    for name, make in epilogues(M, N, g, integer=True).items():
        new, ref = make(), make()
        S = launch(ops, A, B, layout, SPLIT_ON, **new)
        assert S >= 2, f"{name}: the plan did not split (S = {S})"
        assert launch(ops, A, B, layout, 0, **ref) == 1, name
        for k, v in outputs(new).items():
            assert bits_equal(v, outputs(ref)[k]), f"{name}: {k} differs from the single launch"
        if name == "plain":
            assert torch.equal(new["out"], acc64.float())
        elif name == "bias":
            assert torch.equal(new["out"], ((acc64 + new["bias"].double()) * 0.75).float())


@pytest.mark.parametrize("shape,layout", CASES, ids=IDS)
def test_normal_data_within_the_summation_bound(ops, shape, layout):
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(M + N + K + 1)
    A, B = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV)
    acc64 = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    eps = epilogues(M, N, g, integer=False)
    for name in ("plain", "bias"):
        kw = eps[name]()
        alpha = kw.get("alpha", 1.0)
        assert launch(ops, A, B, layout, SPLIT_ON, **kw) >= 2
        ref = (acc64 + (kw["bias"].double() if "bias" in kw else 0.0)) * alpha
        err = (kw["out"].double() - ref).abs()
        bound = (K + 2) * 2.0 ** -24 * abs(alpha) * mag
        print(f"[f32 split] {shape} {layout} {name}: max err / bound = {(err / bound).max().item():.4f}")
        assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements out of bound"


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_deterministic(ops, shape):
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(K)
    A, B = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV)
    make = epilogues(M, N, g, integer=False)["gelubwd_z_rs_colsum_res_beta"]
    one, two = make(), make()
    assert launch(ops, A, B, (True, False), SPLIT_ON, **one) >= 2
    assert launch(ops, A, B, (True, False), SPLIT_ON, **two) >= 2
    assert bits_equal(one["out"], two["out"]) and bits_equal(one["colsum"], two["colsum"])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_small_workspace_falls_back_to_one_launch(ops, shape):
    """ws one float short of two slabs plus the column-sum rows: S = 1, the result of the call
    without the split (the column sums stay ordered: their rows still fit)."""
    from speech_transcript_embeddings_amd import _lib
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(K + 5)
    A, B = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV)
    bias = torch.randn(N, generator=g, device=DEV)
    rows = 2 * ((M + 63) // 64)
    need2 = 2 * M * N + rows * N            # two slabs and the ordered column-sum rows
    ws = torch.empty(need2, device=DEV)

    def call(tiles, ws_floats):
        out, cs = torch.empty(M, N, device=DEV), torch.zeros(N, device=DEV)
        a = _lib.GemmArgs()
        a.M, a.N, a.K, a.batch = M, N, K, 1
        a.A, a.lda, a.a_kc, a.B, a.ldb, a.b_kc = _lib.ptr(A), K, 1, _lib.ptr(B), K, 1
        a.C, a.ldc, a.bias, a.colsum, a.alpha = _lib.ptr(out), N, _lib.ptr(bias), _lib.ptr(cs), 1.0
        a.ws, a.ws_bytes = _lib.ptr(ws), 4 * ws_floats
        with max_tiles(tiles):
            S = int(_lib.fn("ste_gemm_f32_plan")(C.byref(a)))
            _lib.call("ste_gemm_f32", C.byref(a), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return S, out, cs

    S_fit, _, _ = call(SPLIT_ON, need2)
    S_small, out_small, cs_small = call(SPLIT_ON, need2 - 1)
    S_ref, out_ref, cs_ref = call(0, need2 - 1)
    assert (S_fit, S_small, S_ref) == (2, 1, 1)
    assert bits_equal(out_small, out_ref) and bits_equal(cs_small, cs_ref)


@contextlib.contextmanager
def small_tiles(tiles):
    from speech_transcript_embeddings_amd import _lib
    f = _lib.fn("ste_gemm_f32_plan_small_tiles")
    prev = f(tiles)
    try:
        yield
    finally:
        f(prev)


@pytest.mark.parametrize("shape,layout", [(s, l) for s in SHAPES + [(100, 36, 52)] for l in LAYOUTS],
                         ids=IDS + ["100x36x52-%d%d" % l for l in LAYOUTS])
def test_small_tiles_equal_the_64x64_tiling_bitwise(ops, shape, layout):
    from speech_transcript_embeddings_amd import _lib
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(M + 3 * N + 5 * K)
    A, B = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV)
    a = A if layout[0] else A.t().contiguous()
    b = B if layout[1] else B.t().contiguous()
    r, c0 = torch.randn(M, N, generator=g, device=DEV), torch.randn(M, N, generator=g, device=DEV)
    eps = epilogues(M, N, g, integer=False)
    cases = {k: eps[k] for k in ("plain", "bias", "bias_gelu_c2_drop_c3lo")}
    z, rs = torch.randn(M, N, generator=g, device=DEV), torch.rand(M, generator=g, device=DEV)
    cases["gelubwd_z_rs_res_beta"] = lambda: dict(out=c0.clone(), act=_lib.ACT_GELU_BWD, z=z, row_scale=rs, residual=r,
                                                  beta=1.0, alpha=0.5)
    for name, make in cases.items():
        tiles_seen = []
        real = ops.call

        def spy(fname, *args):
            if fname == "ste_gemm_f32":
                tiles_seen.append(int(_lib.fn("ste_gemm_f32_plan_tile")(args[0])))
            return real(fname, *args)

        outs = []
        for limit in (64, 0):
            kw = make()
            ops.call = spy
            try:
                with small_tiles(limit):
                    ops.gemm(a, b, a_kc=layout[0], b_kc=layout[1], M=M, N=N, K=K, **kw)
            finally:
                ops.call = real
            torch.cuda.synchronize()
            outs.append(outputs(kw))
        assert tiles_seen == [32, 64], (name, tiles_seen)
        for k in outs[0]:
            assert bits_equal(outs[0][k], outs[1][k]), f"{name}: {k} differs between the tilings"
