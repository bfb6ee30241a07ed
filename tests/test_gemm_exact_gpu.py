"""Exact-arithmetic parity of the GEMM kernels at their tile edges (cases: gemm_exact_cases.py).

Integer-valued operands (bf16 integers in [-4, 4], or [-1, 1] at the large-M shapes; e4m3 integers in
[-8, 8] with E8M0 block scales 2^-1, 1, 2; fp32 integers in [-64, 64]) make every product and every
partial sum an integer multiple of one power of two below 2^24 of that unit, so fp32 accumulation is
exact in any order and each output must equal the fp64 reference BIT FOR BIT: torch.equal, no
tolerance, whatever the tile shape, slab order or atomic order.  The epilogue scalars keep that
property (alpha in {1, 1/2, 1/16}, beta in {1, 2}, row_scale in {0, 1, 2}, dropout 0.5 whose keep
scale is exactly 2, integer bias / residual / initial C / Z, RELU and RELU_BWD), and every case
asserts the precondition on the reference side before it looks at the kernel's output.

Every case
  * asserts the kernel the library launched (ops.GEMM_TRACE, i.e. ste_gemm_kernel_name or
    ste_gemm_mx8_kernel at the launch) and, for bf16, the ste_gemm_kernel id;
  * keeps every output (C, C2, C3, colsum, q_out, q_scales) inside a larger buffer filled with a
    sentinel (7.0 / 0x5A): 8 guard rows before and after, pad columns up to the row stride, and the
    gap between batch entries; all sentinels must be intact afterwards (the out-of-bounds check a
    norm cannot make).  Operand pad rows / columns and the split-K workspace hold garbage / NaN, so a
    read past K or of an unwritten slab shows up in the values;
  * on a mismatch reports the count of wrong elements and the first one's (row, col), 256x256 tile,
    16-row epilogue pass and K-tile count.

Which shape reaches which branch of csrc/gemm.hip
  group 1  8-phase kernel under ops.bench_gemm_plan(): K = 64 / 128 / 192 / 320 are nk = 1 (vmcnt(0)
           prologue), 2 and 3 (the tail drains) and 5 (steady state); (8, 8) one partial tile whose
           second 128-column half lies past N; (256, 256) the FULL epilogue; (257, 264) full ->
           partial hand-overs in both directions on one CU each; (300, 261) ragged columns
           (N % 8 != 0, the swapped-operand bf16 epilogue's element-wise tail) with 3 pad columns;
           (520, 136) / (264, 120) a tile whose second half is empty.  Plain fp32 / bf16 run the
           compiled <.., 0, 0> / <.., 512, 0> instantiations (epilogue_8ph, epilogue_bf16s), the two
           generic sets <.., -1, 0> with every run-time feature; batch = 3 with strides.
  group 2  every STE_EPI_SPECS instantiation at (257, 264, 64) (partial tiles only, nk = 1) and at the
           hand-over shape M = 256(CU/2 + 8) - 56, N = 264, K = 192: more tiles than CUs, every second
           tile 8 columns wide, so the persistent second round mixes full -> partial, partial -> full
           and full -> full (EPI_OVL, epilogue_8ph_pre, plain hand-over; `extra`, vm_wait8<W, E>).
  group 3  weight-gradient split-K: S = 2, 4 (reduce<4>), 8 (reduce<8>), 17 (reduce<16> + loop), the
           rem leftover K-tiles of operand_bases, the ragged K % 64 tail (launch_k_tail), the
           workspace cap (3 slabs), and the batched plan at batch 120 (every entry compared).
  group 4  few-tile split-K (splitk_epi_kernel) with every epilogue option, even and odd K-tile
           counts, against its twin without a workspace (torch.equal: same dropout mask).
  group 5  the 128x128 kernel in all four layouts including gemm_bf16_kernel<false, true>, batch 3,
           column sums ordered and atomic, N < 8 with an unaligned row stride.
  group 6  MX-fp8: the single-stage kernel with the generic sets, the persistent kernel's six
           STE_MX8_SPECS at nk = 1, 2, 3 and at the hand-over shape, on hand-built operands whose
           random per-block scales make a scale-select error visible in every tile.
  group 7  ste_mx8_quant at rows = 1, K = 128 (the smallest K the entry accepts), a strided ldx, a zero
           block, amax exactly 448·2^k (scale byte 127 + k, payload 0x7E) and the next bf16 above.
  group 8  ste_gemm_f32 in all four layouts, its split plan with and without a workspace.

Cases the contract of include/ste.h excludes are not generated: a k-major A needs M % 8 == 0 (fp32:
M % 4 == 0), so (129, 136, 72), (65, 68, 20) and (3, 8, 4) run with a k-contiguous A only, and
(136, 136, 72) / (68, 72, 20) give the k-major-A layouts a partial-tile shape instead.

Outputs that cannot be exact (SWISH / GELU and their derivatives): the pre-activation copy C2 is
still bit-exact; activated bf16 outputs use _assert_bf16_close against the fp64 activation of the
exact v; fp32 ones |out - ref| <= 1e-5·max(1, |ref|) per element; an [hi | lo] pair
|C + C3 - ref| <= 1e-5·max(1, |ref|) + 2^-17·|ref| (v_kernel - (C + C3) is one bf16 rounding of the
low half, itself <= 2^-9·|v|: 2^-18·|v|); a column sum of such values sum_m 1e-5·max(1, |ref_m|),
the per-element bound summed.

The MX-fp8 copy q_out: the kernel quantises its fp32 value, the reference restates the quantiser on
the fp64 value.  Scale bytes within +-1 (the two amax can straddle 448·2^k).  e4m3 has 3 mantissa
bits: a value y with 2^j <= |y| < 2^(j+1) has spacing 2^(j-3), the subnormal spacing is 2^-9, so
after scaling by 2^e an element x lies within one step max(2^(floor(log2|x|) - 3), 2^(e - 9)) of its
code (half a step of rounding plus the fp32 value's own error); a scale one higher doubles the step.

Measured on an MI355X (256 CUs): the file's 305 cases take 7.6 s; the slowest is the first (0.43 s:
it loads the library), then the MX hand-over cases at M = 34,760 (0.27 s); every other case is
under 0.2 s.  Non-exact outputs, as the largest share of their bound over all cases (each case
prints its own): activated fp32 C (w2v_conv_last) 0.009 of 1e-5·max(1, |ref|); activated bf16 C / C3
0.81 - 0.99 of 2^-8·|ref| + 1e-5·max|ref| (half a bf16 ulp is 2^-8·|ref| just above a power of two,
so a correct output comes close); [hi | lo] pairs C + C3 0.31 - 0.42; column sums of activated values
<= 0.004; q_out 0.500 of one e4m3 step (a rounding tie) with every scale byte equal to the restated
quantiser's.  The tests found no kernel bug: all cases pass on the kernels as they are."""
import contextlib
import ctypes

import pytest
import torch

from gemm_exact_cases import (BY_ID, INEXACT_ACTS, RELU, RELU_BWD, case_m, epi_of, expected_kernel, ids, int_tensor,
                              logical_operands, out_ld, plan_args, ws_floats)
from test_gemm_specs_gpu import SWISH_BWD, GELU_BWD, _act64, _actd64, drop_scale_t
from test_kernels_gpu import _mx8_dequant
from test_w2v2_kernels_gpu import _assert_bf16_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
SENT, SENT8 = 7.0, 0x5A
TWO24 = float(1 << 24)


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def CU():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guard:
    """`batch` [rows, cols] windows (row stride ld, `gap` rows between batch entries) inside a buffer
    filled with a sentinel, 8 guard rows before and after."""

    def __init__(self, rows, cols, dtype, batch=1, ld=None, gap=3):
        self.rows, self.cols, self.batch = rows, cols, batch
        self.ld = ld if ld else (cols + 15) // 16 * 16 + 16
        self.pitch = rows + (gap if batch > 1 else 0)
        self.fill = SENT8 if dtype == U8 else SENT
        self.buf = torch.full((16 + batch * self.pitch, self.ld), self.fill, dtype=dtype, device=DEV)

    @property
    def stride(self):
        return self.pitch * self.ld if self.batch > 1 else 0

    def view(self, b=0):
        r0 = 8 + b * self.pitch
        return self.buf[r0:r0 + self.rows, :self.cols]

    def get(self):
        return torch.stack([self.view(b) for b in range(self.batch)])

    def set(self, vals):
        for b in range(self.batch):
            self.view(b).copy_(vals[b])
        return self.get().double()   # what the buffer now holds (rounded to its dtype)

    def check(self, what):
        t = self.buf.clone()
        for b in range(self.batch):
            r0 = 8 + b * self.pitch
            t[r0:r0 + self.rows, :self.cols] = self.fill
        bad = t != self.fill
        if bad.any():
            r, col = (int(x) for x in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} sentinel(s) overwritten; first at buffer row {r} (output "
                                 f"row {r - 8}), column {col} of {self.cols} valid / row stride {self.ld}")


def _where(c, K, bad):
    b, r, col = (int(x) for x in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} wrong; first at batch {b} (row {r}, col {col}): 256x256 tile "
            f"({r // 256}, {col // 256}), wave row {(r % 256) // 128}, 16-row pass {(r % 128) // 16}, column half "
            f"{(col % 256) // 128}, {K // 64} K-tiles (K = {K})")


def _assert_exact(c, what, got, ref64, lo=False):
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), f"{c.id} {what}: the reference itself is not an fp32 value"
    if lo:
        want = (r32 - r32.bfloat16().float()).bfloat16()
    else:
        want = r32.to(got.dtype)
    if torch.equal(got, want):
        return
    bad = got != want
    b, r, col = (int(x) for x in bad.nonzero()[0])
    raise AssertionError(f"{c.id} {what}: {_where(c, c.K, bad)}: got {got[b, r, col].item()}, want "
                         f"{want[b, r, col].item()}")


def _assert_f32_close(c, what, got, ref64, extra=None):
    """|got - ref| <= 1e-5·max(1, |ref|) (+ extra) per element."""
    bound = 1e-5 * ref64.abs().clamp_min(1.0)
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref64).abs()
    print(f"[gemm exact] {c.id} {what}: max |err| / bound = {(err / bound).max().item():.3f}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{c.id} {what}: {_where(c, c.K, bad)}"


def _bf16_close(c, what, got, ref64):
    """_assert_bf16_close (|out - ref| <= 2^-8·|ref| + 1e-5·max|ref|), printing the measured share of the bound."""
    bound = 2.0 ** -8 * ref64.abs() + 1e-5 * ref64.abs().max()
    print(f"[gemm exact] {c.id} {what}: max |err| / bound = {((got.double() - ref64).abs() / bound).max().item():.3f}")
    _assert_bf16_close(got, ref64, f"{c.id} {what}")


def _phys(x64, kc, dtype, pad):
    """[batch, rows, K] values -> the operand as the kernel reads it (k-contiguous [rows, K] or k-major
    [K, rows] windows of a larger buffer whose pad rows / columns hold 3.0) and its batch stride."""
    nb, rows, K = x64.shape
    src = x64 if kc else x64.transpose(1, 2)
    buf = torch.full((nb, src.shape[1] + 1, src.shape[2] + pad), 3.0, dtype=dtype, device=DEV)
    buf[:, :src.shape[1], :src.shape[2]] = src
    v = buf[:, :src.shape[1], :src.shape[2]]
    return (v if nb > 1 else v[0]), (buf.stride(0) if nb > 1 else 0)


def _phys_mx(q, s, K):
    """e4m3 payload integers [rows, K] -> bytes in a [rows, K + 16] buffer (pad bytes 0x38 = 1.0)."""
    buf = torch.full((q.shape[0] + 1, K + 16), 0x38, dtype=U8, device=DEV)
    buf[:q.shape[0], :K] = q.to(torch.float8_e4m3fn).view(U8)
    assert torch.equal(buf[:q.shape[0], :K].view(torch.float8_e4m3fn).float(), q)   # exact in e4m3
    return buf[:q.shape[0], :K], s.contiguous()


def _check_q8(c, ref, q, qs):
    """The MX-fp8 copy against the quantiser restated on the reference value (module docstring)."""
    M, N = ref.shape
    amax = ref.view(M, N // 32, 32).abs().amax(-1).cpu()
    m, e2 = torch.frexp(amax / 448.0)
    e_ref = torch.where(amax > 0, torch.where(m == 0.5, e2 - 1, e2), torch.full_like(e2, -127)).clamp(-127, 127)
    e_ref = e_ref.to(DEV).long()
    sc = qs.long() - 127
    d = (sc - e_ref).abs().max().item()
    assert d <= 1, f"{c.id} q_scales: scale byte {d} away from the restated quantiser"
    e_el = e_ref.repeat_interleave(32, dim=1).double()
    lg = torch.floor(torch.log2(ref.abs().clamp_min(1e-300)))
    step = torch.maximum(torch.pow(2.0, lg - 3), torch.pow(2.0, e_el - 9))
    bound = step * torch.where(sc > e_ref, 2.0, 1.0).repeat_interleave(32, dim=1)
    err = (_mx8_dequant(q, qs) - ref).abs()
    print(f"[gemm exact] {c.id} q_out: max |err| / step = {(err / bound).max().item():.3f}, scale bytes off by "
          f"<= {d}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{c.id} q_out: {_where(c, c.K, bad[None])}"


def run_case(ops, c, CU, twin=False):
    """Run one case, check every output, and return {name: tensor} of what the call wrote.
    twin: the same inputs without the split-K workspace (default plan)."""
    from speech_transcript_embeddings_amd import _lib
    e = epi_of(c.epi)
    M, N, K, nb = case_m(c, CU), c.N, c.K, c.batch
    f32k, mxk = c.kind == "f32", c.kind == "mx8"
    g, a64, b64, mx = logical_operands(c, CU, DEV)
    alpha, beta, act = e.get("alpha", 1.0), e.get("beta", 0.0), e.get("act", 0)
    unit = min(1.0, alpha) * (0.25 if mxk else 1.0)   # every value below is a multiple of it
    acc = torch.bmm(a64, b64.transpose(1, 2))
    absacc = torch.bmm(a64.abs(), b64.abs().transpose(1, 2)).amax().item()
    assert absacc / unit < TWO24, f"{c.id}: precondition: max sum|a||b| = {absacc} at unit {unit}"

    # ---- operands
    kw = dict(a_kc=c.a_kc, b_kc=c.b_kc, M=M, N=N, K=K, alpha=alpha, beta=beta, act=act, batch=nb)
    if mxk:
        qa, sa, qb, sb = mx
        A, sa = _phys_mx(qa, sa, K)
        B, sb = _phys_mx(qb, sb, K)
    else:
        A, kw["stride_a"] = _phys(a64, c.a_kc, F32 if f32k else BF16, 8)
        B, kw["stride_b"] = _phys(b64, c.b_kc, F32 if f32k else BF16, 8)

    # ---- epilogue operands and guarded outputs
    ld = out_ld(c)
    guards = {}
    Cg = guards["C"] = Guard(M, N, BF16 if c.out_bf16 else F32, nb, ld)
    kw["stride_c"] = Cg.stride
    c0 = Cg.set(int_tensor(g, (nb, M, N), 50, DEV)) if beta else None
    bias = rs = z = r = cs0 = ds = None
    if e.get("bias"):
        bias = kw["bias"] = int_tensor(g, (N,), 30, DEV)
    if e.get("c2") and 1 <= act <= 4:
        guards["C2"] = Guard(M, N, F32 if f32k else BF16, nb, ld)
        kw["pre_out"] = guards["C2"].view()
    if e.get("c3"):
        guards["C3"] = Guard(M, N, BF16, nb, ld)
        kw["out_bf16_copy"], kw["copy_lo"] = guards["C3"].view(), e["c3"] == "lo"
    if act >= 11:
        Zg = Guard(M, N, F32 if f32k else BF16, nb, ld)   # Z shares C's batch stride (offC)
        z = Zg.set(int_tensor(g, (nb, M, N), 4, DEV))
        kw["z"] = Zg.view()
    if e.get("drop"):
        kw["drop_p"], kw["seed"], kw["drop_ld"] = 0.5, c.seed ^ 0x5EED0000, c.drop_ld
        ds = drop_scale_t(kw["seed"], 0.5, M, N, c.drop_ld or N)
        assert set(ds.unique().tolist()) <= {0.0, 2.0}
    if e.get("rs"):
        rs = kw["row_scale"] = torch.randint(0, 3, (M,), generator=g, device=DEV).float()
    if e.get("colsum"):
        guards["colsum"] = Guard(nb, N, F32, 1, ld=N)
        cs0 = int_tensor(g, (nb, N), 5, DEV)
        guards["colsum"].view().copy_(cs0)
        kw["colsum"] = guards["colsum"].view()
    if e.get("r"):
        Rg = Guard(M, N, BF16 if e["r"] == "bf16" else F32, nb, ld + 16, gap=5)
        r = Rg.set(int_tensor(g, (nb, M, N), 1000, DEV))
        kw["residual"], kw["stride_r"] = Rg.view(), Rg.stride
    q8 = None
    if e.get("q8"):
        guards["q_out"] = Guard(M, N, U8, 1, ld=N)
        guards["q_scales"] = Guard(M, N // 32, U8, 1, ld=N // 32)
        q8 = (guards["q_out"].view(), guards["q_scales"].view())
    if mxk:
        kw["mx8"] = (sa, sb) if q8 is None else (sa, sb, q8)
    n_ws = 0 if twin else ws_floats(c, CU)
    if n_ws:   # NaN: an unwritten slab that the reduction reads shows in the result
        kw["ws"] = torch.full((n_ws,), float("nan"), device=DEV)
    kw["out"] = False if e.get("noc") else Cg.view()   # NOC: the guarded C is never handed to the call
    if e.get("noc"):
        kw["out_bf16"] = c.out_bf16

    # ---- the reference (include/ste.h order), with the exactness precondition at every stage
    peak = [0.0]

    def track(v):
        peak[0] = max(peak[0], v.abs().amax().item())
        return v
    ref = {}
    v = acc
    if bias is not None:
        v = v + bias.double()
    v = track(v * alpha)
    inexact = act in INEXACT_ACTS
    if "C2" in guards:
        ref["C2"] = v
    if act == RELU:
        v = v.clamp_min(0.0)
    elif act == RELU_BWD:
        v = v * (z > 0).double()
    elif act in (SWISH_BWD, GELU_BWD):
        v = v * _actd64(z, act)
    elif act:
        v = _act64(v, act)
    if ds is not None:
        v = v * ds
    if rs is not None:
        v = v * rs.double()[None, :, None]
    if not inexact:
        track(v)
    if cs0 is not None:
        ref["colsum"] = cs0.double() + v.sum(1)
        if inexact:
            cs_bound = 1e-5 * v.abs().clamp_min(1.0).sum(1)
        else:
            assert v.abs().sum(1).amax().item() / unit < TWO24, f"{c.id}: precondition: column sums"
    if r is not None:
        v = v + r
    if c0 is not None:
        v = v + beta * c0
    if not inexact:
        track(v)
    assert peak[0] / unit < TWO24, f"{c.id}: precondition: |v| up to {peak[0]} at unit {unit}"
    ref["C"] = v

    # ---- the launch
    twin_name = "gemm_f32_kernel" if f32k else f"gemm_bf16_kernel<{str(c.a_kc).lower()}, {str(c.b_kc).lower()}>"
    want_id, want = (None, twin_name) if twin else expected_kernel(c)
    atomic = e.get("colsum") == "atomic"
    prev_atomic = ops.ATOMIC_SUMS
    with (ops.bench_gemm_plan() if c.low else contextlib.nullcontext()):
        if want_id is not None and not twin:
            got_id = int(_lib.fn("ste_gemm_kernel")(ctypes.byref(plan_args(c, CU))))
            assert got_id == want_id, f"{c.id}: ste_gemm_kernel plans {got_id}, the case needs {want_id}"
        ops.GEMM_TRACE = []
        try:
            if atomic:
                ops.ATOMIC_SUMS = True
            ops.gemm(A, B, **kw)
            torch.cuda.synchronize()
            names = [t[0] for t in ops.GEMM_TRACE]
        finally:
            ops.GEMM_TRACE = None
            ops.ATOMIC_SUMS = prev_atomic
    assert names == [want], f"{c.id}: launched {names}, the case needs {want}"

    # ---- outputs
    got = {k: gd.get() for k, gd in guards.items() if k not in ("colsum", "q_out", "q_scales")}
    if "C2" in guards:
        _assert_exact(c, "C2", got["C2"], ref["C2"])
    if not inexact:
        if not e.get("noc"):
            _assert_exact(c, "C", got["C"], ref["C"])
        if "C3" in guards:
            _assert_exact(c, "C3", got["C3"], ref["C"], lo=e["c3"] == "lo")
        if "colsum" in guards:
            got["colsum"] = guards["colsum"].view().clone()
            _assert_exact(c, "colsum", got["colsum"][None], ref["colsum"][None])
    else:
        if e.get("noc"):
            pass
        elif c.out_bf16:
            _bf16_close(c, "C", got["C"], ref["C"])
        else:
            _assert_f32_close(c, "C", got["C"], ref["C"])
        if "C3" in guards and e["c3"] == "lo":
            _assert_f32_close(c, "C + C3", got["C"].double() + got["C3"].double(), ref["C"],
                              extra=2.0 ** -17 * ref["C"].abs())
        elif "C3" in guards:
            _bf16_close(c, "C3", got["C3"], ref["C"])
        if "colsum" in guards:
            err = (guards["colsum"].view().double() - ref["colsum"]).abs()
            print(f"[gemm exact] {c.id} colsum: max |err| / bound = {(err / cs_bound).max().item():.3f}")
            assert bool((err <= cs_bound).all()), f"{c.id} colsum: {int((err > cs_bound).sum())} columns out of bound"
    if q8 is not None:
        _check_q8(c, ref["C"][0], *q8)
        got["q_out"], got["q_scales"] = q8[0].clone(), q8[1].clone()
    for k, gd in guards.items():
        gd.check(f"{c.id} {k}")
    if e.get("noc"):
        assert bool((Cg.buf == SENT).all()), f"{c.id}: a launch without C wrote to the C image"
    return got


def _run(ops, CU, cid):
    return run_case(ops, BY_ID[cid], CU)


@pytest.mark.parametrize("cid", ids(1))
def test_8ph_ktiles_and_edges(ops, CU, cid):
    _run(ops, CU, cid)


@pytest.mark.parametrize("cid", ids(2))
def test_8ph_every_epilogue_spec(ops, CU, cid):
    c = BY_ID[cid]
    if c.M == 0:   # the hand-over shape: a second persistent round with full and partial tiles
        from speech_transcript_embeddings_amd import _lib
        num_m, num_n = (case_m(c, CU) + 255) // 256, 2
        assert num_m * num_n > CU
        tm, tn = ctypes.c_int(), ctypes.c_int()
        kinds = set()
        for t in range(CU, num_m * num_n):
            assert _lib.fn("ste_gemm_tile_map")(t, num_m, num_n, ctypes.byref(tm), ctypes.byref(tn)) == 0
            kinds.add((tm.value + 1) * 256 <= case_m(c, CU) and (tn.value + 1) * 256 <= c.N)
        assert kinds == {True, False}, kinds
    _run(ops, CU, cid)


@pytest.mark.parametrize("cid", ids(3))
def test_weight_gradient_split_k(ops, CU, cid):
    _run(ops, CU, cid)


@pytest.mark.parametrize("cid", ids(4))
def test_few_tile_split_k_twin(ops, CU, cid):
    c = BY_ID[cid]
    a = run_case(ops, c, CU)
    b = run_case(ops, c, CU, twin=True)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (cid, k)


@pytest.mark.parametrize("cid", ids(5))
def test_small_kernel_layouts(ops, CU, cid):
    _run(ops, CU, cid)


@pytest.mark.parametrize("cid", ids(6))
def test_mx8(ops, CU, cid):
    _run(ops, CU, cid)


@pytest.mark.parametrize("cid", ids(8))
def test_gemm_f32(ops, CU, cid):
    c = BY_ID[cid]
    a = run_case(ops, c, CU)
    if c.ws:   # the split plan and the single launch: bit-identical (both equal fp64)
        b = run_case(ops, c, CU, twin=True)
        assert torch.equal(a["C"], b["C"]), cid


# ------------------------------------------------------------------ group 7: ste_mx8_quant
def _quant_ref(x):
    """ste_mx8_quant restated: e = ceil(log2(amax / 448)) per 32-block through frexp (exact),
    q = e4m3(x / 2^e); zero blocks get scale byte 0."""
    rows, K = x.shape
    xb = x.double().view(rows, K // 32, 32)
    amax = xb.abs().amax(-1).cpu()
    m, e2 = torch.frexp(amax / 448.0)
    e = torch.where(amax > 0, torch.where(m == 0.5, e2 - 1, e2), torch.full_like(e2, -127)).clamp(-127, 127).to(DEV)
    q = (xb / torch.pow(2.0, e.double()).unsqueeze(-1)).view(rows, K).float().to(torch.float8_e4m3fn).view(U8)
    return q, (e + 127).to(U8)


def _quant(ops, x):
    """ops.mx8_quant into sentinel-guarded q / scales."""
    rows, K = x.shape
    qg, sg = Guard(rows, K, U8, 1, ld=K), Guard(rows, K // 32, U8, 1, ld=K // 32)
    ops.mx8_quant(x, qg.view(), sg.view())
    torch.cuda.synchronize()
    qg.check("q")
    sg.check("scales")
    return qg.view().clone(), sg.view().clone()


@pytest.mark.parametrize("rows,K,ldx", [(1, 128, 128), (1, 128, 136), (5, 128, 200), (300, 384, 392)])
def test_mx8_quant_shapes(ops, rows, K, ldx):
    """One row, a strided ldx, several rows per 256-thread block and more than one block, with a zero
    block (scale byte 0, payload 0): bit-equal to the restated quantiser.  (K = 128 is the smallest
    K ste_mx8_quant accepts; a 32-element K is STE_ERR_SHAPE.)"""
    g = torch.Generator(device=DEV).manual_seed(rows * 1000 + ldx)
    buf = torch.full((rows, ldx), 3.0, device=DEV).bfloat16()
    vals = torch.randn(rows, K, device=DEV, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, 1), generator=g,
                                                                                     device=DEV).float())
    buf[:, :K] = vals.bfloat16()
    buf[rows // 2, 32:64] = 0
    x = buf[:, :K]
    q, s = _quant(ops, x)
    qr, sr = _quant_ref(x)
    assert torch.equal(s, sr), (s.long() - sr.long()).abs().max().item()
    assert int(s[rows // 2, 1]) == 0 and not q[rows // 2, 32:64].any()
    if not torch.equal(q, qr):
        i, j = (int(t) for t in (q != qr).nonzero()[0])
        raise AssertionError(f"{int((q != qr).sum())} payload bytes differ; first at ({i}, {j}): x = {x[i, j].item()}, "
                             f"scale byte {int(s[i, j // 32])}, got {int(q[i, j]):#x}, want {int(qr[i, j]):#x}")


@pytest.mark.parametrize("k", [-3, 0, 5])
def test_mx8_quant_amax_at_448_times_power_of_two(ops, k):
    """amax exactly 448·2^k: the scale byte is exactly 127 + k and the max element's payload 0x7E
    (448, the largest e4m3); the next bf16 above it moves the scale to 127 + k + 1.  This is where a
    log2 one ulp high would move the scale."""
    g = torch.Generator(device=DEV).manual_seed(77 + k)
    top = 448.0 * 2.0 ** k
    up = 450.0 * 2.0 ** k   # 448 = 1.75·2^8: bf16 (8 significant bits) is spaced 2·2^k there
    assert torch.tensor(up).bfloat16().item() == up and torch.tensor((top + up) / 2).bfloat16().item() in (top, up)
    x = ((torch.rand(4, 128, device=DEV, generator=g) - 0.5) * top).bfloat16()   # |x| <= top / 2
    x[0, 5], x[1, 40], x[2, 95], x[3, 127] = top, -top, up, -up
    q, s = _quant(ops, x)
    assert int(s[0, 0]) == 127 + k and int(q[0, 5]) == 0x7E
    assert int(s[1, 1]) == 127 + k and int(q[1, 40]) == 0xFE
    assert int(s[2, 2]) == 127 + k + 1 and int(s[3, 3]) == 127 + k + 1
    qr, sr = _quant_ref(x)
    assert torch.equal(s, sr) and torch.equal(q, qr)


def test_mx8_quant_rejects_k32(ops):
    from speech_transcript_embeddings_amd._lib import SteError
    x = torch.zeros(1, 32, device=DEV).bfloat16()
    with pytest.raises(SteError):
        ops.mx8_quant(x)
