"""Case tables and host-side helpers of the exact-arithmetic GEMM tests (test_gemm_exact_gpu.py runs
the cases on the GPU, test_gemm_exact_cpu.py checks their plans and the reference on the CPU).

A case names a shape, an operand layout, an epilogue set and the kernel path the library must plan
for it.  Operands are small integers, so every product and partial sum is an integer below 2^24 and
fp32 accumulation is exact in any order (see the GPU file's docstring)."""
import zlib
from dataclasses import dataclass

import torch

from test_gemm_specs_gpu import (SPECS, COMPILED, SWISH, GELU, SWISH_BWD, GELU_BWD, EF_BIAS, EF_C2, EF_Z, EF_DROP,
                                 EF_RS, EF_COLSUM, EF_R, EF_BETA, EF_CBF16, EF_C3)

RELU, RELU_BWD = 4, 14
EF_RBF16 = 128
INEXACT_ACTS = (SWISH, GELU, SWISH_BWD, GELU_BWD)
CU_DEFAULT = 256          # CUs of an MI355X: what the host-only plan queries assume without a device
HANDOVER = 0              # Case.M placeholder: 256·(CU//2 + 8) − 56 rows (see handover_m)

# ------------------------------------------------------------------ epilogue sets
# alpha in {1, 0.5, 2^-4}, beta in {1, 2}, row_scale in {0, 1, 2}, drop_p = 0.5 (keep scale exactly 2):
# every epilogue value stays a multiple of alpha below 2^24·alpha.
EPIS = {
    "plain": {},
    # the two generic (EF = -1) sets: between them every run-time epilogue feature
    "gen_fwd": dict(bias=1, act=RELU, c2=1, drop=1, rs=1, colsum="ws", r="f32", beta=2.0, alpha=0.5, c3="plain"),
    "gen_bwd": dict(bias=1, act=RELU_BWD, drop=1, rs=1, colsum="atomic", r="bf16", beta=1.0, alpha=0.5, c3="lo"),
    # the same without column sums (the few-tile split-K plan excludes them)
    "gen_fwd_nocs": dict(bias=1, act=RELU, c2=1, drop=1, rs=1, r="f32", beta=2.0, alpha=0.5, c3="plain"),
    "gen_bwd_nocs": dict(bias=1, act=RELU_BWD, drop=1, rs=1, r="bf16", beta=1.0, alpha=0.5, c3="lo"),
    # weight gradients: alpha/beta only
    "dw": dict(alpha=0.5, beta=1.0),
    # column sums alone, through the workspace and through atomics
    "cs_ws": dict(colsum="ws"),
    "cs_atomic": dict(colsum="atomic"),
    # MX-fp8 compile-time epilogues (STE_MX8_SPECS, in its order)
    "mx_bias_bf16": dict(bias=1),
    "mx_bf16": dict(),
    "mx_bias_r": dict(bias=1, r="f32"),
    "mx_ffn_in_q8": dict(bias=1, act=SWISH, c2=1, q8=1, alpha=2.0 ** -4),
    "mx_ffn_in_q8_noc": dict(bias=1, act=SWISH, c2=1, q8=1, noc=1, alpha=2.0 ** -4),
    "mx_dz": dict(act=SWISH_BWD),
}
MX_SPEC_OUT_BF16 = {"mx_bias_bf16": True, "mx_bf16": True, "mx_bias_r": False, "mx_ffn_in_q8": True,
                    "mx_ffn_in_q8_noc": True, "mx_dz": True}


def _spec_epi(name):
    """The epilogue set of a STE_EPI_SPECS entry (flags and activation from test_gemm_specs_gpu.SPECS)."""
    _, _, ef, act, _, _, _, extra = SPECS[name]
    e = dict(act=act)
    if ef & EF_BIAS:
        e["bias"] = 1
    if ef & EF_C2:
        e["c2"] = 1
    if ef & EF_C3:
        e["c3"] = "lo" if extra == "lo" else "plain"
    if ef & EF_DROP:
        e["drop"] = 1
    if ef & EF_RS:
        e["rs"] = 1
    if ef & EF_COLSUM:
        e["colsum"] = "ws"
    if ef & EF_R:
        e["r"] = "f32"
    if ef & EF_BETA:
        e["beta"] = 2.0
    # SWISH / GELU outputs: |v| below about 16 so that the activation is compared where it bends
    e["alpha"] = 0.5 if extra == "alpha" else (2.0 ** -4 if act in (SWISH, GELU) else 1.0)
    return e


def epi_of(name):
    return EPIS[name] if name in EPIS else _spec_epi(name[5:])   # "spec:<SPECS key>"


def epi_flags(e, out_bf16):
    """epi_flags() of csrc/gemm.hip restated: the feature mask a launch is matched with."""
    act = e.get("act", 0)
    fwd, bwd = 1 <= act <= 4, act >= 11
    f = 0
    f |= EF_BIAS if e.get("bias") else 0
    f |= EF_C2 if e.get("c2") and fwd else 0
    f |= EF_Z if bwd else 0
    f |= EF_DROP if e.get("drop") else 0
    f |= EF_RS if e.get("rs") else 0
    f |= EF_COLSUM if e.get("colsum") else 0
    f |= (EF_R | (EF_RBF16 if e["r"] == "bf16" else 0)) if e.get("r") else 0
    f |= EF_BETA if e.get("beta") else 0
    f |= EF_CBF16 if out_bf16 else 0
    f |= EF_C3 if e.get("c3") else 0
    return f


_COMPILED_KEYS = {(SPECS[k][0], SPECS[k][1], SPECS[k][2], SPECS[k][3]) for k in COMPILED} | {(False, False, 0, 0)}


@dataclass(frozen=True)
class Case:
    id: str
    group: int
    path: str              # small | ph8 | dw | bdw | few | f32 | mx1 | mx8ph: the kernel path that must be planned
    M: int
    N: int
    K: int
    a_kc: bool = True
    b_kc: bool = True
    out_bf16: bool = False
    epi: str = "plain"
    batch: int = 1
    vals: int = 4          # operands are integers in [-vals, vals]
    ld: int = 0            # row stride of the outputs (0: next multiple of 16 past N, plus 16)
    ws: str = ""           # "" | dw (ample) | dw3 (exactly three slabs) | few | f32split
    low: bool = False      # run under ops.bench_gemm_plan() (both plan thresholds at one tile)
    drop_ld: int = 0       # dropout row stride (0: N)
    kind: str = "bf16"     # bf16 | f32 | mx8

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


def handover_m(cu):
    """Rows of the hand-over shape: 2·(cu//2 + 8) > cu tiles at two tile columns, the last tile row partial."""
    return 256 * (cu // 2 + 8) - 56


def case_m(c, cu):
    return handover_m(cu) if c.M == HANDOVER else c.M


def out_ld(c):
    return c.ld if c.ld else (c.N + 15) // 16 * 16 + 16


def ws_floats(c, cu):
    M = case_m(c, cu)
    return {"": 0, "dw": 8 << 20, "dw3": 3 * M * c.N, "few": 2 * M * c.N, "f32split": 1 << 20}[c.ws]


def expected_kernel(c):
    """(ste_gemm_kernel id or None, kernel name) the case must run on."""
    ak, bk = str(c.a_kc).lower(), str(c.b_kc).lower()
    variant = (0 if c.a_kc else 2) + (0 if c.b_kc else 1)
    if c.path == "small":
        return variant, f"gemm_bf16_kernel<{ak}, {bk}>"
    if c.path in ("dw", "few"):
        return 12 + variant, f"gemm_8ph_kernel<{ak}, {bk}, 0, 0>"
    if c.path in ("ph8", "bdw"):
        e = epi_of(c.epi)
        key = (c.a_kc, c.b_kc, epi_flags(e, c.out_bf16), e.get("act", 0))
        ef, act = (key[2], key[3]) if key in _COMPILED_KEYS else (-1, 0)
        return 8 + variant, f"gemm_8ph_kernel<{ak}, {bk}, {ef}, {act}>"
    if c.path == "f32":
        return None, "gemm_f32_kernel"
    return None, "gemm_8ph_kernel<mx8>" if c.path == "mx8ph" else "gemm_mx8_kernel"


def plan_args(c, cu):
    """ste_gemm_args of the case with placeholder pointers: what the host-only plan queries read."""
    from speech_transcript_embeddings_amd import _lib
    e, M, ld = epi_of(c.epi), case_m(c, cu), out_ld(c)
    a = _lib.GemmArgs()
    a.M, a.N, a.K, a.batch = M, c.N, c.K, c.batch
    a.A, a.B, a.a_kc, a.b_kc = 16, 16, int(c.a_kc), int(c.b_kc)
    pad = 16 if c.kind == "mx8" else 8
    a.lda = (c.K if c.a_kc else M) + pad
    a.ldb = (c.K if c.b_kc else c.N) + pad
    a.C, a.ldc, a.c_bf16 = (None if e.get("noc") else 16), ld, int(c.out_bf16)
    act = e.get("act", 0)
    if e.get("c2"):
        a.C2, a.ldc2 = 16, ld
    if e.get("c3"):
        a.C3, a.ldc3, a.c3_lo = 16, ld, int(e["c3"] == "lo")
    if e.get("bias"):
        a.bias = 16
    if e.get("r"):
        a.R, a.ldr, a.r_bf16 = 16, ld, int(e["r"] == "bf16")
    if act >= 11:
        a.Z, a.ldz = 16, ld
    if e.get("colsum"):
        a.colsum = 16
    if e.get("rs"):
        a.row_scale = 16
    a.alpha, a.beta, a.act = e.get("alpha", 1.0), e.get("beta", 0.0), act
    a.drop_p = 0.5 if e.get("drop") else 0.0
    n = ws_floats(c, cu)
    if n:
        a.ws, a.ws_bytes = 16, 4 * n
    elif e.get("colsum") == "ws" and c.kind != "mx8":
        a.ws, a.ws_bytes = 16, 4 << 20
    return a


def int_tensor(g, shape, lim, device, dtype=torch.float32):
    """Integers in [-lim, lim] from the case's generator."""
    return torch.randint(-lim, lim + 1, shape, generator=g, device=device).to(dtype)


def logical_operands(c, cu, device):
    """(A [batch, M, K], B [batch, N, K]) as fp64 — for MX-fp8: integers in [-8, 8] times a random
    per-32-block scale in {2^-1, 1, 2} (also returned: the integer payloads and the scale bytes)."""
    g = torch.Generator(device=device).manual_seed(c.seed)
    M = case_m(c, cu)
    if c.kind == "mx8":
        qa, qb = int_tensor(g, (M, c.K), 8, device), int_tensor(g, (c.N, c.K), 8, device)
        sa = torch.randint(126, 129, (M, c.K // 32), generator=g, device=device).to(torch.uint8)
        sb = torch.randint(126, 129, (c.N, c.K // 32), generator=g, device=device).to(torch.uint8)

        def deq(q, s):
            return q.double() * torch.pow(2.0, s.double().repeat_interleave(32, dim=1) - 127)
        return g, deq(qa, sa)[None], deq(qb, sb)[None], (qa, sa, qb, sb)
    a = int_tensor(g, (c.batch, M, c.K), c.vals, device).double()
    b = int_tensor(g, (c.batch, c.N, c.K), c.vals, device).double()
    return g, a, b, None


# ------------------------------------------------------------------ the case tables
def _cases():
    out = []

    def add(**kw):
        out.append(Case(**kw))

    # group 1: the 8-phase bf16 kernel, K-tile counts 1, 2, 3, 5 x tile edges
    shapes1 = [(8, 8, 0), (256, 256, 0), (257, 264, 0), (300, 261, 264), (520, 136, 0), (264, 120, 0)]
    for K in (64, 128, 192, 320):
        for M, N, ld in shapes1:
            for b_kc in (True, False):
                if not b_kc and N % 8:
                    continue
                lay = "kk" if b_kc else "km"
                for bf in (False, True):
                    add(id=f"g1-{M}x{N}x{K}-{lay}-{'bf16' if bf else 'f32'}-plain", group=1, path="ph8", M=M, N=N, K=K,
                        b_kc=b_kc, out_bf16=bf, ld=ld, low=True)
            add(id=f"g1-{M}x{N}x{K}-kk-f32-gen_fwd", group=1, path="ph8", M=M, N=N, K=K, epi="gen_fwd", ld=ld, low=True)
            km = N % 8 == 0
            add(id=f"g1-{M}x{N}x{K}-{'km' if km else 'kk'}-bf16-gen_bwd", group=1, path="ph8", M=M, N=N, K=K,
                b_kc=not km, out_bf16=True, epi="gen_bwd", ld=ld, low=True)
    add(id="g1-257x264x192-kk-f32-gen_fwd-batch3", group=1, path="ph8", M=257, N=264, K=192, epi="gen_fwd", batch=3,
        drop_ld=269, low=True)
    add(id="g1-264x120x64-km-bf16-gen_bwd-batch3", group=1, path="ph8", M=264, N=120, K=64, b_kc=False, out_bf16=True,
        epi="gen_bwd", batch=3, drop_ld=125, low=True)
    add(id="g1-300x261x128-kk-bf16-plain-batch3", group=1, path="ph8", M=300, N=261, K=128, out_bf16=True, batch=3,
        ld=264, low=True)

    # group 2: every STE_EPI_SPECS entry (and the two generic cases of SPECS) at a partial-tile shape
    # and at the hand-over shape
    for name, (a_kc, b_kc, ef, act, _, _, _, extra) in SPECS.items():
        for tag, M, K, vals in (("a", 257, 64, 4), ("b", HANDOVER, 192, 1)):
            add(id=f"g2{tag}-{name}", group=2, path="ph8", M=M, N=264, K=K, a_kc=a_kc, b_kc=b_kc,
                out_bf16=bool(ef & EF_CBF16), epi="spec:" + name, vals=vals, low=True)

    # group 3: weight-gradient split-K (both operands k-major)
    for M, N, K, ws in ((8, 8, 1024, "dw"), (264, 520, 1096, "dw"), (256, 256, 64 * 35 + 24, "dw"),
                        (256, 256, 64 * 67, "dw"), (256, 256, 64 * 141, "dw"), (264, 520, 64 * 67, "dw3")):
        add(id=f"g3-{M}x{N}x{K}-{ws}", group=3, path="dw", M=M, N=N, K=K, a_kc=False, b_kc=False, epi="dw", ws=ws)
    add(id="g3-256x512x1064-batch120", group=3, path="bdw", M=256, N=512, K=1064, a_kc=False, b_kc=False, epi="dw",
        batch=120)

    # group 4: few-tile split-K with every epilogue option (each run has a twin without ws)
    for K in (2560, 64 * 41):
        add(id=f"g4-2048x264x{K}-gen_fwd", group=4, path="few", M=2048, N=264, K=K, epi="gen_fwd_nocs", ws="few")
        add(id=f"g4-2048x264x{K}-gen_bwd", group=4, path="few", M=2048, N=264, K=K, out_bf16=True, epi="gen_bwd_nocs",
            ws="few")

    # group 5: the 128x128 kernel, all four layouts (a k-major operand needs its M or N % 8 == 0)
    for M, N, K in ((129, 136, 72), (8, 8, 8), (128, 128, 64), (136, 261, 200), (136, 136, 72)):
        for a_kc in (True, False):
            for b_kc in (True, False):
                if (not a_kc and M % 8) or (not b_kc and N % 8):
                    continue
                lay = ("k" if a_kc else "m") + ("k" if b_kc else "m")
                add(id=f"g5-{M}x{N}x{K}-{lay}-f32-plain", group=5, path="small", M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc)
                add(id=f"g5-{M}x{N}x{K}-{lay}-bf16-gen_bwd", group=5, path="small", M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc,
                    out_bf16=True, epi="gen_bwd")
    for a_kc in (True, False):
        for b_kc in (True, False):
            lay = ("k" if a_kc else "m") + ("k" if b_kc else "m")
            add(id=f"g5-136x136x72-{lay}-f32-gen_fwd-batch3", group=5, path="small", M=136, N=136, K=72, a_kc=a_kc,
                b_kc=b_kc, epi="gen_fwd", batch=3, drop_ld=141)
    add(id="g5-129x136x72-kk-f32-cs_ws", group=5, path="small", M=129, N=136, K=72, epi="cs_ws")
    add(id="g5-129x136x72-kk-f32-cs_atomic", group=5, path="small", M=129, N=136, K=72, epi="cs_atomic")
    add(id="g5-136x261x200-mk-f32-cs_ws-batch3", group=5, path="small", M=136, N=261, K=200, a_kc=False, epi="cs_ws",
        batch=3)
    for bf in (False, True):   # N < 8: the element-wise tail, any alignment
        add(id=f"g5-16x5x64-kk-{'bf16' if bf else 'f32'}-ld11", group=5, path="small", M=16, N=5, K=64, out_bf16=bf,
            ld=11, epi="gen_fwd")
        add(id=f"g5-16x5x64-mk-{'bf16' if bf else 'f32'}-ld11", group=5, path="small", M=16, N=5, K=64, a_kc=False,
            out_bf16=bf, ld=11)

    # group 6: MX-fp8, single-stage (default threshold) and persistent (threshold 1)
    for M, N, K in ((1, 8, 128), (257, 264, 128), (300, 261, 384)):
        add(id=f"g6-single-{M}x{N}x{K}-gen_fwd", group=6, path="mx1", kind="mx8", M=M, N=N, K=K, epi="gen_fwd")
        add(id=f"g6-single-{M}x{N}x{K}-gen_bwd", group=6, path="mx1", kind="mx8", M=M, N=N, K=K, out_bf16=True,
            epi="gen_bwd")
    for spec, bf in MX_SPEC_OUT_BF16.items():
        q8 = "q8" in spec
        for K in (128, 256, 384):
            add(id=f"g6-8ph-{spec[3:]}-{300 if q8 else 257}x{512 if q8 else 264}x{K}", group=6, path="mx8ph", kind="mx8",
                M=300 if q8 else 257, N=512 if q8 else 264, K=K, out_bf16=bf, epi=spec, low=True)
        add(id=f"g6-8ph-{spec[3:]}-handover", group=6, path="mx8ph", kind="mx8", M=HANDOVER, N=512, K=256, out_bf16=bf,
            epi=spec, low=True)

    # group 8: ste_gemm_f32 on integer fp32 operands (a k-major operand needs its M or N % 4 == 0)
    for M, N, K in ((65, 68, 20), (64, 64, 16), (3, 8, 4), (68, 72, 20)):
        for a_kc in (True, False):
            for b_kc in (True, False):
                if (not a_kc and M % 4) or (not b_kc and N % 4):
                    continue
                lay = ("k" if a_kc else "m") + ("k" if b_kc else "m")
                add(id=f"g8-{M}x{N}x{K}-{lay}-plain", group=8, path="f32", kind="f32", M=M, N=N, K=K, a_kc=a_kc,
                    b_kc=b_kc, vals=64)
    add(id="g8-65x68x20-kk-gen_fwd", group=8, path="f32", kind="f32", M=65, N=68, K=20, epi="gen_fwd", vals=64)
    add(id="g8-65x68x20-km-gen_bwd", group=8, path="f32", kind="f32", M=65, N=68, K=20, b_kc=False, epi="gen_bwd",
        vals=64)
    add(id="g8-64x72x1028-mm-split", group=8, path="f32", kind="f32", M=64, N=72, K=1028, a_kc=False, b_kc=False,
        epi="dw", ws="f32split", vals=64)
    add(id="g8-64x72x1028-kk-split", group=8, path="f32", kind="f32", M=64, N=72, K=1028, epi="dw", ws="f32split",
        vals=64)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def ids(group):
    return [c.id for c in CASES if c.group == group]
