"""Per-kernel parity of the layer-norm wav2vec2 feature-encoder entry points (csrc/w2v2.hip:
ste_w2v_conv0_ln_fwd/_bwd, ste_w2v_ln_gelu_fwd/_bwd and their *_work queries), each alone against
a float64 torch reference of its header contract, at the smallest shapes that take every branch:
fewer rows than a block's four waves, ragged last blocks and frame tiles, more blocks than the grid
cap (grid-strided rows), at most and more than 32 partial slabs (one- and two-level column sums),
C = 64 / 96 / 512 / 1024 and 100 / 260 / 1020 (a partly idle wave; 8 or 4 channels per lane access,
one / two / four quads per lane), both tap-count instantiations, the S0·(T0-1) + K0 = N edge, fp32 and bf16 dh, bf16 and fp32 h, every optional
output NULL, and the error returns (host-side argument checks only).

Tolerances are those of tests/test_w2v2_kernels_gpu.py (its gn_fwd / gn_bwd / conv_fold cases),
imported from there: fp32 elementwise outputs and statistics relative L2 < 1e-6 against fp64; bf16
outputs |out - ref| <= 2^-8·|ref| + 1e-5·max|ref|; gradient reductions max(1e-6, 10·e32) with e32 the
error of plain fp32 torch autograd on the same inputs against the same fp64 reference."""
import pytest
import torch
import torch.nn.functional as F

from test_w2v2_kernels_gpu import BF16, DEV, EPS, ERR_SHAPE, F32, F32_TOL, F64, _assert_bf16_close, _margin, _p, _rel, _s

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


def _ln_gelu(y, gamma, beta):
    """gelu(LayerNorm_c(y)·γ + β) over the last dim, in the dtype of its arguments -> (h, mean, rstd)."""
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + EPS)
    return F.gelu((y - mu) * rs * gamma + beta), mu.squeeze(-1), rs.squeeze(-1)


# ------------------------------------------------------------------ LayerNorm + GELU (layers >= 1)
def _ln_fwd(lib, z, gamma, beta, h_f32):
    rows, Cc = z.shape
    h = torch.full((rows, Cc), 7.0, device=DEV, dtype=F32 if h_f32 else BF16)
    mean, rstd = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    rc = lib.fn("ste_w2v_ln_gelu_fwd")(_p(z), _p(gamma), _p(beta), rows, Cc, EPS, _p(h), int(h_f32), _p(mean),
                                       _p(rstd), _s(lib))
    return rc, h, mean, rstd


# C % 8 == 0: 8 channels per lane (two / four quads); else 4 per lane (one / two / four quads)
LN_SHAPES = [(1, 64), (7, 96), (130, 512), (5, 1024), (8200, 64), (3, 100), (6, 260), (3, 1020)]


@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
def test_ln_gelu_fwd(lib, rows, Cc):
    """h = gelu(LN(z)·γ + β) as bf16 and as fp32, mean / rstd per row; row 0 exactly constant:
    var = 0, rstd = 1/sqrt(eps), h = gelu(beta)."""
    torch.manual_seed(rows * 7 + Cc)
    z = (torch.randn(rows, Cc) * (0.5 + torch.rand(rows, 1)) + torch.randn(rows, 1)).bfloat16()
    z[0] = 1.5
    gamma, beta = 1 + 0.3 * torch.randn(Cc), 0.3 * torch.randn(Cc)
    href, mu, rs = _ln_gelu(z.double(), gamma.double(), beta.double())
    for h_f32 in (False, True):
        rc, h, mean, rstd = _ln_fwd(lib, z.to(DEV), gamma.to(DEV), beta.to(DEV), h_f32)
        assert rc == 0
        assert _rel(mean, mu) < F32_TOL and _rel(rstd, rs) < F32_TOL
        assert float(mean[0]) == 1.5
        if h_f32:
            assert _rel(h, href) < F32_TOL
        else:
            _assert_bf16_close(h, href, "h")


def _ln_bwd_ref(z, gamma, beta, dh, dtype):
    a = [t.to(dtype).clone().requires_grad_() for t in (z, gamma, beta)]
    (_ln_gelu(a[0], a[1], a[2])[0] * dh.to(dtype)).sum().backward()
    return dict(dz=a[0].grad, dgamma=a[1].grad, dbeta=a[2].grad, dbias=a[0].grad.sum(0))


@pytest.mark.parametrize("dh_bf16", [False, True])
@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
def test_ln_gelu_bwd(lib, rows, Cc, dh_bf16):
    """dz bf16 and the three column sums against fp64 autograd; the sums accumulate (+=), each may be
    NULL (all NULL: no workspace), and two runs are bit-identical."""
    torch.manual_seed(rows * 11 + Cc + dh_bf16)
    z = (torch.randn(rows, Cc) * (0.5 + torch.rand(rows, 1)) + torch.randn(rows, 1)).bfloat16()
    gamma, beta = 1 + 0.3 * torch.randn(Cc), 0.3 * torch.randn(Cc)
    dh = torch.randn(rows, Cc)
    if dh_bf16:
        dh = dh.bfloat16()
    ref = _ln_bwd_ref(z.float(), gamma, beta, dh.float(), F64)
    t32 = _ln_bwd_ref(z.float(), gamma, beta, dh.float(), F32)
    z_d, g_d, b_d, dh_d = z.to(DEV), gamma.to(DEV), beta.to(DEV), dh.to(DEV)
    rc, _, mean, rstd = _ln_fwd(lib, z_d, g_d, b_d, False)
    assert rc == 0
    nwork = int(lib.fn("ste_w2v_ln_gelu_work")(rows, Cc))
    assert nwork > 0
    work = torch.empty(nwork, device=DEV)
    sums = ("dgamma", "dbeta", "dbias")

    def run(init, has=sums, use_work=True):
        out = {n: (init[n].clone() if n in has else None) for n in sums}
        dz = torch.full((rows, Cc), 7.0, device=DEV, dtype=BF16)
        lib.call("ste_w2v_ln_gelu_bwd", _p(dh_d), int(dh_bf16), _p(z_d), _p(mean), _p(rstd), _p(g_d), _p(b_d), rows, Cc,
                 _p(dz), _p(out["dgamma"]), _p(out["dbeta"]), _p(out["dbias"]), _p(work) if use_work else None,
                 nwork if use_work else 0, _s(lib))
        out["dz"] = dz
        return out

    zeros = {n: torch.zeros(Cc, device=DEV) for n in sums}
    o1, o2 = run(zeros), run(zeros)
    _assert_bf16_close(o1["dz"], ref["dz"], "dz")
    for n in sums + ("dz",):
        assert torch.equal(o1[n], o2[n]), n                      # deterministic: no atomics
    for n in sums:
        _margin(_rel(o1[n], ref[n]), _rel(t32[n], ref[n]), f"ln_gelu_bwd {n} rows={rows} C={Cc} bf16={dh_bf16}")
    pre = {n: torch.randn_like(v) for n, v in zeros.items()}
    o3 = run(pre)
    for n in sums:                                               # +=: one fp32 add on top of the prefill
        assert _rel(o3[n], pre[n].double() + o1[n].double()) < F32_TOL, n
    for n in sums:                                               # each output alone, the others NULL
        o = run(zeros, has=(n,))
        assert torch.equal(o[n], o1[n]) and torch.equal(o["dz"], o1["dz"]), n
    o5 = run(zeros, has=(), use_work=False)
    assert torch.equal(o5["dz"], o1["dz"])


def test_ln_gelu_error_returns(lib):
    z = torch.randn(8, 1028, device=DEV).bfloat16()
    g = torch.ones(1028, device=DEV)
    work_fn, bwd = lib.fn("ste_w2v_ln_gelu_work"), lib.fn("ste_w2v_ln_gelu_bwd")
    h, mean, rstd = torch.empty_like(z), torch.empty(8, device=DEV), torch.empty(8, device=DEV)

    def fwd(rows, Cc):
        return lib.fn("ste_w2v_ln_gelu_fwd")(_p(z), _p(g), _p(g), rows, Cc, EPS, _p(h), 0, _p(mean), _p(rstd), _s(lib))

    assert fwd(8, 64) == 0
    assert fwd(8, 6) == ERR_SHAPE and int(work_fn(8, 6)) == 0         # C % 4 != 0
    assert fwd(8, 1028) == ERR_SHAPE and int(work_fn(8, 1028)) == 0   # C > 1024
    assert fwd(0, 64) == ERR_SHAPE and int(work_fn(0, 64)) == 0
    nwork = int(work_fn(8, 64))
    work = torch.empty(nwork, device=DEV)
    dz, dg = torch.empty_like(z), torch.zeros(64, device=DEV)

    def run(rows, Cc, dgamma, w, nw):
        return bwd(_p(z), 1, _p(z), _p(g), _p(g), _p(g), _p(g), rows, Cc, _p(dz), _p(dgamma), None, None, _p(w), nw,
                   _s(lib))

    assert run(8, 64, dg, work, nwork) == 0
    assert run(8, 64, dg, work, nwork - 1) == ERR_SHAPE               # work one float short
    assert run(8, 64, dg, None, nwork) == ERR_SHAPE                   # a sum without a workspace
    assert run(8, 64, None, None, 0) == 0
    assert run(8, 6, dg, work, nwork) == ERR_SHAPE
    assert run(8, 1028, dg, work, nwork) == ERR_SHAPE


# ------------------------------------------------------------------ conv0 + bias + LayerNorm + GELU
def _c0_chain(wave, w0, bias, gamma, beta, S0):
    """gelu(LN_c(conv0(wave) + bias)) in the dtype of its arguments -> (h, mean, rstd) [B, T0(, C)]."""
    y = F.conv1d(wave[:, None], w0[:, None], bias, stride=S0).transpose(1, 2)
    return _ln_gelu(y, gamma, beta)


def _c0_fwd(lib, big, N, w0, bias, gamma, beta, T0, S0, K0=None, Cc=None):
    B, ldw = big.shape
    Cc, K0 = w0.shape[0] if Cc is None else Cc, w0.shape[1] if K0 is None else K0
    h = torch.full((B * T0, Cc), 7.0, device=DEV, dtype=BF16)
    mean, rstd = torch.full((B * T0,), 7.0, device=DEV), torch.full((B * T0,), 7.0, device=DEV)
    rc = lib.fn("ste_w2v_conv0_ln_fwd")(_p(big), ldw, _p(w0), _p(bias), _p(gamma), _p(beta), B, N, T0, Cc, K0, S0, EPS,
                                        _p(h), _p(mean), _p(rstd), _s(lib))
    return rc, h, mean, rstd


# (B, T0, C, K0, S0, samples past the last window): one frame; a ragged 64-frame tile; three tiles per
# clip with a 2-frame last one and stride < kernel < 10 taps; C = 512 (two chunks per lane); 16 taps at
# stride 8 (the full LDS staging buffer); 1200 backward blocks of two tiles each (two-level slab sum)
C0_SHAPES = [(3, 1, 64, 10, 5, 3), (3, 77, 64, 10, 5, 0), (2, 130, 96, 3, 2, 3), (2, 7, 512, 10, 5, 3),
             (2, 70, 260, 16, 8, 0), (600, 130, 64, 3, 2, 3)]


def _c0_inputs(B, T0, Cc, K0, S0, extra):
    torch.manual_seed(B * 100 + T0 + Cc)
    Nw = S0 * (T0 - 1) + K0
    N = Nw + extra                       # extra = 0: S0·(T0-1) + K0 == N
    big = torch.randn(B, N + 5)
    w0, bias = torch.randn(Cc, K0) * 0.3, 0.3 * torch.randn(Cc)
    gamma, beta = 1 + 0.3 * torch.randn(Cc), 0.3 * torch.randn(Cc)
    return Nw, N, big, w0, bias, gamma, beta


@pytest.mark.parametrize("B,T0,Cc,K0,S0,extra", C0_SHAPES)
def test_conv0_ln_fwd(lib, B, T0, Cc, K0, S0, extra):
    Nw, N, big, w0, bias, gamma, beta = _c0_inputs(B, T0, Cc, K0, S0, extra)
    href, mu, rs = _c0_chain(big[:, :Nw].double(), w0.double(), bias.double(), gamma.double(), beta.double(), S0)
    rc, h, mean, rstd = _c0_fwd(lib, big.to(DEV), N, w0.to(DEV), bias.to(DEV), gamma.to(DEV), beta.to(DEV), T0, S0)
    assert rc == 0
    assert _rel(mean, mu.reshape(-1)) < F32_TOL and _rel(rstd, rs.reshape(-1)) < F32_TOL
    _assert_bf16_close(h, href.reshape(B * T0, Cc), "h")


def _c0_grads(wave, w0, bias, gamma, beta, dh, S0, dtype):
    a = [t.to(dtype).clone().requires_grad_() for t in (w0, bias, gamma, beta)]
    (_c0_chain(wave.to(dtype), *a, S0)[0] * dh.to(dtype)).sum().backward()
    return dict(dw0=a[0].grad, dbias=a[1].grad, dgamma=a[2].grad, dbeta=a[3].grad)


@pytest.mark.parametrize("B,T0,Cc,K0,S0,extra", C0_SHAPES)
def test_conv0_ln_bwd(lib, B, T0, Cc, K0, S0, extra):
    """dgamma / dbeta / dbias / dw0 against fp64 autograd; the outputs accumulate (+=), each may be
    NULL, and two runs are bit-identical."""
    Nw, N, big, w0, bias, gamma, beta = _c0_inputs(B, T0, Cc, K0, S0, extra)
    dh = torch.randn(B, T0, Cc)
    ref = _c0_grads(big[:, :Nw], w0, bias, gamma, beta, dh, S0, F64)
    t32 = _c0_grads(big[:, :Nw], w0, bias, gamma, beta, dh, S0, F32)
    big_d, w_d, bi_d, g_d, b_d = (t.to(DEV) for t in (big, w0, bias, gamma, beta))
    dh_d = dh.reshape(B * T0, Cc).to(DEV)
    rc, _, mean, rstd = _c0_fwd(lib, big_d, N, w_d, bi_d, g_d, b_d, T0, S0)
    assert rc == 0
    nwork = int(lib.fn("ste_w2v_conv0_ln_work")(B, T0, Cc, K0))
    assert nwork > 0
    work = torch.empty(nwork, device=DEV)
    names = ("dgamma", "dbeta", "dbias", "dw0")

    def run(init, has=names):
        out = {n: (init[n].clone() if n in has else None) for n in names}
        lib.call("ste_w2v_conv0_ln_bwd", _p(dh_d), _p(big_d), big.shape[1], _p(mean), _p(rstd), _p(w_d), _p(bi_d),
                 _p(g_d), _p(b_d), B, N, T0, Cc, K0, S0, _p(out["dgamma"]), _p(out["dbeta"]), _p(out["dbias"]),
                 _p(out["dw0"]), _p(work), nwork, _s(lib))
        return out

    zeros = {n: torch.zeros(Cc, device=DEV) for n in names[:3]}
    zeros["dw0"] = torch.zeros(Cc, K0, device=DEV)
    o1, o2 = run(zeros), run(zeros)
    for n in names:
        assert torch.equal(o1[n], o2[n]), n                      # deterministic: no atomics
        _margin(_rel(o1[n], ref[n]), _rel(t32[n], ref[n]), f"conv0_ln_bwd {n} B={B} T0={T0} C={Cc}")
    pre = {n: torch.randn_like(v) for n, v in zeros.items()}
    o3 = run(pre)
    for n in names:                                              # +=: one fp32 add on top of the prefill
        assert _rel(o3[n], pre[n].double() + o1[n].double()) < F32_TOL, n
    for n in names:                                              # each output alone, the others NULL
        assert torch.equal(run(zeros, has=(n,))[n], o1[n]), n


def test_conv0_ln_error_returns(lib):
    big = torch.randn(2, 200, device=DEV)
    w = torch.randn(516, 17, device=DEV)
    v = torch.ones(516, device=DEV)

    def fwd(N, T0, S0, K0, Cc=8):
        return _c0_fwd(lib, big, N, w, v, v, v, T0, S0, K0=K0, Cc=Cc)[0]

    assert fwd(200, 8, 5, 17) == ERR_SHAPE             # more than 16 taps
    assert fwd(200, 8, 9, 10) == ERR_SHAPE             # stride above 8
    assert fwd(5 * 38 + 10, 39, 5, 10) == 0            # S0·(T0-1) + K0 == N
    assert fwd(5 * 38 + 9, 39, 5, 10) == ERR_SHAPE     # last window past N
    assert fwd(200, 8, 5, 10, Cc=6) == ERR_SHAPE       # C % 4 != 0
    assert fwd(200, 8, 5, 10, Cc=516) == ERR_SHAPE     # C > 512
    work_fn = lib.fn("ste_w2v_conv0_ln_work")
    assert int(work_fn(2, 8, 6, 10)) == 0 and int(work_fn(2, 8, 516, 10)) == 0 and int(work_fn(2, 8, 8, 17)) == 0
    nwork = int(work_fn(2, 8, 8, 10))
    work = torch.empty(nwork, device=DEV)
    dh = torch.randn(16, 8, device=DEV)
    dg = torch.zeros(8, device=DEV)

    def bwd(N, T0, S0, K0, Cc, nw):
        return lib.fn("ste_w2v_conv0_ln_bwd")(_p(dh), _p(big), 200, _p(v), _p(v), _p(w), _p(v), _p(v), _p(v), 2, N, T0,
                                              Cc, K0, S0, _p(dg), None, None, None, _p(work), nw, _s(lib))

    assert bwd(200, 8, 5, 10, 8, nwork) == 0
    assert bwd(200, 8, 5, 10, 8, nwork - 1) == ERR_SHAPE          # work one float short
    assert bwd(5 * 7 + 9, 8, 5, 10, 8, nwork) == ERR_SHAPE        # last window past N
    assert bwd(200, 8, 5, 10, 6, nwork) == ERR_SHAPE
    assert bwd(200, 8, 9, 10, 8, nwork) == ERR_SHAPE
