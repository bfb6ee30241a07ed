"""Per-kernel parity of the wav2vec2 front-end entry points (csrc/w2v2.hip, the ste_w2v_* block of
include/ste.h), each against a float64 torch / numpy reference of the contract the header states,
at the smallest shapes that take every branch of the kernel: ragged last tiles and chunks, channel
counts that do not divide the 256-thread block, strides larger than the kernel, odd tap counts,
row strides past the row, NULL options and the error returns.

Tolerances:
* fp32 outputs of short sums / elementwise work: relative L2 < 1e-6 against fp64 (F32_TOL);
* bf16 outputs computed from fp32 values: |out - ref| <= 2^-8·|ref| + 1e-5·max|ref| elementwise
  (round-to-nearest-even costs at most 2^-9 relative, the rest covers the fp32 error before it);
* pure moves: torch.equal;
* gradient reductions (and the mean-50 / std-0.01 clip of wave_norm): max(1e-6, 10·e32), e32 being
  the relative L2 error of plain fp32 torch (autograd) on the same inputs against the same fp64
  reference; the factor 10 covers a different summation order.  e32 comes from the reference
  side only; both figures are in the assert message.
References are computed on the CPU (float64 convolutions) and compared there.

Measured on an MI355X, kernel error / e32 (bound = max(1e-6, 10·e32)):
  gn_bwd (B,T0,C)     dgamma               dbeta                dw0
  (3,77,12)           1.0e-7 / 1.4e-7      4.9e-8 / 1.7e-7      1.5e-7 / 1.9e-7
  (2,40,260)          8.7e-8 / 1.4e-7      6.4e-8 / 1.2e-7      1.4e-7 / 2.0e-7
  (40,64,8)           9.9e-8 / 1.5e-7      1.8e-7 / 1.1e-7      1.5e-7 / 2.6e-7
  (2,600,8)           2.9e-7 / 3.9e-7      9.0e-8 / 2.2e-7      2.0e-7 / 2.1e-7
  wnorm_bwd (D,K)     dv                   dg
  (16,5)              4.2e-8 / 5.3e-8      5.1e-8 / 1.3e-7
  (64,16)             4.2e-8 / 5.4e-8      5.9e-8 / 1.9e-7
  wave_norm, the mean-50 / std-0.01 clip: 2.8e-8 / 1.7e-4 (777 samples), 2.5e-8 / 7.4e-5 (1000)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kref import drop_scale, w2v2_frame_mask_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ERR_SHAPE = 1002       # STE_ERR_SHAPE (include/ste.h)
F32_TOL = 1e-6
EPS = float(np.float32(1e-5))   # the GroupNorm eps as the kernel receives it (a float argument)


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


def _s(lib):
    return lib.stream_ptr()


def _p(t):
    return None if t is None else t.data_ptr()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _assert_bf16_close(out, ref, what=""):
    """bf16 output of an fp32 value: |out - ref| <= 2^-8·|ref| + 1e-5·max|ref| elementwise."""
    assert out.dtype == BF16
    o, r = out.double().cpu(), ref.double().cpu().reshape(out.shape)
    excess = (o - r).abs() - (2.0 ** -8 * r.abs() + 1e-5 * r.abs().max())
    assert float(excess.max()) <= 0, (what, float(excess.max()), int((excess > 0).sum()))


def _margin(err, e32, what):
    """The measured-margin rule for reductions: kernel error <= max(1e-6, 10·e32)."""
    bound = max(1e-6, 10 * e32)
    print(f"{what}: kernel {err:.3e}, fp32 torch {e32:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: kernel error {err:.3e} > bound {bound:.3e} (fp32 torch error e32 = {e32:.3e})"


def _gelu_d64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * np.pi) ** 0.5


# ------------------------------------------------------------------ conv0 forward
def _conv0_fwd(lib, big, N, w0, T0, S0, K0=None):
    B, ldw = big.shape
    C_, K0 = w0.shape[0], w0.shape[1] if K0 is None else K0
    y = torch.full((B * T0, C_), 7.0, device=DEV)
    rc = lib.fn("ste_w2v_conv0_fwd")(_p(big), ldw, _p(w0), B, N, T0, C_, K0, S0, _p(y), _s(lib))
    return rc, y


@pytest.mark.parametrize("K0,S0,T0,Cc", [(10, 5, 77, 12), (16, 8, 33, 260), (1, 1, 32, 4), (3, 5, 40, 8)])
def test_conv0_fwd(lib, K0, S0, T0, Cc):
    """y[b·T0 + t, c] = Σ_j w0[c, j]·wave[b, S0·t + j]: ragged last 32-frame tile (T0 = 77, 33), the
    full LDS staging buffer (K0 = 16, S0 = 8: 264 of 272 floats), C > 256 (a second channel pass),
    stride > kernel, a wave row stride past N and samples past the last window."""
    torch.manual_seed(K0 * 100 + T0)
    B = 3
    N = S0 * (T0 - 1) + K0 + 3
    big = torch.randn(B, N + 5)
    w0 = torch.randn(Cc, K0)
    ref = F.conv1d(big[:, None, :N].double(), w0[:, None].double(), stride=S0)[:, :, :T0]
    ref = ref.transpose(1, 2).reshape(B * T0, Cc)
    rc, y = _conv0_fwd(lib, big.to(DEV), N, w0.to(DEV), T0, S0)
    assert rc == 0
    assert _rel(y, ref) < F32_TOL


def test_conv0_fwd_error_returns(lib):
    big = torch.randn(2, 200, device=DEV)
    w = torch.randn(8, 17, device=DEV)
    assert _conv0_fwd(lib, big, 200, w, 8, 5, K0=17)[0] == ERR_SHAPE          # more than 16 taps
    assert _conv0_fwd(lib, big, 200, w, 8, 9, K0=10)[0] == ERR_SHAPE          # stride above 8
    assert _conv0_fwd(lib, big, 5 * 38 + 10, w, 39, 5, K0=10)[0] == 0         # S0·(T0-1) + K0 == N
    assert _conv0_fwd(lib, big, 5 * 38 + 9, w, 39, 5, K0=10)[0] == ERR_SHAPE  # last window past N


# ------------------------------------------------------------------ GroupNorm + GELU
def _gn_fwd(lib, y, gamma, beta, B, T0, Cc, short=0):
    mean, rstd = torch.full((B * Cc,), 7.0, device=DEV), torch.full((B * Cc,), 7.0, device=DEV)
    h = torch.full((B * T0, Cc), 7.0, device=DEV, dtype=BF16)
    nwork = int(lib.fn("ste_w2v_gn_work")(B, T0, Cc, 1))
    work = torch.empty(max(nwork, 1), device=DEV)
    rc = lib.fn("ste_w2v_gn_fwd")(_p(y), _p(gamma), _p(beta), B, T0, Cc, EPS, _p(mean), _p(rstd), _p(h), _p(work),
                                  nwork - short, _s(lib))
    return rc, mean, rstd, h


@pytest.mark.parametrize("B,T0,Cc", [(2, 600, 8), (3, 3, 8), (2, 40, 768), (1, 20, 1024), (2, 50, 4), (2, 77, 12)])
def test_gn_fwd(lib, B, T0, Cc):
    """GroupNorm(C groups) over time + affine + GELU: two 512-row chunks with a ragged second
    (T0 = 600), fewer rows than row groups (T0 = 3), Q = C/4 = 192 and 3 (idle threads past the last
    whole row group), one row group (C = 1024), Q = 1; one channel of one clip exactly constant:
    var = 0, rstd = 1/sqrt(eps), h = gelu(beta)."""
    torch.manual_seed(B * 1000 + T0 + Cc)
    y = torch.randn(B, T0, Cc) * (0.5 + torch.rand(Cc)) + torch.randn(Cc)
    y[0, :, 1] = 1.5
    gamma, beta = 1 + 0.3 * torch.randn(Cc), 0.3 * torch.randn(Cc)
    yd = y.double()
    mu = yd.mean(1, keepdim=True)
    var = ((yd - mu) ** 2).mean(1, keepdim=True)
    rs = 1 / torch.sqrt(var + EPS)
    href = F.gelu((yd - mu) * rs * gamma.double() + beta.double()).reshape(B * T0, Cc)
    rc, mean, rstd, h = _gn_fwd(lib, y.reshape(B * T0, Cc).to(DEV), gamma.to(DEV), beta.to(DEV), B, T0, Cc)
    assert rc == 0
    assert _rel(mean, mu.reshape(-1)) < F32_TOL
    assert _rel(rstd, rs.reshape(-1)) < F32_TOL
    assert float(rstd[1]) == float(np.float32(1 / np.sqrt(EPS))) and float(mean[1]) == 1.5
    _assert_bf16_close(h, href, "h")
    assert torch.equal(h.view(B, T0, Cc)[0, :, 1].cpu(), F.gelu(beta[1]).bfloat16().expand(T0))


def test_gn_fwd_error_returns(lib):
    y = torch.randn(2 * 8 * 1028, device=DEV)
    g = torch.ones(1028, device=DEV)
    assert _gn_fwd(lib, y, g, g, 2, 8, 8, short=1)[0] == ERR_SHAPE     # work one float short
    assert _gn_fwd(lib, y, g, g, 2, 8, 8)[0] == 0
    assert int(lib.fn("ste_w2v_gn_work")(2, 8, 6, 1)) == 0
    assert _gn_fwd(lib, y, g, g, 2, 8, 6)[0] == ERR_SHAPE              # C % 4 != 0
    assert _gn_fwd(lib, y, g, g, 2, 8, 1028)[0] == ERR_SHAPE           # C > 1024


def _gn_chain(wave, w0, gamma, beta, dh, S0):
    """Σ dh·gelu(GroupNorm(conv0(wave, w0))) in the dtype of its arguments; dh [B, C, T0]."""
    y = F.conv1d(wave[:, None], w0[:, None], stride=S0)
    mu = y.mean(2, keepdim=True)
    var = ((y - mu) ** 2).mean(2, keepdim=True)
    z = (y - mu) * torch.rsqrt(var + EPS) * gamma[None, :, None] + beta[None, :, None]
    return (F.gelu(z) * dh).sum()


def _gn_grads(wave, w0, gamma, beta, dh, S0, dtype):
    a = [t.to(dtype).clone().requires_grad_() for t in (w0, gamma, beta)]
    _gn_chain(wave.to(dtype), a[0], a[1], a[2], dh.to(dtype), S0).backward()
    return dict(dw0=a[0].grad, dgamma=a[1].grad, dbeta=a[2].grad)


@pytest.mark.parametrize("B,T0,Cc,K0,S0", [(3, 77, 12, 10, 5), (2, 40, 260, 3, 5), (40, 64, 8, 10, 5),
                                           (2, 600, 8, 16, 8)])
def test_gn_bwd(lib, B, T0, Cc, K0, S0):
    """dgamma / dbeta / dw0 of conv0 + GroupNorm + GELU against fp64 autograd: a 13-row last dW
    block (T0 = 77), a second channel pass with inactive lanes (C = 260), B·nc0 = 80 > 32 partial
    slabs (the two-level sum), two GroupNorm chunks (T0 = 600).  The outputs accumulate (+=), each
    may be NULL, and two runs are bit-identical."""
    torch.manual_seed(B * 100 + T0)
    Nw = S0 * (T0 - 1) + K0
    N, ldw = Nw + 3, Nw + 8
    big = torch.randn(B, ldw)
    wave = big[:, :Nw]
    w0 = torch.randn(Cc, K0) * 0.3
    gamma, beta = 1 + 0.3 * torch.randn(Cc), 0.3 * torch.randn(Cc)
    dh = torch.randn(B, Cc, T0)
    ref = _gn_grads(wave, w0, gamma, beta, dh, S0, F64)
    t32 = _gn_grads(wave, w0, gamma, beta, dh, S0, F32)
    y = F.conv1d(wave[:, None], w0[:, None], stride=S0).transpose(1, 2).reshape(B * T0, Cc).contiguous().to(DEV)
    g_d, b_d, big_d = gamma.to(DEV), beta.to(DEV), big.to(DEV)
    dh_d = dh.transpose(1, 2).reshape(B * T0, Cc).contiguous().to(DEV)
    rc, mean, rstd, _ = _gn_fwd(lib, y, g_d, b_d, B, T0, Cc)
    assert rc == 0
    nwork = int(lib.fn("ste_w2v_gn_work")(B, T0, Cc, K0))
    work = torch.empty(nwork, device=DEV)

    def run(init, has=("dgamma", "dbeta", "dw0")):
        out = {n: (init[n].clone() if n in has else None) for n in ("dgamma", "dbeta", "dw0")}
        lib.call("ste_w2v_gn_bwd", _p(dh_d), _p(y), _p(mean), _p(rstd), _p(g_d), _p(b_d), _p(big_d), ldw, B, N, T0, Cc,
                 K0, S0, _p(out["dgamma"]), _p(out["dbeta"]), _p(out["dw0"]), _p(work), nwork, _s(lib))
        return out

    zeros = dict(dgamma=torch.zeros(Cc, device=DEV), dbeta=torch.zeros(Cc, device=DEV),
                 dw0=torch.zeros(Cc, K0, device=DEV))
    o1, o2 = run(zeros), run(zeros)
    for n in zeros:
        assert torch.equal(o1[n], o2[n]), n                      # deterministic: no atomics
        _margin(_rel(o1[n], ref[n]), _rel(t32[n], ref[n]), f"gn_bwd {n} B={B} T0={T0} C={Cc}")
    pre = {n: torch.randn_like(v) for n, v in zeros.items()}
    o3 = run(pre)
    for n in zeros:                                              # +=: one fp32 add on top of the prefill
        assert _rel(o3[n], pre[n].double() + o1[n].double()) < F32_TOL, n
    o4 = run(zeros, has=("dgamma", "dbeta"))
    assert torch.equal(o4["dgamma"], o1["dgamma"]) and torch.equal(o4["dbeta"], o1["dbeta"])
    o5 = run(zeros, has=("dw0",))
    assert torch.equal(o5["dw0"], o1["dw0"])


# ------------------------------------------------------------------ col2im fold
@pytest.mark.parametrize("Cc", [4, 260])
@pytest.mark.parametrize("k,s", [(3, 2), (2, 2), (10, 5), (3, 5), (1, 1)])
def test_conv_fold(lib, k, s, Cc):
    """out[b, s·to + j] += dcol[b·To + to, j·C:(j+1)·C], times gelu'(z) when z is given: overlapping
    windows, stride > kernel (gaps: uncovered rows are exactly 0), two trailing frames in no window,
    C = 260 (65 vectors per row, 520 > 256 per block), ldd past k·C, fp32 and bf16 outputs;
    k = s = 1 with z is the engine's "gelu' only" call."""
    torch.manual_seed(k * 10 + s + Cc)
    B, To = 3, 9
    Ti = s * (To - 1) + k + 2
    for ldd in (k * Cc, k * Cc + 8):
        dbig = torch.randn(B * To, ldd)
        z = torch.randn(B * Ti, Cc).bfloat16()
        fold = torch.zeros(B, Ti, Cc, dtype=F64)
        cover = torch.zeros(Ti, dtype=torch.long)
        dv = dbig.double().view(B, To, ldd)
        for to in range(To):
            for j in range(k):
                fold[:, s * to + j] += dv[:, to, j * Cc:(j + 1) * Cc]
                cover[s * to + j] += 1
        assert int((cover[-2:] != 0).sum()) == 0
        dbig_d, z_d = dbig.to(DEV), z.to(DEV)
        for with_z in (False, True):
            ref = fold.view(B * Ti, Cc) * (_gelu_d64(z) if with_z else 1.0)
            for out_bf16 in (0, 1):
                out = torch.full((B * Ti, Cc), 7.0, device=DEV, dtype=BF16 if out_bf16 else F32)
                lib.call("ste_w2v_conv_fold", _p(dbig_d), ldd, _p(z_d) if with_z else None, B, Ti, To, Cc, k, s,
                         _p(out), out_bf16, _s(lib))
                what = f"ldd={ldd} z={with_z} bf16={out_bf16}"
                if out_bf16:
                    _assert_bf16_close(out, ref, what)
                else:
                    assert _rel(out, ref) < F32_TOL, what
                assert int(torch.count_nonzero(out.view(B, Ti, Cc)[:, (cover == 0).to(DEV)])) == 0, what


# ------------------------------------------------------------------ slab sum, permute
@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("n", [1000, 3_000_000])
def test_slab_sum(lib, n, S):
    """out[i] += Σ_s part[s·n + i] in slab order: bit-equal to the same fp32 sequence in torch;
    n = 3·10^6 runs the grid-stride loop (the grid is capped at 8192 blocks of 256)."""
    torch.manual_seed(n + S)
    part = torch.randn(S, n, device=DEV)
    out0 = torch.randn(n, device=DEV)
    out = out0.clone()
    lib.call("ste_w2v_slab_sum", _p(out), _p(part), n, S, _s(lib))
    a = torch.zeros(n, device=DEV)
    for sl in range(S):
        a += part[sl]
    assert torch.equal(out, out0 + a)
    assert _rel(out, out0.double() + part.double().sum(0)) < F32_TOL


@pytest.mark.parametrize("A,P,Q", [(5, 3, 7), (4, 64, 2)])
def test_perm12(lib, A, P, Q):
    """[A][P][Q] -> [A][Q][P]: the bf16 copy, and the fp32 += (one add per element: bit-exact)."""
    torch.manual_seed(A + P + Q)
    src = torch.randn(A, P, Q, device=DEV)
    sb = src.bfloat16()
    db = torch.full((A, Q, P), 7.0, device=DEV, dtype=BF16)
    lib.call("ste_w2v_perm12", _p(sb), _p(db), A, P, Q, 0, _s(lib))
    assert torch.equal(db, sb.transpose(1, 2).contiguous())
    d0 = torch.randn(A, Q, P, device=DEV)
    d = d0.clone()
    lib.call("ste_w2v_perm12", _p(src), _p(d), A, P, Q, 1, _s(lib))
    assert torch.equal(d, d0 + src.transpose(1, 2))


# ------------------------------------------------------------------ positional conv
def _pos_pack(lib, x, B, T, D, G, K, padl):
    Cg, Tp = D // G, T + K - 1
    out = torch.full((G, B * Tp + K, Cg), 7.0, device=DEV, dtype=BF16)
    rc = lib.fn("ste_w2v_pos_pack")(_p(x), B, T, D, G, K, padl, _p(out), _s(lib))
    return rc, out


def _pos_pack_ref(x, B, T, D, G, K, padl):
    """out[g][b·Tp + u][ci] = bf16(x[b, u - padl, g·Cg + ci]), zero outside [0, T) and in the K tail rows."""
    Cg, Tp = D // G, T + K - 1
    ref = torch.zeros(G, B * Tp + K, Cg, dtype=BF16, device=x.device)
    xb = x.bfloat16().view(B, T, G, Cg)
    for b in range(B):
        ref[:, b * Tp + padl:b * Tp + padl + T] = xb[b].transpose(0, 1)
    return ref


@pytest.mark.parametrize("B,T,D,G,K,padl", [(2, 19, 32, 2, 4, 2), (2, 19, 32, 2, 4, 1), (3, 7, 48, 3, 5, 2),
                                            (1, 5, 16, 1, 16, 8)])
def test_pos_pack(lib, B, T, D, G, K, padl):
    """The group-major zero-padded bf16 copy: both paddings the engine uses (K/2 forward, K-1-K/2
    for the gradient), an odd tap count, more taps than frames."""
    torch.manual_seed(T * K + padl)
    x = torch.randn(B * T, D, device=DEV)
    rc, out = _pos_pack(lib, x, B, T, D, G, K, padl)
    assert rc == 0
    assert torch.equal(out, _pos_pack_ref(x, B, T, D, G, K, padl))


def test_pos_pack_error_returns(lib):
    x = torch.randn(2 * 19, 32, device=DEV)
    assert _pos_pack(lib, x, 2, 19, 32, 2, 4, 4)[0] == ERR_SHAPE      # padl = K
    assert _pos_pack(lib, x, 2, 19, 32, 8, 4, 2)[0] == ERR_SHAPE      # (D/G) % 8 != 0


def test_pos_elem(lib):
    """mode 0 src + gelu(cpad + bias); mode 1 src·gelu'(cpad + bias); mode 2 (src + cpad)·maskf[row]
    (maskf NULL = 1); cpad rows b·Tp + t with Tp = T + K - 1, D = 20 (5 vectors per row)."""
    torch.manual_seed(11)
    B, T, D, K = 3, 19, 20, 4
    Tp = T + K - 1
    cpad, bias, src = torch.randn(B * Tp, D), torch.randn(D), torch.randn(B * T, D)
    maskf = (torch.rand(B * T) < 0.7).float()
    cp = cpad.double().view(B, Tp, D)[:, :T].reshape(B * T, D)
    c, sd = cp + bias.double(), src.double()
    refs = {(0, False): sd + F.gelu(c), (1, False): sd * _gelu_d64(c), (2, False): sd + cp,
            (2, True): (sd + cp) * maskf[:, None]}
    cpad_d, bias_d, src_d, m_d = (t.to(DEV) for t in (cpad, bias, src, maskf))
    for (mode, with_mask), ref in refs.items():
        out = torch.full((B * T, D), 7.0, device=DEV)
        lib.call("ste_w2v_pos_elem", mode, _p(cpad_d), _p(bias_d) if mode < 2 else None, _p(src_d),
                 _p(m_d) if with_mask else None, B, T, D, Tp, _p(out), _s(lib))
        assert _rel(out, ref) < F32_TOL, (mode, with_mask)
    assert lib.fn("ste_w2v_pos_elem")(0, _p(cpad_d), None, _p(src_d), None, B, T, D, Tp, _p(out), _s(lib)) == ERR_SHAPE


@pytest.mark.parametrize("K", [4, 5])
def test_pos_conv_composed(lib, K):
    """The positional conv as the engine runs it: pos_pack -> the batched GEMM whose A rows overlap
    (row stride Cg < K·Cg) and whose C is a column slice (ldc = D, stride_c = Cg) -> pos_elem, for
    the forward (mode 0) and the input gradient (padl = K-1-K/2, reversed-tap operand wf, mode 2),
    against F.conv1d(padding = K/2, groups = G) with the SamePad trim (even K) + GELU + residual
    and its autograd in fp64.  wr / wf are built by hand in the documented layouts from one set of
    bf16 values and x / dY are bf16-exact, so both sides multiply identical numbers: fp32
    accumulation, relative L2 < 1e-5 as in the GEMM tests."""
    from speech_transcript_embeddings_amd import wav2vec2
    torch.manual_seed(K)
    B, T, D, G = 2, 19, 32, 2
    Cg, Tp = D // G, T + K - 1
    seg = B * Tp + K
    wr = (torch.randn(G, Cg, K, Cg) * 0.2).bfloat16()                        # [g][co][j][ci]
    W = wr.permute(0, 1, 3, 2).reshape(D, Cg, K).double()                    # W[g·Cg + co, ci, j]
    wf = wr.flip(2).permute(0, 3, 2, 1).contiguous()                         # [g][ci][K-1-j][co]
    x = torch.randn(B * T, D).bfloat16().float()
    bias = torch.randn(D)
    dY = torch.randn(B * T, D).bfloat16().float()
    dxe = torch.randn(B * T, D)
    maskf = (torch.rand(B * T) < 0.7).float()
    xd = x.double().view(B, T, D).transpose(1, 2).clone().requires_grad_()
    conv = F.conv1d(xd, W, bias.double(), padding=K // 2, groups=G)[:, :, :T]
    out_ref = (xd + F.gelu(conv)).transpose(1, 2).reshape(B * T, D)
    (conv * dY.double().view(B, T, D).transpose(1, 2)).sum().backward()
    dx_ref = (dxe.double() + xd.grad.transpose(1, 2).reshape(B * T, D)) * maskf[:, None]

    x_d, bias_d, dY_d, dxe_d, m_d = (t.to(DEV) for t in (x, bias, dY, dxe, maskf))
    wr_d, wf_d = wr.to(DEV).reshape(-1), wf.to(DEV).reshape(-1)
    rc, xp = _pos_pack(lib, x_d, B, T, D, G, K, K // 2)
    assert rc == 0
    cpad = torch.full((B * Tp, D), 7.0, device=DEV)
    wav2vec2._pos_gemm(xp.reshape(-1), wr_d, cpad, B * Tp, G, Cg, K, seg)
    out = torch.empty(B * T, D, device=DEV)
    lib.call("ste_w2v_pos_elem", 0, _p(cpad), _p(bias_d), _p(x_d), None, B, T, D, Tp, _p(out), _s(lib))
    assert _rel(out, out_ref) < 1e-5
    assert _rel(cpad.view(B, Tp, D)[:, :T], (conv - bias.double()[:, None]).transpose(1, 2)) < 1e-5

    rc, dyp = _pos_pack(lib, dY_d, B, T, D, G, K, K - 1 - K // 2)
    assert rc == 0
    dxpad = torch.full((B * Tp, D), 7.0, device=DEV)
    wav2vec2._pos_gemm(dyp.reshape(-1), wf_d, dxpad, B * Tp, G, Cg, K, seg)
    dx = torch.empty(B * T, D, device=DEV)
    lib.call("ste_w2v_pos_elem", 2, _p(dxpad), None, _p(dxe_d), _p(m_d), B, T, D, Tp, _p(dx), _s(lib))
    assert _rel(dx, dx_ref) < 1e-5


# ------------------------------------------------------------------ weight norm
def _wnorm_W(v, g):
    """W[o, i, j] = g[j]·v[o, i, j]/‖v[:, :, j]‖ (weight_norm, dim = 2) in the dtype of v."""
    return g[None, None, :] * v / v.pow(2).sum((0, 1), keepdim=True).sqrt()


def _wnorm_grads(v, g, dW, dtype):
    a = [t.to(dtype).clone().requires_grad_() for t in (v, g)]
    (_wnorm_W(a[0], a[1]) * dW.to(dtype)).sum().backward()
    return dict(dv=a[0].grad, dg=a[1].grad)


@pytest.mark.parametrize("D,Cg,K", [(16, 8, 5), (64, 8, 16)])
def test_wnorm_fwd_bwd(lib, D, Cg, K):
    """weight_norm over (out, in) per tap: norms, the forward operand wr[g][co][j][ci] and the
    reversed-tap operand wf[g][ci][K-1-j][co] (n = D·Cg = 128 < 256 threads and 512 > 256); the
    backward from dW in the wr layout against fp64 autograd of Σ W·dW, dv / dg accumulating, each
    NULL in turn."""
    torch.manual_seed(D + K)
    G = D // Cg
    v, g = torch.randn(D, Cg, K), 1 + 0.5 * torch.rand(K)
    W = _wnorm_W(v.double(), g.double())
    v_d, g_d = v.to(DEV), g.to(DEV)
    norms = torch.full((K,), 7.0, device=DEV)
    wr = torch.full((G, Cg, K, Cg), 7.0, device=DEV, dtype=BF16)
    wf = torch.full((G, Cg, K, Cg), 7.0, device=DEV, dtype=BF16)
    lib.call("ste_w2v_wnorm_fwd", _p(v_d), _p(g_d), D, Cg, K, _p(norms), _p(wr), _p(wf), _s(lib))
    assert _rel(norms, v.double().pow(2).sum((0, 1)).sqrt()) < F32_TOL
    wr_ref = W.view(G, Cg, Cg, K).permute(0, 1, 3, 2)                  # [g][co][j][ci] = W[g·Cg + co, ci, j]
    wf_ref = W.view(G, Cg, Cg, K).flip(3).permute(0, 2, 3, 1)          # [g][ci][K-1-j][co]
    _assert_bf16_close(wr, wr_ref, "wr")
    _assert_bf16_close(wf, wf_ref, "wf")
    assert torch.equal(wf, wr.flip(2).permute(0, 3, 2, 1).contiguous())   # the same rounded values, moved

    dwr = torch.randn(G, Cg, K, Cg)                                     # dW in the wr layout
    dW = dwr.permute(0, 1, 3, 2).reshape(D, Cg, K)
    ref, t32 = _wnorm_grads(v, g, dW, F64), _wnorm_grads(v, g, dW, F32)
    dwr_d = dwr.to(DEV)

    def run(dv, dg):
        lib.call("ste_w2v_wnorm_bwd", _p(dwr_d), _p(v_d), _p(g_d), _p(norms), D, Cg, K, _p(dv), _p(dg), _s(lib))
        return dv, dg

    dv, dg = run(torch.zeros(D, Cg, K, device=DEV), torch.zeros(K, device=DEV))
    _margin(_rel(dv, ref["dv"]), _rel(t32["dv"], ref["dv"]), f"wnorm_bwd dv D={D} K={K}")
    _margin(_rel(dg, ref["dg"]), _rel(t32["dg"], ref["dg"]), f"wnorm_bwd dg D={D} K={K}")
    pv, pg = torch.randn(D, Cg, K, device=DEV), torch.randn(K, device=DEV)
    dv2, dg2 = run(pv.clone(), pg.clone())
    assert _rel(dv2, pv.double() + dv.double()) < F32_TOL and _rel(dg2, pg.double() + dg.double()) < F32_TOL
    assert torch.equal(run(torch.zeros_like(dv), None)[0], dv)
    assert torch.equal(run(None, torch.zeros_like(dg))[1], dg)


# ------------------------------------------------------------------ masks, normalisation, dropout
def _frame_mask(lib, mask, B, N, Tf, ks, ss, want_f=True, want_i=True):
    maskf = torch.full((B * Tf,), 7.0, device=DEV) if want_f else None
    mask32 = torch.full((B * Tf,), 7, device=DEV, dtype=torch.int32) if want_i else None
    n = len(ks)
    lib.call("ste_w2v_frame_mask", _p(mask), B, N, Tf, n, (C.c_int * n)(*ks), (C.c_int * n)(*ss), _p(maskf),
             _p(mask32), _s(lib))
    return maskf, mask32


def _sample_mask(sums, N):
    """[B, N] int64 with the given numbers of ones: prefixes, one clip's ones scattered (the kernel
    and transformers both count them)."""
    mask = (torch.arange(N)[None, :] < torch.tensor(sums)[:, None]).long()
    r = len(sums) // 2
    g = torch.Generator().manual_seed(5)
    mask[r] = 0
    mask[r, torch.randperm(N, generator=g)[:sums[r]]] = 1
    assert mask.sum(-1).tolist() == list(sums)
    return mask


FRAME_STACKS = {"mini": ((10, 3, 2), (5, 2, 2), 400, 19, [0, 1, 9, 10, 14, 25, 26, 399, 400]),
                "base": ((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2), 4000, 12,
                         [0, 1, 9, 10, 14, 25, 26, 399, 400, 1234, 3999, 4000])}


@pytest.mark.parametrize("stack", ["mini", "base"])
def test_frame_mask(lib, stack):
    """transformers' _get_feature_vector_attention_mask (kref.w2v2_frame_mask_ref, pinned to it by
    tests/test_w2v2_cpu.py), including clips shorter than the receptive field: a conv output
    length L <= 0 indexes from the end, so L = 0 marks every frame and L = -1 all but the last.
    More than 256 samples per clip (the block reduction), mask = NULL, either output alone."""
    ks, ss, N, Tf, sums = FRAME_STACKS[stack]
    mask = _sample_mask(sums, N)
    B = len(sums)
    ref = w2v2_frame_mask_ref(mask, Tf, ks, ss)
    mask_d = mask.to(DEV)
    maskf, mask32 = _frame_mask(lib, mask_d, B, N, Tf, ks, ss)
    short = [i for i, n in enumerate(sums) if n < 10]
    assert torch.equal(maskf.view(B, Tf)[short].cpu(), ref[short].float()), "clips below the first conv kernel"
    assert torch.equal(maskf.view(B, Tf).cpu(), ref.float())
    assert torch.equal(mask32.view(B, Tf).cpu(), ref.int())
    f_only, none = _frame_mask(lib, mask_d, B, N, Tf, ks, ss, want_i=False)
    assert none is None and torch.equal(f_only, maskf)
    none, i_only = _frame_mask(lib, mask_d, B, N, Tf, ks, ss, want_f=False)
    assert none is None and torch.equal(i_only, mask32)
    allf, alli = _frame_mask(lib, None, B, N, Tf, ks, ss)
    assert torch.equal(allf, torch.ones(B * Tf, device=DEV)) and torch.equal(alli, torch.ones_like(alli))


def test_frame_mask_wrapper(lib):
    """wav2vec2.frame_mask (what the encoder calls) on the mini stack."""
    from speech_transcript_embeddings_amd import wav2vec2
    ks, ss, N, Tf, sums = FRAME_STACKS["mini"]
    mask = _sample_mask(sums, N)
    maskf, mask32 = wav2vec2.frame_mask(SimpleNamespace(conv_kernel=ks, conv_stride=ss), mask.to(DEV), len(sums), N,
                                        Tf, DEV)
    ref = w2v2_frame_mask_ref(mask, Tf, ks, ss)
    assert torch.equal(maskf.view(-1, Tf).cpu(), ref.float()) and torch.equal(mask32.view(-1, Tf).cpu(), ref.int())


def _wave_norm_ref(x, lens, pad):
    out = np.full(x.shape, pad, np.float64)
    for b, n in enumerate(lens):
        n = min(int(n), x.shape[1])
        if n > 0:
            v = x[b, :n].astype(np.float64)
            out[b, :n] = (v - v.mean()) / np.sqrt(v.var() + 1e-7)
    return out


@pytest.mark.parametrize("with_lengths", [True, False])
def test_wave_norm(lib, with_lengths):
    """Wav2Vec2FeatureExtractor(do_normalize=True) through wav2vec2.wave_normalize: lengths clamped
    to N, a single sample -> 0, an empty clip -> all pad, lengths = NULL, a row stride past N, and
    a clip with mean 50 / std 0.01 (bounded by fp32 torch's own error on it, times 10)."""
    from speech_transcript_embeddings_amd import wav2vec2
    torch.manual_seed(21)
    B, N, ldw, pad = 5, 1000, 1024, -1.5
    big = torch.randn(B, ldw)
    big[1] = 50 + 0.01 * torch.randn(ldw)
    lens = [1000, 777, 1, 0, 5000] if with_lengths else [N] * B
    ref = torch.from_numpy(_wave_norm_ref(big[:, :N].numpy(), lens, pad))
    out = wav2vec2.wave_normalize(big.to(DEV)[:, :N], torch.tensor(lens) if with_lengths else None, pad=pad).cpu()
    for b in range(B):
        n = min(lens[b], N)
        assert torch.equal(out[b, n:], torch.full((N - n,), pad)), b          # the pad region is a pure move
        if n < 2:
            assert torch.count_nonzero(out[b, :n]) == 0, b                     # one sample: exactly 0
        elif b == 1:
            v = big[b, :n]
            t32 = (v - v.mean()) / torch.sqrt(v.var(unbiased=False) + 1e-7)
            _margin(_rel(out[b, :n], ref[b, :n]), _rel(t32, ref[b, :n]), f"wave_norm mean-50 clip, {n} samples")
        else:
            assert _rel(out[b, :n], ref[b, :n]) < F32_TOL, b


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_drop_rows(lib, p):
    """x[r, c] *= keep(seed, r·N + c)/(1 - p) · maskf[r] in place: the zero pattern of the numpy
    copy of the hash (kref.drop_scale), kept values to 1e-6, p = 0 with a mask exactly x·maskf[r];
    and the same keep mask as the GEMM epilogue's dropout on an [M, N] output (the header's claim)."""
    from speech_transcript_embeddings_amd import ops
    torch.manual_seed(31)
    M, N, seed = 37, 100, 0x9E3779B97F4A7C15
    x = torch.randn(M, N).abs() + 0.1
    maskf = (torch.rand(M) < 0.7).float()
    p32 = float(np.float32(p))                     # the kernel receives p as a float
    scale = torch.from_numpy(drop_scale(seed, np.arange(M * N, dtype=np.uint64), p32)).view(M, N)
    maskf_d = maskf.to(DEV)
    for m in (None, maskf):
        out = x.to(DEV)
        lib.call("ste_w2v_drop_rows", _p(out), M, N, p, seed, None if m is None else _p(maskf_d), _s(lib))
        ref = x.double() * scale.double() * (1.0 if m is None else m.double()[:, None])
        assert torch.equal(out.cpu() == 0, ref == 0), "zero pattern"
        assert _rel(out, ref) < F32_TOL
        if p == 0.0:
            assert torch.equal(out.cpu(), x if m is None else x * m[:, None])
    if p > 0:
        ones = torch.ones(M, N, device=DEV)
        lib.call("ste_w2v_drop_rows", _p(ones), M, N, p, seed, None, _s(lib))
        a = torch.ones(M, 8, device=DEV, dtype=BF16)
        w = torch.ones(N, 8, device=DEV, dtype=BF16)
        y = ops.linear(a, w, drop_p=p, seed=seed)
        assert torch.equal(y != 0, ones != 0)
        assert 0 < int((ones == 0).sum()) < M * N
