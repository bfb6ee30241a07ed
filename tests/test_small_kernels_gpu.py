"""Unit parity of the small C-ABI kernels that the model tests otherwise reach only inside a whole
step: SpecAugment row masking, the in-batch InfoNCE, the epoch pair metrics, the small fp32
row-matrix product, strided axpby, the fp32 -> bf16 cast, the strided 2-D copy, the row scaling
and the int64 mask conversion — each against a float64 torch reference of the contract
include/ste.h states for it (pure moves and single fp32 operations: bit-exact)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops as _ops
    return _ops


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("rows,cols", [(999, 1024), (64, 160)])
def test_spec_mask_fwd_bwd(ops, rows, cols):
    """ste_spec_mask_fwd / _bwd (tf:…wav2vec2_bert…:944-988): masked valid rows take the embedding;
    the backward sums their gradient rows into dembed (fixed order: bitwise repeatable) and zeroes them."""
    torch.manual_seed(rows)
    x = torch.randn(rows, cols, device=DEV)
    spec = (torch.rand(rows, device=DEV) < 0.3).int()
    valid = (torch.rand(rows, device=DEV) < 0.85).float()
    emb = torch.randn(cols, device=DEV)
    sel = (spec != 0) & (valid != 0)
    y = x.clone()
    ops.spec_mask_fwd(y, spec, valid, emb)
    assert torch.equal(y[sel], emb.expand(int(sel.sum()), cols)) and torch.equal(y[~sel], x[~sel])
    dx = torch.randn(rows, cols, device=DEV)
    outs = []
    for _ in range(2):
        d = dx.clone()
        de = torch.zeros(cols, device=DEV)
        ops.spec_mask_bwd(d, spec, valid, de)
        outs.append((d, de))
    assert torch.equal(outs[0][1], outs[1][1])
    d, de = outs[0]
    assert _rel(de, dx[sel].double().sum(0)) < 1e-6
    assert torch.count_nonzero(d[sel]) == 0 and torch.equal(d[~sel], dx[~sel])


@pytest.mark.parametrize("B,NB,row0", [(37, 100, 20), (64, 64, 0)])
def test_inbatch_ce(ops, B, NB, row0):
    """ste_inbatch_ce: loss += weight/B Σ_i CE(S[i, :NB]/τ, row0+i); dS = weight·gs/B·(softmax − onehot)/τ."""
    torch.manual_seed(B + NB)
    tau, weight, gs = 0.07, 0.5, 2.0
    ld = NB + 24                                  # a row stride past NB: the extra columns are ignored
    S = torch.randn(B, ld, device=DEV) * 0.3
    loss = torch.full((1,), 1.25, device=DEV)
    dS = torch.full((B, NB), 9.0, device=DEV)
    ops.inbatch_ce(S, B, NB, row0, tau, weight, torch.tensor([gs], device=DEV), loss, dS)
    Sd = S[:, :NB].double().clone().requires_grad_()
    tgt = torch.arange(B, device=DEV) + row0
    ref = weight * torch.nn.functional.cross_entropy(Sd / tau, tgt, reduction="sum") / B
    ref.backward()
    r = ref.item()
    assert abs(float(loss[0]) - (1.25 + r)) < 1e-5 * max(1.0, abs(r))
    assert _rel(dS, Sd.grad * gs) < 1e-5


def test_pair_metrics(ops):
    """ste_pair_metrics (ref to_human_readable :924-939, train_epoch :1120-1161): fp64 sums of the
    clean / corrupt sigmoids, s_pos > s_neg, in-batch top-1 hits, rows and the weighted losses."""
    torch.manual_seed(3)
    NB, tau, lw = 77, 0.1, 0.25
    S = torch.randn(NB, 2 * NB + 8, device=DEV)
    S[torch.arange(NB), torch.arange(NB)] += 1.5 * (torch.rand(NB, device=DEV) < 0.6)
    losses = torch.rand(5, device=DEV)
    acc = torch.zeros(6, device=DEV, dtype=torch.float64)
    ops.pair_metrics(S, NB, tau, acc, losses=losses, loss_w=lw)
    Sd = S.double()
    sp, sn = Sd.diagonal()[:NB], Sd[torch.arange(NB), NB + torch.arange(NB)]
    want = torch.stack([torch.sigmoid(sp / tau).sum(), torch.sigmoid(sn / tau).sum(), (sp > sn).double().sum(),
                        (Sd[:, :NB].argmax(1) == torch.arange(NB, device=DEV)).double().sum(),
                        torch.tensor(float(NB), device=DEV, dtype=torch.float64), lw * losses.double().sum()])
    assert torch.equal(acc[2:5], want[2:5])
    assert torch.allclose(acc[[0, 1, 5]], want[[0, 1, 5]], rtol=1e-6, atol=0)


@pytest.mark.parametrize("R,C,P,tx", [(64, 768, 8, False), (33, 100, 4, True), (1, 256, 12, False)])
def test_rowmat(ops, R, C, P, tx):
    torch.manual_seed(R * C)
    X = torch.randn(C, R, device=DEV) if tx else torch.randn(R, C, device=DEV)
    Y = torch.randn(C, P, device=DEV)
    out = torch.randn(R, P, device=DEV)
    want = out.double() + (X.double().t() if tx else X.double()) @ Y.double()
    ops.rowmat(X, Y, out, transpose_x=tx)
    assert _rel(out, want) < 1e-6


def test_axpby_strided(ops):
    torch.manual_seed(4)
    big_y, big_x = torch.randn(50, 300, device=DEV), torch.randn(50, 260, device=DEV)
    y, x = big_y[:, 10:210], big_x[:, 4:204]       # row strides 300 / 260, 200 columns
    want = 0.75 * x.double() - 2.0 * y.double()
    rest = big_y.clone()
    ops.axpby(y, x, alpha=0.75, beta=-2.0)
    assert _rel(y, want) < 1e-7
    assert torch.equal(big_y[:, :10], rest[:, :10]) and torch.equal(big_y[:, 210:], rest[:, 210:])


def test_cast_bf16_round_to_nearest_even(ops):
    torch.manual_seed(5)
    x = torch.randn(100_003, device=DEV) * 10
    x[:4] = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), 3e38], device=DEV)   # ties, large
    y = torch.empty(x.numel(), device=DEV, dtype=torch.bfloat16)
    ops.cast_bf16(x, y)
    assert torch.equal(y, x.bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_copy2d_values(ops, dtype):
    """ste_copy2d: 4- and 2-byte elements between views of different row strides, 300 columns (more
    than the 256 threads of a row's block); bytes outside the window stay."""
    torch.manual_seed(6)
    big_y = torch.randn(50, 340, device=DEV).to(dtype)
    big_x = torch.randn(50, 310, device=DEV).to(dtype)
    y, x = big_y[:, 10:310], big_x[:, 4:304]       # row strides 340 / 310, 300 columns
    rest = big_y.clone()
    ops.copy2d(y, x)
    assert torch.equal(y, x)
    assert torch.equal(big_y[:, :10], rest[:, :10]) and torch.equal(big_y[:, 310:], rest[:, 310:])


@pytest.mark.parametrize("cols,ld", [(1028, 1032), (7, 12), (8, 10)])
def test_scale_rows_values(cols, ld):
    """ste_scale_rows: x[r, c] *= scale[r] for c < cols (one fp32 multiply: bit-exact) on the 16-B
    vector path (cols and ld multiples of 4; 1028 columns: a second pass of the 256 threads) and
    the scalar path (cols = 7, or ld = 10); columns past cols stay."""
    from speech_transcript_embeddings_amd import _lib
    torch.manual_seed(cols)
    rows = 37
    big = torch.randn(rows, ld, device=DEV)
    sc = torch.randn(rows, device=DEV)
    want = big.clone()
    want[:, :cols] *= sc[:, None]
    assert big.data_ptr() % 16 == 0
    _lib.call("ste_scale_rows", big.data_ptr(), sc.data_ptr(), rows, cols, ld, _lib.stream_ptr())
    assert torch.equal(big, want)


def test_mask_i64_to_f32_values():
    """ste_mask_i64_to_f32: f = (m != 0) as float, i32 = (m != 0) as int32, either output alone."""
    from speech_transcript_embeddings_amd import _lib
    torch.manual_seed(7)
    n = 1000
    m = torch.randint(0, 3, (n,), device=DEV, dtype=torch.int64)
    for want_f, want_i in ((True, True), (True, False), (False, True)):
        f = torch.full((n,), 7.0, device=DEV) if want_f else None
        i32 = torch.full((n,), 7, device=DEV, dtype=torch.int32) if want_i else None
        _lib.call("ste_mask_i64_to_f32", m.data_ptr(), _lib.ptr(f), _lib.ptr(i32), n, _lib.stream_ptr())
        assert f is None or torch.equal(f, (m != 0).float())
        assert i32 is None or torch.equal(i32, (m != 0).int())
