"""Kernel parity of the word-timestamp kernels (csrc/align_infer.hip), each entry point
alone against tests/kref_align.py.

ste_align_decode is BIT-exact against viterbi_ref: both sides do the same single fp32 add per cell
and the same strict comparison, so spans and score are compared with array_equal.  Which shape
reaches which branch: L <= 64 is the one-token-per-lane kernel, L > 64 the four-token one (64 | 65);
L = 256 with lde = 256 takes its 16-byte row loads with every lane live, L = 65 in lde = 68 takes
them with a lane straddling L and lanes past it, L = 65 / 70 in an odd lde the scalar loads; T = 150
and 300 run the 8-row pipeline's whole chunks and a ragged tail (149 and 299 steps = 18·8 + 5 and
37·8 + 3), T = 1 and 5 only the tail; T = 2048 with L > 64 is the LDS limit (64 KiB of advance
bits).  Every call checks a guard region after spans and score.

ste_align_matrix_fwd follows tests/test_heads_optim_kernels_gpu.py: the matrix against float64 under
the margin rule max(1e-6, 10·e32), e32 the same formula in fp32 torch; out under _assert_bf16_close;
emit against the float64 log of the kernel's own matrix within 2^-21·max(1, |value|) (4 fp32 ulp).
"""
import numpy as np
import pytest
import torch

from kref_align import align_matrix_ref, emit_ref, planted, viterbi_batch_ref
from test_w2v2_kernels_gpu import BF16, DEV, ERR_SHAPE, F32, _assert_bf16_close, _margin, _p, _rel, _s

pytestmark = pytest.mark.gpu
I32 = torch.int32
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops():
    from speech_transcript_embeddings_amd import ops
    return ops


def _lds_limit():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).shared_memory_per_block)


# ------------------------------------------------------------------ decode
def _decode(lib, emit, L, ntok, nfrm):
    """ste_align_decode on emit (numpy float32 [B, T, lde]) -> (spans [B, L, 2], score [B]) as numpy;
    the GUARD elements after each output must come back untouched."""
    B, T, lde = emit.shape
    e = torch.from_numpy(np.ascontiguousarray(emit)).to(DEV)
    nt = torch.tensor(list(ntok), dtype=I32, device=DEV)
    nf = torch.tensor(list(nfrm), dtype=I32, device=DEV)
    spans = torch.full((B * L * 2 + GUARD,), 77, dtype=I32, device=DEV)
    score = torch.full((B + GUARD,), 7.0, dtype=F32, device=DEV)
    rc = lib.fn("ste_align_decode")(_p(e), lde, _p(nt), _p(nf), B, L, T, _p(spans), _p(score), _s(lib))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((spans[B * L * 2:] == 77).all()) and bool((score[B:] == 7.0).all())
    return spans[:B * L * 2].view(B, L, 2).cpu().numpy(), score[:B].cpu().numpy()


def _check(lib, emit, L, ntok, nfrm):
    spans, score = _decode(lib, emit, L, ntok, nfrm)
    rs, rsc = viterbi_batch_ref(emit, ntok, nfrm, L)
    assert np.array_equal(spans, rs), np.argwhere(spans != rs)[:5]
    assert np.array_equal(score.view(np.int32), rsc.view(np.int32)), (score, rsc)     # the same bits
    return spans, score


def _diag(n, F):
    return np.zeros(F, dtype=np.int64) if F == 1 else (np.arange(F) * (n - 1)) // (F - 1)


def _emissions(kind, L, T, n, F, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-8, 1, (T, L)).astype(np.float32)
    if kind == "normal":
        return rng.standard_normal((T, L)).astype(np.float32)
    if kind == "zeros":
        return np.zeros((T, L), dtype=np.float32)
    if kind == "band":      # -inf off a band of +-2 tokens round the diagonal path, which keeps it feasible
        e = rng.standard_normal((T, L)).astype(np.float32)
        centre = np.zeros(T, dtype=np.int64)
        centre[:F] = _diag(n, F)
        e[np.abs(np.arange(L)[None, :] - centre[:, None]) > 2] = -np.inf
        return e
    assert kind == "planted"
    return planted(L, T, n, F, seed)[0]


# (L, T, n, F): see the module docstring
SHAPES = [(1, 1, 1, 1), (5, 5, 5, 5), (64, 150, 64, 150), (65, 150, 65, 149), (256, 300, 256, 300),
          (70, 2048, 50, 2048), (8, 2048, 8, 2048)]


@pytest.mark.parametrize("kind", ["int", "normal", "zeros", "band", "planted"])
@pytest.mark.parametrize("L,T,n,F", SHAPES)
def test_decode_matches_reference_bitwise(lib, L, T, n, F, kind):
    e = _emissions(kind, L, T, n, F, seed=L * 31 + T)
    spans, score = _check(lib, e[None], L, [n], [F])
    assert spans[0, 0, 0] == 0 and spans[0, n - 1, 1] == F and (spans[0, n:] == -1).all()
    assert np.array_equal(spans[0, 1:n, 0], spans[0, :n - 1, 1])            # the spans tile [0, F)
    if kind == "planted":
        assert np.array_equal(spans[0, :n], planted(L, T, n, F, L * 31 + T)[1]) and score[0] == 0.0
    if kind == "zeros" and F > n:
        assert spans[0, :n, 1].tolist() == list(range(1, n)) + [F]          # a tie stays: earliest advance
    if n == F:
        assert spans[0, :n, 0].tolist() == list(range(n))                   # only the diagonal exists


def test_decode_ragged_batch(lib):
    """B = 4: a plain pair, an infeasible one (F < n), n = 1 and n = F."""
    L, T = 9, 20
    e = np.random.default_rng(5).standard_normal((4, T, L)).astype(np.float32)
    spans, score = _check(lib, e, L, [5, 9, 1, 7], [20, 4, 13, 7])
    assert (spans[1] == -1).all() and np.isneginf(score[1])
    assert spans[2, 0].tolist() == [0, 13] and (spans[2, 1:] == -1).all()
    # the other infeasible kinds: no token, more tokens than columns, more frames than rows
    spans, score = _check(lib, e[:3], L, [0, 10, 3], [5, 20, 21])
    assert (spans == -1).all() and np.isneginf(score).all()


@pytest.mark.parametrize("L,lde", [(64, 67), (65, 68), (70, 73)])
def test_decode_ignores_padding_columns(lib, L, lde):
    """Columns L..lde-1 hold a sentinel that would win every comparison if it were a token."""
    T, n, F = 40, L - 3, 37
    e = np.full((2, T, lde), 1e30, dtype=np.float32)
    e[:, :, :L] = np.random.default_rng(L).standard_normal((2, T, L)).astype(np.float32)
    spans, score = _check(lib, e, L, [n, L], [F, T])
    dense, dscore = _decode(lib, np.ascontiguousarray(e[:, :, :L]), L, [n, L], [F, T])
    assert np.array_equal(spans, dense) and np.array_equal(score, dscore)


@pytest.mark.parametrize("L", [40, 130])
def test_decode_pair_is_independent_of_the_batch(lib, L):
    T = 90
    e = np.random.default_rng(L).standard_normal((5, T, L)).astype(np.float32)
    ntok, nfrm = [L, 7, L - 9, 1, 30], [T, 50, 77, 3, 64]
    spans, score = _check(lib, e, L, ntok, nfrm)
    for b in (0, 2):
        one, s1 = _decode(lib, e[b:b + 1], L, [ntok[b]], [nfrm[b]])
        assert np.array_equal(one[0], spans[b]) and s1[0].tobytes() == score[b].tobytes()
    perm = [4, 2, 0, 3, 1]
    ps, psc = _decode(lib, e[perm], L, [ntok[i] for i in perm], [nfrm[i] for i in perm])
    assert np.array_equal(ps, spans[perm]) and psc.tobytes() == score[perm].tobytes()


def test_decode_limits(lib):
    t = torch.zeros(1 << 12, device=DEV)
    n = torch.ones(4, dtype=I32, device=DEV)
    f = lib.fn("ste_align_decode")
    assert f(_p(t), 257, _p(n), _p(n), 1, 257, 4, _p(t), _p(t), _s(lib)) == ERR_SHAPE
    assert f(_p(t), 1, _p(n), _p(n), 1, 1, 2049, _p(t), _p(t), _s(lib)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_ops_wrapper_and_custom_op(ops):
    L, T = 12, 33
    e = np.random.default_rng(2).standard_normal((3, T, L + 4)).astype(np.float32)
    ntok, nfrm = [12, 4, 9], [33, 20, 9]
    rs, rsc = viterbi_batch_ref(e, ntok, nfrm, L)
    ed = torch.from_numpy(e).to(DEV)
    nt, nf = torch.tensor(ntok, dtype=I32, device=DEV), torch.tensor(nfrm, dtype=I32, device=DEV)
    spans, score = ops.align_decode(ed[:, :, :L], nt, nf)                    # a column view: lde = L + 4
    assert np.array_equal(spans.cpu().numpy(), rs) and np.array_equal(score.cpu().numpy(), rsc)
    spans, score = torch.ops.ste.align_decode(ed[:, :, :L], nt.long(), nf.long())
    assert spans.dtype == I32 and np.array_equal(spans.cpu().numpy(), rs) and np.array_equal(score.cpu().numpy(), rsc)


# ------------------------------------------------------------------ matrix
def _matrix_case(ops, B, L, T, P, nh, masked):
    what = f"align_matrix B={B} L={L} T={T} P={P} mask={masked}"
    torch.manual_seed(L * 1000 + T + P)
    qb, kvb = torch.randn(B * L, P + 8).bfloat16(), torch.randn(B * T, 2 * P + 8).bfloat16()
    q, kv = qb[:, :P], kvb[:, :2 * P]
    kmask = None
    if masked:                                       # a prefix mask on the last clip (never a whole clip)
        kmask = torch.ones(B, T, dtype=I32)
        kmask[B - 1, T - max(1, T // 3):] = 0
    km = None if kmask is None else kmask.view(-1)
    mref, oref = align_matrix_ref(q, kv, km, B, L, T, P, nh)
    m32, _ = align_matrix_ref(q, kv, km, B, L, T, P, nh, dt=F32)
    q_d, kv_d = qb.to(DEV)[:, :P], kvb.to(DEV)[:, :2 * P]
    km_d = None if km is None else km.to(DEV)
    lde = L + 3

    def run(want):
        matrix = torch.full((B, L, T), 7.0, device=DEV) if "m" in want else None
        emit = torch.full((B, T, lde), 7.0, device=DEV) if "e" in want else None
        outb = torch.full((B * L, P + 16), 7.0, device=DEV, dtype=BF16) if "o" in want else None
        ops.align_matrix_fwd(q_d, kv_d, km_d, B, L, T, nh, matrix=matrix, emit=None if emit is None else emit[:, :, :L],
                             out=None if outb is None else outb[:, :P])
        return matrix, emit, outb

    matrix, emit, outb = run("meo")
    _margin(_rel(matrix, mref), _rel(m32, mref), what + " matrix")
    assert float((matrix.double().sum(-1) - 1).abs().max()) <= 1e-5
    if masked:
        dead = (kmask == 0).to(DEV)[:, None, :].expand(B, L, T)
        assert float(matrix[dead].abs().max()) == 0.0
    want = emit_ref(matrix)                                                   # frame-major [B, T, L]
    got = emit[:, :, :L].double().cpu()
    assert bool(torch.isfinite(got).all())
    excess = (got - want).abs() - 2.0 ** -21 * want.abs().clamp_min(1.0)
    assert float(excess.max()) <= 0, (what, float(excess.max()))
    assert float((emit[:, :, L:] - 7.0).abs().max()) == 0.0
    _assert_bf16_close(outb[:, :P], oref, what + " out")
    assert float((outb[:, P:].float() - 7.0).abs().max()) == 0.0
    for sub in ("m", "e", "o", "me", "mo", "eo"):
        m2, e2, o2 = run(sub)
        assert m2 is None or torch.equal(m2, matrix), sub
        assert e2 is None or torch.equal(e2, emit), sub
        assert o2 is None or torch.equal(o2, outb), sub
    return matrix, outb, q_d, kv_d, km_d


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,L,T,P", [(2, 9, 17, 32), (1, 70, 300, 768)])
def test_align_matrix(ops, B, L, T, P, masked):
    """d = 8 with a query group of one (L = 9) and a ragged key tail; d = 192 with T = 300 longer than
    the 256-thread key loop and L = 70 (a last group of 6)."""
    matrix, outb, q_d, kv_d, km_d = _matrix_case(ops, B, L, T, P, 4, masked)
    # the attention output is the training kernel's at drop_p = 0, bit for bit
    probs = torch.empty(B * 4 * L * T, device=DEV)
    old = torch.empty(B * L, P, device=DEV, dtype=BF16)
    ops.align_attn_fwd(q_d, kv_d, km_d, B, L, T, 4, probs, old)
    assert torch.equal(old, outb[:, :P])


@pytest.mark.parametrize("masked", [False, True])
def test_align_matrix_limit(ops, lib, masked):
    """T = 2048, the largest accepted: 2·8·T·4 B of dynamic LDS (score rows and the running head sum)
    on top of 8 KiB static must fit the per-block limit the runtime reports; T = 2049 is refused."""
    T = 2048
    assert _lds_limit() >= 2 * 8 * T * 4 + 8 * 1024, _lds_limit()
    _matrix_case(ops, 1, 3, T, 64, 4, masked)
    t = torch.zeros(1 << 16, device=DEV)
    assert lib.fn("ste_align_matrix_fwd")(_p(t), 64, _p(t), 128, None, 1, 3, T + 1, 64, 4, _p(t), _p(t), 3, _p(t), 64,
                                          _s(lib)) == ERR_SHAPE
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_align_matrix_custom_op(ops):
    torch.manual_seed(9)
    B, L, T, P, nh = 2, 5, 21, 32, 4
    q, kv = torch.randn(B, L, P).bfloat16(), torch.randn(B, T, 2 * P).bfloat16()
    kmask = torch.ones(B, T, dtype=torch.int64)
    kmask[1, 15:] = 0
    m, e, o = torch.ops.ste.align_matrix(q.to(DEV), kv.to(DEV), kmask.to(DEV), nh)
    mref, oref = align_matrix_ref(q.view(B * L, P), kv.view(B * T, 2 * P), kmask.view(-1), B, L, T, P, nh)
    assert m.shape == (B, L, T) and e.shape == (B, T, L) and o.shape == (B, L, P) and o.dtype == BF16
    assert _rel(m, mref) < 1e-6
    assert float((e.double().cpu() - emit_ref(m)).abs().max()) <= 2.0 ** -21 * 88
    _assert_bf16_close(o.view(B * L, P), oref, "custom op out")
