"""Long recordings without a GPU: plan_recording against brute force, best_per_recording
against a Python loop, the ste::attn_pool_seg schema and fake implementation, ops.attn_pool_seg_fwd's
argument errors and the C ABI of ste_attn_pool_seg_fwd[_f32] (declared, exported, in the ctypes table,
contract violations returned before any launch)."""
import ctypes as C
import random

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from speech_transcript_embeddings_amd import torch_ops
from speech_transcript_embeddings_amd.retrieval import ALIGN_MAX_FRAMES, best_per_recording, plan_recording

ERR_ARG, ERR_SHAPE = 1001, 1002
PLANS = [(8, 4, 5, 2), (8, 8, 8, 0), (7, 3, 4, 9), (64, 1, 3, 1)]


# ------------------------------------------------------------------ plan_recording
@pytest.mark.parametrize("window,hop,chunk,context", PLANS)
def test_plan_recording_against_brute_force(window, hop, chunk, context):
    found_long = 0
    for F in range(1, 71):
        p = plan_recording(F, window, hop, chunk, context)
        assert p["frames"] == F
        # the kept ranges partition [0, F) in chunks of `chunk`
        covered = [f for a, b in p["keep"] for f in range(a, b)]
        assert covered == list(range(F))
        assert all(b - a == chunk for a, b in p["keep"][:-1]) and 1 <= p["keep"][-1][1] - p["keep"][-1][0] <= chunk
        assert [a for a, _ in p["keep"]] == [c * chunk for c in range(len(p["keep"]))]
        # the chunk inputs are the clipped widenings
        assert p["input"] == [(max(a - context, 0), min(b + context, F)) for a, b in p["keep"]]
        # the window count and lengths follow the rule
        nwin = 1 if F <= window else (F - window + hop - 1) // hop + 1
        assert p["window_start"] == [i * hop for i in range(nwin)]
        assert p["window_len"] == [min(window, F - s) for s in p["window_start"]]
        assert all(n >= 1 for n in p["window_len"]) and p["window_start"][-1] + p["window_len"][-1] == F
        wins = [(s, s + n) for s, n in zip(p["window_start"], p["window_len"])]

        def inside(a, b):
            return any(s <= a and b <= e for s, e in wins)

        # every span of at most window - hop + 1 frames lies inside a window, by enumeration
        for n in range(1, min(window - hop + 1, F) + 1):
            for a in range(0, F - n + 1):
                assert inside(a, a + n), (F, a, n)
        # and the bound is tight: one frame more fits no window, somewhere, when F allows
        n = window - hop + 2
        if n <= window and nwin > 1 and any(not inside(a, a + n) for a in range(0, F - n + 1)):
            found_long += 1
    if hop > 1:
        assert found_long > 0
    else:                      # hop = 1: window - hop + 2 > window, no longer span could fit a window at all
        assert found_long == 0


def test_plan_recording_tight_bound_example():
    """window 8, hop 4: every 5-frame span is inside a window, the 6-frame span [3, 9) is in none."""
    p = plan_recording(20, 8, 4, 5, 2)
    wins = [(s, s + n) for s, n in zip(p["window_start"], p["window_len"])]
    assert wins == [(0, 8), (4, 12), (8, 16), (12, 20)]
    assert not any(s <= 3 and 9 <= e for s, e in wins)


def test_plan_recording_errors():
    ok = dict(frames=10, window_frames=8, hop_frames=4, chunk_frames=5, context_frames=2)
    plan_recording(**ok)
    for bad in (dict(frames=0), dict(hop_frames=0), dict(hop_frames=9), dict(window_frames=8193, hop_frames=8),
                dict(window_frames=0, hop_frames=0), dict(chunk_frames=0), dict(context_frames=-1)):
        with pytest.raises(ValueError):
            plan_recording(**{**ok, **bad})
    plan_recording(9000, 8192, 8192, 1000, 0)
    with pytest.raises(ValueError, match="2048"):
        plan_recording(9000, ALIGN_MAX_FRAMES + 1, 100, 1000, 0, max_window=ALIGN_MAX_FRAMES)
    plan_recording(9000, ALIGN_MAX_FRAMES, 100, 1000, 0, max_window=ALIGN_MAX_FRAMES)


# ------------------------------------------------------------------ best_per_recording
def _best_loop(values, idx, rec_of, k):
    out = []
    for vrow, irow in zip(values.tolist(), idx.tolist()):
        seen, row = set(), []
        for v, i in zip(vrow, irow):
            if i < 0 or rec_of[i] in seen:
                continue
            seen.add(rec_of[i])
            row.append((v, rec_of[i], i))
        row = (row + [(float("-inf"), -1, -1)] * k)[:k]
        out.append(row)
    return out


@pytest.mark.parametrize("k", [1, 3, 6, 12])
def test_best_per_recording_against_loop(k):
    rng = random.Random(23 + k)
    N, R, Q, m = 40, 5, 16, 9
    rec_of = [rng.randrange(R) for _ in range(N)]
    idx = torch.tensor([[rng.choice([-1] + list(range(N))) for _ in range(m)] for _ in range(Q)], dtype=torch.int32)
    idx[0] = -1                                              # a row of empty slots
    idx[1] = torch.tensor([7] * m, dtype=torch.int32)        # one window repeated
    values = torch.randn(Q, m).sort(1, descending=True)[0]
    vals, recs, wins = best_per_recording(values, idx, torch.tensor(rec_of, dtype=torch.int32), k)
    assert vals.shape == recs.shape == wins.shape == (Q, k)
    assert vals.dtype == torch.float32 and recs.dtype == idx.dtype and wins.dtype == idx.dtype
    want = _best_loop(values, idx, rec_of, k)
    assert vals.tolist() == [[w[0] for w in row] for row in want]
    assert recs.tolist() == [[w[1] for w in row] for row in want]
    assert wins.tolist() == [[w[2] for w in row] for row in want]
    for row in recs.tolist():                                # no recording twice
        live = [r for r in row if r >= 0]
        assert len(live) == len(set(live))
    assert (recs[0] == -1).all() and torch.isneginf(vals[0]).all()
    assert recs[1, 0] == rec_of[7] and (recs[1, 1:] == -1).all()


def test_best_per_recording_errors():
    with pytest.raises(ValueError):
        best_per_recording(torch.zeros(2, 3), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        best_per_recording(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), 0)


# ------------------------------------------------------------------ torch op
def test_op_schema_and_fake():
    assert "attn_pool_seg" in torch_ops.OPS
    s = str(torch.ops.ste.attn_pool_seg.default._schema)
    assert s == ("ste::attn_pool_seg(Tensor t, Tensor w2, Tensor b2, Tensor h, Tensor seg_row, Tensor seg_len) "
                 "-> Tensor"), s
    with FakeTensorMode():
        for dt in (torch.float32, torch.bfloat16):
            t, h = torch.empty(50, 64, dtype=dt), torch.empty(50, 768, dtype=dt)
            out = torch.ops.ste.attn_pool_seg(t, torch.empty(64), torch.empty(1), h,
                                              torch.empty(7, dtype=torch.int64), torch.empty(7, dtype=torch.int32))
            assert out.shape == (7, 768) and out.dtype == torch.float32


# ------------------------------------------------------------------ ops wrapper
def test_ops_attn_pool_seg_fwd_argument_errors():
    """Every refusal comes before the library is touched: the operands live on the CPU here."""
    from speech_transcript_embeddings_amd import ops
    rows, Hh, H, G = 10, 8, 12, 3
    ok = dict(t=torch.zeros(rows, Hh), w2=torch.zeros(Hh), b2=torch.zeros(1), h=torch.zeros(rows, H),
              seg_row=torch.zeros(G, dtype=torch.int64), seg_len=torch.ones(G, dtype=torch.int32))

    def refuse(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.attn_pool_seg_fwd(**{**ok, **kw})

    refuse("rows", t=torch.zeros(rows + 1, Hh))
    refuse("rows", h=torch.zeros(rows, H, 1))
    refuse("rows", t=torch.zeros(0, Hh), h=torch.zeros(0, H))
    refuse("multiples of 4", t=torch.zeros(rows, 6), w2=torch.zeros(6))
    refuse("multiples of 4", h=torch.zeros(rows, 10))
    refuse("float32 or both bfloat16", h=torch.zeros(rows, H, dtype=torch.bfloat16))
    refuse("float32 or both bfloat16", t=torch.zeros(rows, Hh).double(), h=torch.zeros(rows, H).double())
    refuse("w2 and b2", w2=torch.zeros(Hh + 4))
    refuse("w2 and b2", b2=torch.zeros(2))
    refuse("w2 and b2", w2=torch.zeros(Hh, dtype=torch.bfloat16))
    refuse("int64", seg_row=torch.zeros(G, dtype=torch.int32))
    refuse("int32", seg_len=torch.ones(G, dtype=torch.int64))
    refuse(r"\[G\]", seg_row=torch.zeros(G + 1, dtype=torch.int64))
    refuse(r"\[G\]", seg_row=torch.zeros(0, dtype=torch.int64), seg_len=torch.ones(0, dtype=torch.int32))
    refuse("pooled", pooled=torch.zeros(G, H + 4))
    refuse("pooled", pooled=torch.zeros(G, H, dtype=torch.bfloat16))
    refuse("pooled_bf16", pooled_bf16=torch.zeros(G, H))
    refuse("contiguous", h=torch.zeros(rows, 2 * H)[:, :H])
    refuse("GPU")                                              # valid shapes, but no CPU path exists


# ------------------------------------------------------------------ C ABI
@pytest.mark.parametrize("name", ["ste_attn_pool_seg_fwd", "ste_attn_pool_seg_fwd_f32"])
def test_symbol_declared_exported_and_bound(name):
    from pathlib import Path

    from speech_transcript_embeddings_amd import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "ste.h").read_text()
    assert f"int {name}(" in header
    assert name in _lib.SYMBOLS and len(_lib._SIGS[name][1]) == 15 and _lib._SIGS[name][0] is C.c_int
    assert _lib._SIGS[name][1][4] is C.c_int64               # rows: 64-bit
    assert _lib.fn(name) is not None                         # exported by libste.so


@pytest.mark.parametrize("name", ["ste_attn_pool_seg_fwd", "ste_attn_pool_seg_fwd_f32"])
def test_argument_errors_return_status_without_launch(name):
    """No GPU here: a launch would fail differently.  Pointers are never dereferenced."""
    from speech_transcript_embeddings_amd import _lib
    f = _lib.fn(name)
    A = 1 << 20

    def call(t=A, w2=A, b2=A, h=A, rows=100, seg_row=A, seg_len=A, G=3, Hh=64, H=768, score=A, stat=A, pooled=A,
             pooled_bf16=None):
        return f(t, w2, b2, h, rows, seg_row, seg_len, G, Hh, H, score, stat, pooled, pooled_bf16, None)

    for arg in ("t", "w2", "b2", "h", "seg_row", "seg_len", "score", "stat", "pooled"):
        assert call(**{arg: None}) == ERR_ARG, arg
    assert call(G=0) == ERR_SHAPE and call(G=-1) == ERR_SHAPE
    assert call(rows=0) == ERR_SHAPE and call(rows=-5) == ERR_SHAPE
    assert call(Hh=66) == ERR_SHAPE and call(H=770) == ERR_SHAPE
    assert call(Hh=0) == ERR_SHAPE and call(H=0) == ERR_SHAPE
    assert call(G=0, t=None) == ERR_SHAPE                    # the shape is judged first
