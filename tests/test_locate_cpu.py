"""Timestamped search hits without a GPU: the hit-span rule of align.hit_spans against
loops, align_bytes_per_frame, the ste::align_matrix_seg schema and fake implementation, the new
symbol in include/ste.h and _lib.py, and the argument contract of ste_align_matrix_seg_fwd (which
returns before any launch)."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import _lib, torch_ops
from speech_transcript_embeddings_amd.align import hit_spans
from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame, kv_bytes_per_frame

ROOT = Path(__file__).resolve().parent.parent


def test_names_are_exported():
    assert callable(ste.search_clips)
    sig = inspect.signature(ste.AudioStateStore.__init__)
    assert sig.parameters["align_rows"].default is False
    sig = inspect.signature(ste.search_clips)
    assert sig.parameters["rerank"].default is True and sig.parameters["locate"].default is True
    assert sig.parameters["word_ids"].default is None


def _tiling(n, F, L):
    """Spans [L, 2] of n tokens tiling F frames one frame each but the last, (-1, -1) beyond."""
    sp = torch.full((L, 2), -1, dtype=torch.int32)
    for l in range(n):
        sp[l, 0], sp[l, 1] = l, (l + 1 if l < n - 1 else F)
    return sp


def _hit_by_loop(sp, n, lead, trail):
    if n < lead + trail + 1 or sp[0, 0] < 0:
        return [-1, -1]
    return [int(sp[lead, 0]), int(sp[n - 1 - trail, 1])]


@pytest.mark.parametrize("lead,trail", [(1, 1), (0, 0), (2, 1), (0, 3)])
def test_hit_spans_match_loops(lead, trail):
    L = 8
    ns = [0, 1, 2, 3, 4, 7, 8]
    spans = torch.stack([_tiling(n, 20 + n, L) for n in ns])
    ntok = torch.tensor(ns, dtype=torch.int32)
    got = hit_spans(spans, ntok, lead, trail)
    assert got.dtype == torch.int32 and got.shape == (len(ns), 2)
    assert got.tolist() == [_hit_by_loop(spans[i], n, lead, trail) for i, n in enumerate(ns)]


def test_hit_spans_rules():
    L = 6
    sp = _tiling(5, 30, L)                                  # <s> w x y </s>
    assert hit_spans(sp[None], torch.tensor([5])).tolist() == [[1, 4]]
    # n < 3 with the default lead = trail = 1: no phrase token is left
    for n in (0, 1, 2):
        assert hit_spans(_tiling(n, 9, L)[None], torch.tensor([n])).tolist() == [[-1, -1]]
    assert hit_spans(_tiling(3, 9, L)[None], torch.tensor([3])).tolist() == [[1, 2]]      # exactly one phrase token
    assert hit_spans(_tiling(2, 9, L)[None], torch.tensor([2]), 0, 0).tolist() == [[0, 9]]
    # an infeasible pair: the decode left (-1, -1) everywhere
    none = torch.full((1, L, 2), -1, dtype=torch.int32)
    assert hit_spans(none, torch.tensor([5])).tolist() == [[-1, -1]]
    # leading dimensions are kept: [Q, k, L, 2] with ntok [Q, k]
    both = torch.stack([torch.stack([sp, none[0]]), torch.stack([none[0], sp])])
    got = hit_spans(both, torch.tensor([[5, 5], [0, 5]]))
    assert got.shape == (2, 2, 2) and got.tolist() == [[[1, 4], [-1, -1]], [[-1, -1], [1, 4]]]
    with pytest.raises(ValueError):
        hit_spans(sp[None], torch.tensor([5]), -1, 1)


def test_align_bytes_per_frame():
    assert align_bytes_per_frame(768) == 3072 and align_bytes_per_frame(128) == 512
    # one more bf16 K|V row: it doubles a bf16 store's rows and stays bf16 beside an mx8 store's
    assert align_bytes_per_frame(768) == kv_bytes_per_frame(768, "bf16")
    assert kv_bytes_per_frame(768, "mx8") == 1584            # unchanged


def test_align_matrix_seg_schema_and_fake():
    assert "align_matrix_seg" in torch_ops.OPS
    s = str(torch.ops.ste.align_matrix_seg.default._schema).replace("SymInt", "int")
    assert s == ("ste::align_matrix_seg(Tensor q, Tensor qblk, Tensor pseg, Tensor kv, Tensor seg_row, "
                 "Tensor seg_len, int Tmax, int nh) -> (Tensor, Tensor, Tensor)"), s
    with FakeTensorMode():
        i32 = lambda *n: torch.empty(*n, dtype=torch.int32)                       # noqa: E731
        m, e, o = torch.ops.ste.align_matrix_seg(torch.empty(5, 12, 128, dtype=torch.bfloat16), i32(7), i32(7),
                                                 torch.empty(300, 256, dtype=torch.bfloat16),
                                                 torch.empty(4, dtype=torch.int64), i32(4), 49, 4)
        assert m.shape == (7, 12, 49) and m.dtype == torch.float32
        assert e.shape == (7, 49, 12) and e.dtype == torch.float32
        assert o.shape == (7, 12, 128) and o.dtype == torch.bfloat16


def test_symbol_declared_and_bound():
    header = (ROOT / "include" / "ste.h").read_text()
    proto = re.search(r"int ste_align_matrix_seg_fwd\(([^;]*)\);", header)
    assert proto, "ste_align_matrix_seg_fwd is not declared in include/ste.h"
    nargs = len(proto.group(1).split(","))
    assert nargs == 20
    name = "ste_align_matrix_seg_fwd"
    assert name in _lib.SYMBOLS and len(_lib._SIGS[name][1]) == nargs and _lib._SIGS[name][0] is C.c_int
    assert hasattr(_lib.load(), name)


def test_argument_errors_return_before_a_launch():
    """Every NULL / shape / alignment violation comes back as a status; the pointers are never read."""
    f = _lib.fn("ste_align_matrix_seg_fwd")
    ERR_ARG, ERR_SHAPE = 1001, 1002
    A = 4096                                                   # a 16-B aligned address that is never dereferenced

    def call(q=A, ldq=64, qblk=A, pseg=A, kv=A, ldkv=128, seg_row=A, seg_len=A, R=1, G=1, L=3, Tmax=16, P=64, nh=8,
             matrix=A, emit=A, lde=3, out=A, ldo=64):
        return f(q, ldq, qblk, pseg, kv, ldkv, seg_row, seg_len, R, G, L, Tmax, P, nh, matrix, emit, lde, out, ldo,
                 None)

    assert call(matrix=None, emit=None, out=None) == ERR_ARG               # no output requested
    for name in ("q", "qblk", "pseg", "kv", "seg_row", "seg_len"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(Tmax=2049) == ERR_SHAPE and call(Tmax=0) == ERR_SHAPE
    assert call(P=1040, nh=4, ldq=1040, ldkv=2080, ldo=1040) == ERR_SHAPE  # d = 260 > 256
    assert call(P=80, nh=8, ldq=80, ldkv=160, ldo=80) == ERR_SHAPE         # d = 10: not a multiple of 8
    assert call(P=64, nh=7) == ERR_SHAPE                                   # P % nh != 0
    assert call(R=0) == ERR_SHAPE and call(G=0) == ERR_SHAPE and call(L=0) == ERR_SHAPE
    assert call(ldkv=120) == ERR_SHAPE and call(ldkv=132) == ERR_SHAPE     # ldkv < 2P; ldkv % 8 != 0
    assert call(kv=A + 8) == ERR_SHAPE and call(ldq=60) == ERR_SHAPE       # kv not 16-B aligned; ldq < P
    assert call(lde=2) == ERR_SHAPE and call(ldo=60) == ERR_SHAPE          # lde < L; ldo < P
