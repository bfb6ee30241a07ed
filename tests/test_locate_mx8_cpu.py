"""MX-fp8 alignment rows without a GPU: align_bytes_per_frame with its align_dtype, the
exported names, the ste::align_matrix_seg_mx8 schema and fake implementation, the new symbol in
include/ste.h and _lib.py, and the argument contract of ste_align_matrix_seg_mx8_fwd (which returns
before any launch)."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import _lib, ops, torch_ops
from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame, kv_bytes_per_frame

ROOT = Path(__file__).resolve().parent.parent
NAME = "ste_align_matrix_seg_mx8_fwd"


def test_align_bytes_per_frame():
    assert align_bytes_per_frame(768) == 3072                     # the one-argument call keeps its value
    assert align_bytes_per_frame(768, "bf16") == 3072
    assert align_bytes_per_frame(768, "mx8") == 1584 == kv_bytes_per_frame(768, "mx8")
    assert align_bytes_per_frame(128, "mx8") == 256 + 8
    # the table of the store's rows at P = 768: bytes per frame
    assert kv_bytes_per_frame(768, "mx8") + align_bytes_per_frame(768, "mx8") == 3168
    assert kv_bytes_per_frame(768, "mx8") + align_bytes_per_frame(768) == 4656
    with pytest.raises(ValueError, match="align_dtype"):
        align_bytes_per_frame(768, "fp8")


def test_names_are_exported():
    sig = inspect.signature(ste.AudioStateStore.__init__)
    assert sig.parameters["align_dtype"].default == "bf16"
    assert sig.parameters["align_rows"].default is False and sig.parameters["kv_dtype"].default == "bf16"
    assert callable(ops.align_matrix_seg_fwd)              # one entry for both row dtypes: scales= selects MX-fp8
    names = list(inspect.signature(ops.align_matrix_seg_fwd).parameters)
    assert names == ["q", "qblk", "pseg", "kv", "seg_row", "seg_len", "L", "Tmax", "nh", "scales", "matrix", "emit",
                     "out"]
    # the callers gain no argument
    assert "align_dtype" not in inspect.signature(ste.search_clips).parameters


def test_align_matrix_seg_mx8_schema_and_fake():
    assert "align_matrix_seg_mx8" in torch_ops.OPS
    s = str(torch.ops.ste.align_matrix_seg_mx8.default._schema).replace("SymInt", "int")
    assert s == ("ste::align_matrix_seg_mx8(Tensor q, Tensor qblk, Tensor pseg, Tensor kv, Tensor scales, "
                 "Tensor seg_row, Tensor seg_len, int Tmax, int nh) -> (Tensor, Tensor, Tensor)"), s
    with FakeTensorMode():
        i32 = lambda *n: torch.empty(*n, dtype=torch.int32)                       # noqa: E731
        m, e, o = torch.ops.ste.align_matrix_seg_mx8(torch.empty(5, 12, 128, dtype=torch.bfloat16), i32(7), i32(7),
                                                     torch.empty(300, 256, dtype=torch.uint8),
                                                     torch.empty(300, 8, dtype=torch.uint8),
                                                     torch.empty(4, dtype=torch.int64), i32(4), 49, 4)
        assert m.shape == (7, 12, 49) and m.dtype == torch.float32
        assert e.shape == (7, 49, 12) and e.dtype == torch.float32
        assert o.shape == (7, 12, 128) and o.dtype == torch.bfloat16


def test_symbol_declared_and_bound():
    header = (ROOT / "include" / "ste.h").read_text()
    proto = re.search(r"int ste_align_matrix_seg_mx8_fwd\(([^;]*)\);", header)
    assert proto, f"{NAME} is not declared in include/ste.h"
    nargs = len(proto.group(1).split(","))
    assert nargs == 22
    assert NAME in _lib.SYMBOLS and len(_lib._SIGS[NAME][1]) == nargs and _lib._SIGS[NAME][0] is C.c_int
    assert hasattr(_lib.load(), NAME)


def test_argument_errors_return_before_a_launch():
    """Every NULL / shape / alignment violation comes back as a status; the pointers are never read."""
    f = _lib.fn(NAME)
    ERR_ARG, ERR_SHAPE = 1001, 1002
    A = 4096                                                   # an aligned address that is never dereferenced

    def call(q=A, ldq=64, qblk=A, pseg=A, kv=A, ldkv=128, scales=A, lds=4, seg_row=A, seg_len=A, R=1, G=1, L=3,
             Tmax=16, P=64, nh=8, matrix=A, emit=A, lde=3, out=A, ldo=64):
        return f(q, ldq, qblk, pseg, kv, ldkv, scales, lds, seg_row, seg_len, R, G, L, Tmax, P, nh, matrix, emit, lde,
                 out, ldo, None)

    assert call(matrix=None, emit=None, out=None) == ERR_ARG               # no output requested
    for name in ("q", "qblk", "pseg", "kv", "scales", "seg_row", "seg_len"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(Tmax=2049) == ERR_SHAPE and call(Tmax=0) == ERR_SHAPE
    assert call(P=1040, nh=4, ldq=1040, ldkv=2080, lds=65, ldo=1040) == ERR_SHAPE   # d = 260 > 256
    assert call(P=160, nh=16, ldq=160, ldkv=320, lds=10, ldo=160) == ERR_SHAPE      # d = 10: not a multiple of 8
    assert call(P=48, nh=2, ldq=48, ldkv=96, lds=3, ldo=48) == ERR_SHAPE            # P % 32 != 0 (d = 24 is fine)
    assert call(P=64, nh=7) == ERR_SHAPE                                   # P % nh != 0
    assert call(R=0) == ERR_SHAPE and call(G=0) == ERR_SHAPE and call(L=0) == ERR_SHAPE
    assert call(ldkv=120) == ERR_SHAPE and call(ldkv=132) == ERR_SHAPE     # ldkv < 2P; ldkv % 8 != 0
    assert call(kv=A + 4) == ERR_SHAPE and call(ldq=60) == ERR_SHAPE       # kv not 8-B aligned; ldq < P
    assert call(lds=3) == ERR_SHAPE                                        # lds < 2P/32
    assert call(lde=2) == ERR_SHAPE and call(ldo=60) == ERR_SHAPE          # lde < L; ldo < P
    assert call(Tmax=2048, ldkv=1 << 20) == ERR_SHAPE                      # Tmax·ldkv + 2P >= 2^31
    assert call(Tmax=2048, lds=1 << 20) == ERR_SHAPE                       # Tmax·lds + 2P/32 >= 2^31
