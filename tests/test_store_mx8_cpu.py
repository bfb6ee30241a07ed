"""The MX-fp8 audio-state store without a GPU: the numpy reading of stored bytes
(tests/kref_mx8.py) against hand-written bytes, the ste::xattn_seg_mx8 schema and fake implementation,
the bytes-per-frame formula, the store's argument errors and the argument contracts of
ste_xattn_seg_mx8_fwd and ste_mx8_dequant (which return before touching the device)."""
import inspect
import types

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import kref_mx8
import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import retrieval, torch_ops


def _deq(byte, scale):
    q = np.zeros((1, 32), dtype=np.uint8)
    q[0, 0] = byte
    return kref_mx8.mx8_dequant(q, np.array([[scale]], dtype=np.uint8))[0, 0], \
        kref_mx8.mx8_dequant_bits(q, np.array([[scale]], dtype=np.uint8))[0, 0]


def test_numpy_dequantiser_on_hand_written_bytes():
    # S.EEEE.MMM, bias 7: 0x7e = 0.1111.110 = 1.75 * 2^8 = 448, the largest; 0xfe = -448
    assert _deq(0x7E, 127) == (448.0, 0x43E0) and _deq(0xFE, 127) == (-448.0, 0xC3E0)
    assert _deq(0x7E, 130)[0] == 3584.0 and _deq(0x7E, 117)[0] == 0.4375
    # 0x38 = 0.0111.000 = 1.0; 0x01 the smallest subnormal 2^-9; 0x08 the smallest normal 2^-6
    assert _deq(0x38, 127) == (1.0, 0x3F80) and _deq(0x01, 127)[0] == 2.0 ** -9 and _deq(0x08, 127)[0] == 2.0 ** -6
    assert _deq(0x07, 127)[0] == 7 * 2.0 ** -9 and _deq(0x81, 128)[0] == -2.0 ** -8
    # NaN bytes and the NaN scale
    assert np.isnan(_deq(0x7F, 127)[0]) and np.isnan(_deq(0xFF, 127)[0]) and np.isnan(_deq(0x38, 255)[0])
    assert _deq(0x7F, 127)[1] == 0x7FC0
    # scale byte 0x00 is 2^-127: a zero block is exact zeros (sign kept), 1.0 becomes the bf16 subnormal 0x0040
    zero = kref_mx8.mx8_dequant_bits(np.zeros((2, 64), dtype=np.uint8), np.zeros((2, 2), dtype=np.uint8))
    assert zero.shape == (2, 64) and not zero.any()
    assert _deq(0x80, 0)[1] == 0x8000 and _deq(0x38, 0) == (2.0 ** -127, 0x0040)
    # below bf16's normal range the value is rounded to nearest even: bf16 subnormals step by 2^-133
    assert _deq(0x01, 0)[1] == 0x0000                       # 2^-136 -> 0
    assert _deq(0x39, 0)[1] == 0x0048                       # 1.125 * 2^-127, exact
    assert _deq(0x09, 0)[1] == 0x0001                       # 1.125 * 2^-133 -> 2^-133
    assert _deq(0x0C, 0)[1] == 0x0002                       # 1.5 * 2^-133: a tie, to the even 2 * 2^-133
    assert _deq(0x0A, 1)[1] == 0x0002                       # 1.25 * 2^-132 = 2.5 * 2^-133: a tie, to even
    assert _deq(0x0E, 1)[1] == 0x0004                       # 1.75 * 2^-132 = 3.5 * 2^-133: a tie, to even
    # the block of a scale: columns 32 .. 63 take the second byte
    q = np.full((1, 64), 0x38, dtype=np.uint8)
    v = kref_mx8.mx8_dequant(q, np.array([[126, 129]], dtype=np.uint8))
    assert (v[0, :32] == 0.5).all() and (v[0, 32:] == 4.0).all()
    assert kref_mx8.same_bf16([0x7FC0, 0x3F80], [0xFFC1, 0x3F80]) and not kref_mx8.same_bf16([0x0000], [0x8000])


def test_every_finite_product_is_exact_in_bf16_above_its_subnormal_range():
    """The exactness argument of §19: 4 significant bits times a power of two."""
    q = np.tile(np.arange(256, dtype=np.uint8), (1, 1))
    for e in (7, 8, 64, 127, 200, 246):
        sc = np.full((1, 8), e, dtype=np.uint8)
        exact = kref_mx8.e4m3_to_float64(q) * 2.0 ** (e - 127)
        got = kref_mx8.mx8_dequant(q, sc)
        keep = ~np.isnan(exact)
        assert np.array_equal(got[keep], exact[keep]), e
    # from 2^128 on the fp32 product is infinite: 448 * 2^120 = 1.75 * 2^128, 240 * 2^120 = 1.875 * 2^127
    big = kref_mx8.mx8_dequant(q, np.full((1, 8), 247, dtype=np.uint8))
    assert np.isinf(big[0, 0x7E]) and big[0, 0x77] == 240 * 2.0 ** 120 and big[0, 0xFE] == -np.inf


def test_xattn_seg_mx8_schema_and_fake():
    assert "xattn_seg_mx8" in torch_ops.OPS
    s = str(torch.ops.ste.xattn_seg_mx8.default._schema).replace("SymInt", "int")
    assert s == ("ste::xattn_seg_mx8(Tensor q, Tensor qrow, Tensor pseg, Tensor k, Tensor v, Tensor ks, Tensor vs, "
                 "Tensor seg_row, Tensor seg_len, Tensor tile_first, Tensor tile_cnt, int nh) -> Tensor"), s
    with FakeTensorMode():
        i32 = lambda *n: torch.empty(*n, dtype=torch.int32)                       # noqa: E731
        u8 = lambda *n: torch.empty(*n, dtype=torch.uint8)                        # noqa: E731
        out = torch.ops.ste.xattn_seg_mx8(torch.empty(5, 64), i32(12), i32(12), u8(300, 64), u8(300, 64), u8(300, 2),
                                          u8(300, 2), torch.empty(4, dtype=torch.int64), i32(4), i32(6), i32(6), 8)
        assert out.shape == (12, 64) and out.dtype == torch.float32
    out = torch.ops.ste.xattn_seg_mx8(torch.empty(5, 64, device="meta"), *(torch.empty(12, dtype=torch.int32, device="meta"),) * 2,
                                      *(torch.empty(300, 64, dtype=torch.uint8, device="meta"),) * 2,
                                      *(torch.empty(300, 2, dtype=torch.uint8, device="meta"),) * 2,
                                      torch.empty(4, dtype=torch.int64, device="meta"),
                                      *(torch.empty(4, dtype=torch.int32, device="meta"),) * 3, 8)
    assert out.device.type == "meta" and out.shape == (12, 64) and out.dtype == torch.float32


def test_bytes_per_frame():
    f = retrieval.kv_bytes_per_frame
    assert f(768) == f(768, "bf16") == 3072 and f(768, "mx8") == 1584
    assert f(768, "mx8") / f(768) == 0.515625                   # for every P: (2P + P/16) / 4P = 33/64
    for P in (64, 128, 1024):
        assert f(P, "mx8") * 64 == f(P) * 33 and f(P, "mx8") == 2 * P + 2 * P // 32
    with pytest.raises(ValueError):
        f(768, "fp8")


def test_store_argument_errors_and_defaults():
    sig = inspect.signature(ste.AudioStateStore.__init__)
    assert sig.parameters["kv_dtype"].default == "bf16"
    assert list(sig.parameters)[:6] == ["self", "model", "device", "index_dtype", "reserve_frames", "kv_dtype"]
    sig = inspect.signature(ste.evaluate_retrieval)
    assert sig.parameters["store_kv_dtype"].default == "bf16"
    fused = types.SimpleNamespace(projection_dim=96, use_cross_modal=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        ste.AudioStateStore(fused, "cpu", kv_dtype="fp8")
    with pytest.raises(ValueError, match="64"):
        ste.AudioStateStore(fused, "cpu", kv_dtype="mx8")          # P % 64 != 0
    # without use_cross_modal no K/V is kept and the argument has no effect
    plain = types.SimpleNamespace(projection_dim=96, use_cross_modal=False)
    st = ste.AudioStateStore(plain, "cpu", kv_dtype="mx8")
    assert st.kv.numel() == 0 and len(st) == 0
    with pytest.raises(ValueError):
        st.kv_rows(0)
    ok = ste.AudioStateStore(types.SimpleNamespace(projection_dim=128, use_cross_modal=True), "cpu", reserve_frames=10,
                             kv_dtype="mx8")
    assert ok.kv.shape == (10, 256) and ok.kv.dtype == torch.uint8 and ok.kv_scales.shape == (10, 8)
    ok.rows = 4                                                   # growth keeps both buffers in step
    ok.kv[:4] = 5
    ok.kv_scales[:4] = 6
    ok._reserve(11)
    assert ok.kv.shape == (20, 256) and ok.kv_scales.shape == (20, 8)
    assert (ok.kv[:4] == 5).all() and (ok.kv_scales[:4] == 6).all()


def test_argument_errors_return_before_a_launch():
    """Every shape / alignment violation comes back as STE_ERR_SHAPE; the pointers are never read."""
    from speech_transcript_embeddings_amd import _lib
    f = _lib.fn("ste_xattn_seg_mx8_fwd")
    ERR_SHAPE = 1002
    A = 4096                                                   # an aligned address that is never dereferenced

    def call(k=A, v=A + 64, ldkv=128, ks=A, vs=A + 2, lds=4, ntile=1, R=1, G=1, P=64, nh=8, out=A):
        return f(A, A, A, k, v, ldkv, ks, vs, lds, A, A, A, A, ntile, R, G, P, nh, 0.35, out, None)

    assert call(P=80, nh=10, ldkv=160, lds=5) == ERR_SHAPE     # dh = 8, but P % 32 != 0
    assert call(P=48, nh=6) == ERR_SHAPE
    assert call(P=64, nh=7) == ERR_SHAPE and call(P=2048, nh=8, ldkv=4096, lds=128) == ERR_SHAPE
    assert call(R=0) == ERR_SHAPE and call(G=0) == ERR_SHAPE and call(ntile=0) == ERR_SHAPE
    assert call(ldkv=60) == ERR_SHAPE and call(ldkv=132) == ERR_SHAPE    # ldkv < P; ldkv % 8 != 0
    assert call(k=A + 4) == ERR_SHAPE and call(v=A + 68) == ERR_SHAPE    # 8-byte alignment of the bytes
    assert call(out=A + 4) == ERR_SHAPE and call(lds=1) == ERR_SHAPE and call(ks=None) == ERR_SHAPE
    g = _lib.fn("ste_mx8_dequant")
    for rows, K, ldq in ((0, 128, 128), (1, 32, 32), (1, 192, 192), (1, 128, 120), (1, 128, 132)):
        assert g(A, ldq, rows, K, A, A, None) == ERR_SHAPE, (rows, K, ldq)
    assert g(A + 4, 128, 1, 128, A, A, None) == ERR_SHAPE and g(A, 128, 1, 128, A, A + 8, None) == ERR_SHAPE
