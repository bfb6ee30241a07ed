"""retrieval.RowBank, the unit an AudioStateStore keeps its K|V rows in, and the host helpers
beside it, without a GPU: the bank's write / reserve / shapes / errors / byte counts, the store's kv* / akv*
properties over its two banks, Engine's candidate check, and the dtype-specific argument checks of the merged
ops.xattn_seg_fwd / ops.align_matrix_seg_fwd (which assert before any library call)."""
import types

import pytest
import torch

import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import ops
from speech_transcript_embeddings_amd.engine import _candidates
from speech_transcript_embeddings_amd.retrieval import RowBank

BF16, U8, I32, I64 = torch.bfloat16, torch.uint8, torch.int32, torch.int64
P, B, T = 64, 3, 5


def _src():
    return (torch.arange(B * T * 2 * P, dtype=torch.float32).view(B * T, 2 * P) % 251 - 125).to(BF16)


def test_bf16_write_of_ragged_clips():
    src, frames = _src(), [5, 2, 4]
    bank = RowBank(P, "bf16", 20, "cpu")
    assert bank.data.shape == (20, 2 * P) and bank.data.dtype == BF16 and bank.scales is None
    bank.data.fill_(-7)
    bank.write(3, src, frames, T)
    at = 3
    for b, n in enumerate(frames):                       # each clip's prefix rows at the running offset
        assert torch.equal(bank.data[at:at + n], src[b * T:b * T + n]), b
        assert torch.equal(bank.rows(at, at + n), src[b * T:b * T + n]) and bank.rows(at, at + n).data_ptr() \
            == bank.data[at].data_ptr()                  # a view
        at += n
    assert at == 14 and (bank.data[:3] == -7).all() and (bank.data[14:] == -7).all()    # nothing else is touched


def test_bf16_write_of_full_length_clips():
    src = _src()
    bank = RowBank(P, "bf16", 20, "cpu")
    bank.data.fill_(-7)
    bank.write(2, src, [T] * B, T)
    assert torch.equal(bank.data[2:2 + B * T], src)
    assert (bank.data[:2] == -7).all() and (bank.data[2 + B * T:] == -7).all()


def test_reserve_doubles_and_keeps_the_used_rows():
    bank = RowBank(P, "mx8", 10, "cpu")
    bank.data[:4], bank.scales[:4] = 5, 6
    data, scales = bank.data, bank.scales
    bank.reserve(10, 4)                                                  # enough: nothing moves
    assert bank.data is data and bank.scales is scales
    bank.reserve(11, 4)
    assert bank.data.shape == (20, 2 * P) and bank.scales.shape == (20, 2 * P // 32)
    assert (bank.data[:4] == 5).all() and (bank.scales[:4] == 6).all()
    bank.reserve(100, 4)                                                 # past the double: what was asked for
    assert bank.data.shape[0] == bank.scales.shape[0] == 100 and (bank.data[:4] == 5).all()
    bf = RowBank(P, "bf16", 0, "cpu")
    bf.reserve(3, 0)
    assert bf.data.shape == (3, 2 * P) and bf.scales is None


def test_mx8_shapes_and_dtypes():
    bank = RowBank(128, "mx8", 7, "cpu")
    assert bank.dtype == "mx8"
    assert bank.data.shape == (7, 256) and bank.data.dtype == U8
    assert bank.scales.shape == (7, 8) and bank.scales.dtype == U8
    k, v, sc = bank.xattn_operands()
    assert k.shape == v.shape == (7, 128) and sc["ks"].shape == sc["vs"].shape == (7, 4)
    assert v.data_ptr() == bank.data[:, 128:].data_ptr() and sc["vs"].data_ptr() == bank.scales[:, 4:].data_ptr()
    kv, sc = bank.align_operands()
    assert kv is bank.data and sc["scales"] is bank.scales
    bf = RowBank(128, "bf16", 7, "cpu")
    assert bf.xattn_operands()[2] == {} and bf.align_operands() == (bf.data, {})


def test_argument_errors_name_the_callers_argument():
    with pytest.raises(ValueError, match="kv_dtype"):
        RowBank(128, "fp8", 0, "cpu", arg="kv_dtype")
    with pytest.raises(ValueError, match="align_dtype"):
        RowBank(128, "fp4", 0, "cpu", arg="align_dtype")
    with pytest.raises(ValueError, match=r"align_dtype.*64"):
        RowBank(96, "mx8", 0, "cpu", arg="align_dtype")
    with pytest.raises(ValueError, match=r"kv_dtype.*64"):
        RowBank(96, "mx8", 0, "cpu", arg="kv_dtype")
    RowBank(96, "bf16", 0, "cpu")                                        # bf16 rows have no such rule
    with pytest.raises(ValueError, match="kv_dtype"):
        RowBank(96, "fp8", 0, "cpu", arg="kv_dtype", held=False)         # the name is checked even for an empty bank
    assert RowBank(96, "mx8", 9, "cpu", held=False).data.shape == (0, 192)


def test_bytes_per_frame():
    f = RowBank.bytes_per_frame
    assert f(768) == f(768, "bf16") == 3072 and f(768, "mx8") == 1584
    assert ste.retrieval.kv_bytes_per_frame(768, "mx8") == ste.retrieval.align_bytes_per_frame(768, "mx8") == 1584
    with pytest.raises(ValueError, match="align_dtype"):
        ste.retrieval.align_bytes_per_frame(768, "fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        ste.retrieval.kv_bytes_per_frame(768, "fp8")


def test_the_stores_tensors_are_its_banks():
    model = types.SimpleNamespace(projection_dim=128, use_cross_modal=True, use_word_alignment=True)
    st = ste.AudioStateStore(model, "cpu", reserve_frames=6, kv_dtype="mx8", align_rows=True, align_dtype="mx8")
    for got, want in ((st.kv, st.kv_bank.data), (st.kv_scales, st.kv_bank.scales), (st.akv, st.align_bank.data),
                      (st.akv_scales, st.align_bank.scales)):
        assert got.shape[0] == 6 and got.data_ptr() == want.data_ptr()
    st._reserve(7)                                                       # the properties follow a growth
    assert st.kv.shape[0] == st.akv.shape[0] == 12 and st.kv.data_ptr() == st.kv_bank.data.data_ptr()
    st = ste.AudioStateStore(model, "cpu", reserve_frames=6, align_rows=True)
    assert st.kv.dtype == BF16 and st.kv_scales is None and st.akv.dtype == BF16 and st.akv_scales is None
    assert st.akv.data_ptr() == st.align_bank.data.data_ptr() != st.kv.data_ptr()
    st = ste.AudioStateStore(model, "cpu", reserve_frames=6, align_dtype="mx8")     # no align_rows: no such rows
    assert st.akv is None and st.akv_scales is None and st.kv.shape == (6, 256)
    plain = types.SimpleNamespace(projection_dim=128, use_cross_modal=False)
    st = ste.AudioStateStore(plain, "cpu", reserve_frames=6)
    assert st.kv.shape == (0, 256) and st.kv_scales is None and st.akv is None


def test_candidates_check():
    cand = torch.tensor([[0, 3, -1], [2, 2, 1]], dtype=I64)
    got, lo, hi = _candidates(cand, 2, 4, "k")
    assert got.dtype == I32 and got.is_contiguous() and torch.equal(got, cand.to(I32)) and (lo, hi) == (-1, 3)
    more = (cand.sum(dtype=I32), torch.tensor(9, dtype=I32))             # read in the same transfer
    assert _candidates(cand, 2, 4, "k", more=more)[1:] == (-1, 3, 7, 9)
    assert _candidates(got, 2, 4, "k")[0] is got                         # a checked list passes through as it is
    with pytest.raises(ValueError, match=r"\[3, k >= 1\]"):
        _candidates(cand, 3, 4, "k")                                     # the wrong number of rows
    with pytest.raises(ValueError, match=r"\[2, C >= 1\]"):
        _candidates(cand[:, :0], 2, 4, "C")                              # no column
    with pytest.raises(ValueError, match=r"\[2, C >= 1\]"):
        _candidates(cand.view(-1), 2, 4, "C")                            # not a matrix
    with pytest.raises(ValueError, match=r"lie in \[-1, 3\), got \[-1, 3\]"):
        _candidates(cand, 2, 3, "k")                                     # an id past the end
    with pytest.raises(ValueError, match=r"lie in \[-1, 4\), got \[-2, 3\]"):
        _candidates(cand - (cand < 0).long(), 2, 4, "k")                 # below -1


def _meta(*shape, dtype):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_xattn_seg_rejects_mismatched_rows_and_scales():
    R, G, Pq = 4, 2, 64
    q, out = _meta(3, Pq, dtype=torch.float32), _meta(R, Pq, dtype=torch.float32)
    idx = [_meta(R, dtype=I32), _meta(R, dtype=I32)]
    seg = [_meta(G, dtype=I64), _meta(G, dtype=I32), _meta(1, dtype=I32), _meta(1, dtype=I32), 8, out]
    bf, u8, sc = _meta(40, 2 * Pq, dtype=BF16), _meta(40, 2 * Pq, dtype=U8), _meta(40, 2 * Pq // 32, dtype=U8)
    kv = lambda t: [t[:, :Pq], t[:, Pq:]]                                 # noqa: E731
    with pytest.raises(AssertionError):                                  # bf16 rows with scales given
        ops.xattn_seg_fwd(q, *idx, *kv(bf), *seg, ks=sc[:, :2], vs=sc[:, 2:])
    with pytest.raises(AssertionError):                                  # uint8 rows without
        ops.xattn_seg_fwd(q, *idx, *kv(u8), *seg)
    with pytest.raises(AssertionError):                                  # one scale view only
        ops.xattn_seg_fwd(q, *idx, *kv(u8), *seg, ks=sc[:, :2])
    with pytest.raises(AssertionError):                                  # scales of another row stride
        ops.xattn_seg_fwd(q, *idx, *kv(u8), *seg, ks=sc[:, :2], vs=_meta(40, 2, dtype=U8))
    with pytest.raises(AssertionError):                                  # scales that are not bytes
        ops.xattn_seg_fwd(q, *idx, *kv(u8), *seg, ks=sc[:, :2].to(I32), vs=sc[:, 2:].to(I32))
    with pytest.raises(AssertionError):                                  # k and v of two dtypes
        ops.xattn_seg_fwd(q, *idx, bf[:, :Pq], u8[:, Pq:], *seg)


def test_align_matrix_seg_rejects_mismatched_rows_and_scales():
    R, G, L, Tmax, Pq = 2, 2, 3, 16, 64
    q = _meta(2 * L, Pq, dtype=BF16)
    head = [q, _meta(R, dtype=I32), _meta(R, dtype=I32)]
    tail = [_meta(G, dtype=I64), _meta(G, dtype=I32), L, Tmax, 4]
    out = dict(out=_meta(R * L, Pq, dtype=BF16))
    bf, u8, sc = _meta(40, 2 * Pq, dtype=BF16), _meta(40, 2 * Pq, dtype=U8), _meta(40, 2 * Pq // 32, dtype=U8)
    with pytest.raises(AssertionError):                                  # bf16 rows with scales given
        ops.align_matrix_seg_fwd(*head, bf, *tail, scales=sc, **out)
    with pytest.raises(AssertionError):                                  # uint8 rows without
        ops.align_matrix_seg_fwd(*head, u8, *tail, **out)
    with pytest.raises(AssertionError):                                  # a wrong scale width
        ops.align_matrix_seg_fwd(*head, u8, *tail, scales=_meta(40, 2 * Pq // 32 + 1, dtype=U8), **out)
    with pytest.raises(AssertionError):                                  # scales of fewer rows
        ops.align_matrix_seg_fwd(*head, u8, *tail, scales=sc[:39], **out)
    with pytest.raises(AssertionError):                                  # scales that are not bytes
        ops.align_matrix_seg_fwd(*head, u8, *tail, scales=sc.to(I32), **out)
