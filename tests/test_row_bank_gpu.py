"""retrieval.RowBank holding MX-fp8 rows on the GPU, alone and as both banks of an AudioStateStore, at the
shapes of the locate fixtures (P = 128, 2 clips of T = 49 frames, 49 and 39 of them valid).  Exact: the stored
bytes and scales of a clip are ops.mx8_quant of that clip's bf16 rows, and what rows() reads back is
ops.mx8_dequant of them (quantisation is per row, so neither depends on where or with what a clip was written)."""
import pytest
import torch

from test_locate_mx8_gpu import _fx

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, B, T, FRAMES = 128, 2, 49, [49, 39]


def _is_quantised(ops, bank, a, rows_bf16):
    """Rows a .. of bank hold mx8_quant(rows_bf16), and bank.rows reads back their dequantisation."""
    n = rows_bf16.shape[0]
    q, s = ops.mx8_quant(rows_bf16.contiguous())
    assert torch.equal(bank.data[a:a + n], q) and torch.equal(bank.scales[a:a + n], s)
    got = bank.rows(a, a + n)
    assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), ops.mx8_dequant(q, s).view(torch.int16))


def test_mx8_bank_write_and_rows():
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.retrieval import RowBank
    gen = torch.Generator(device=DEV).manual_seed(5)
    src = (torch.randn(B * T, 2 * P, device=DEV, generator=gen) * 3).to(torch.bfloat16)
    bank = RowBank(P, "mx8", 0, DEV)
    bank.reserve(sum(FRAMES) + 4, 0)
    bank.data.fill_(0xAB)
    bank.scales.fill_(0xCD)
    bank.write(2, src, FRAMES, T)                                        # ragged: a copy per clip
    assert bank.data.dtype == torch.uint8 and bank.scales.shape == (bank.data.shape[0], 2 * P // 32)
    at = 2
    for b, n in enumerate(FRAMES):
        _is_quantised(ops, bank, at, src[b * T:b * T + n])
        at += n
    assert (bank.data[:2] == 0xAB).all() and (bank.data[at:] == 0xAB).all() and (bank.scales[at:] == 0xCD).all()
    full = RowBank(P, "mx8", B * T, DEV)
    full.write(0, src, [T] * B, T)                                       # full length: one copy
    _is_quantised(ops, full, 0, src)


def test_both_banks_of_a_store():
    from speech_transcript_embeddings_amd import AudioStateStore, ops
    fx = _fx()
    model, wave, amask, bf = fx["model"], fx["wave"], fx["amask"], fx["bf"]
    st = AudioStateStore(model, DEV, kv_dtype="mx8", align_rows=True, align_dtype="mx8")
    with torch.no_grad():
        enc = model.encode_audio(wave, amask)                            # the model is in eval mode
    st.add(wave, amask, audio_encoded=enc)
    assert st.frames.tolist() == FRAMES and st.rows == sum(FRAMES) and st.seg_row.tolist() == [0, FRAMES[0]]
    assert st.kv.data_ptr() == st.kv_bank.data.data_ptr() and st.akv_scales.data_ptr() == st.align_bank.scales.data_ptr()
    for n in range(B):
        _is_quantised(ops, st.kv_bank, st._seg_row[n], bf.kv_rows(n))
        _is_quantised(ops, st.align_bank, st._seg_row[n], bf.align_kv_rows(n))
        assert torch.equal(st.kv_rows(n), st.kv_bank.rows(st._seg_row[n], st._seg_row[n] + FRAMES[n]))
        assert torch.equal(st.align_kv_rows(n), st.align_bank.rows(st._seg_row[n], st._seg_row[n] + FRAMES[n]))
