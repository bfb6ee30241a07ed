"""The resampler without a GPU: the host-only plan and coefficient table of libste.so against the
fp64 restatement (tests/kref_resample.py), argument validation before any launch, the fake op,
the host length helper, the signal properties the filter definition itself must have (checked on
the restatement in fp64: no bit-level reference exists for this step), and the data path's
behaviour with and without rate information."""
import ctypes as C

import numpy as np
import pytest
import torch

import kref_resample as kr

ERR_ARG, ERR_SHAPE = 1001, 1002   # include/ste.h STE_ERR_ARG / STE_ERR_SHAPE
PLANS = {48000: (3, 1, 406), 44100: (441, 160, 374), 32000: (2, 1, 272), 24000: (3, 2, 204),
         22050: (441, 320, 188), 11025: (441, 640, 136), 8000: (1, 2, 136)}


@pytest.fixture(scope="module")
def lib():
    from speech_transcript_embeddings_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.fail("libste.so not built — run __graft_entry__.build()")
    return _lib


@pytest.mark.parametrize("sr", sorted(PLANS))
def test_plan_table(lib, sr):
    M, L, K = C.c_int(), C.c_int(), C.c_int()
    assert lib.fn("ste_resample_plan")(sr, 16000, C.byref(M), C.byref(L), C.byref(K)) == 0
    assert (M.value, L.value, K.value) == PLANS[sr] == kr.plan(sr)[:3]
    assert L.value * K.value == {48000: 406, 44100: 59840, 32000: 272, 24000: 408, 22050: 60160, 11025: 87040,
                                 8000: 272}[sr]
    assert lib.fn("ste_resample_tile")(M.value, L.value, K.value) % L.value == 0


def test_plan_errors(lib):
    f = lib.fn("ste_resample_plan")
    M, L, K = C.c_int(), C.c_int(), C.c_int()
    for a, b in ((0, 16000), (-48000, 16000), (48000, 0), (48000, -1)):
        assert f(a, b, C.byref(M), C.byref(L), C.byref(K)) == ERR_ARG
    assert f(16001, 16000, C.byref(M), C.byref(L), C.byref(K)) == ERR_SHAPE       # L = 16000 phases
    assert f(16000 * 17, 16000, C.byref(M), C.byref(L), C.byref(K)) == ERR_SHAPE  # L = 1, K = 2298 taps
    assert f(48000, 16000, None, None, None) == 0
    buf = np.empty(8, np.float32)
    assert lib.fn("ste_resample_table")(16001, 16000, buf.ctypes.data, 8) == ERR_SHAPE
    assert lib.fn("ste_resample_table")(48000, 16000, buf.ctypes.data, 8) == ERR_ARG   # buffer too small
    assert lib.fn("ste_resample_table")(48000, 16000, None, 406) == ERR_ARG


@pytest.mark.parametrize("sr", [48000, 44100, 24000, 8000])
def test_table_within_one_ulp_of_restatement(lib, sr):
    M, L, K = PLANS[sr]
    got = np.full(L * K + 2, np.float32(777.0))
    assert lib.fn("ste_resample_table")(sr, 16000, got.ctypes.data, L * K) == 0
    assert (got[L * K:] == 777.0).all()                       # nothing written past L·K
    ref = kr.table(sr).astype(np.float32).reshape(-1)         # [K, L] row-major = tap-major t·L + i
    err = np.abs(got[: L * K].astype(np.float64) - ref.astype(np.float64))
    ulp = np.spacing(np.abs(ref)).astype(np.float64)
    print(f"{sr}: worst error {np.max(err / ulp):.2f} ulp")
    assert (err <= ulp).all()
    assert np.abs(ref).max() > 0.1                            # a real filter, not zeros


def test_launch_arguments_rejected_before_any_launch(lib):
    f = lib.fn("ste_resample")
    p = 4096   # non-NULL placeholders: validation returns before anything is dereferenced or launched
    ok = dict(wav=p, ld_wav=100, lengths=p, B=2, M=3, L=1, K=406, table=p, out=p, ld_out=40, n=34, ol=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["wav"], a["ld_wav"], a["lengths"], a["B"], a["M"], a["L"], a["K"], a["table"], a["out"],
                 a["ld_out"], a["n"], a["ol"], None)
    assert call(B=-1) == ERR_ARG
    assert call(ld_wav=-1) == ERR_ARG
    assert call(table=None) == ERR_ARG
    assert call(wav=None) == ERR_ARG and call(lengths=None) == ERR_ARG and call(out=None) == ERR_ARG
    assert call(K=405) == ERR_ARG and call(M=0) == ERR_ARG
    assert call(L=1025) == ERR_SHAPE and call(K=2050) == ERR_SHAPE
    assert call(ld_out=33) == ERR_SHAPE        # a row shorter than n_out_max
    assert call(B=0) == 0 and call(n=0) == 0   # nothing to do: no launch either


def test_host_tensors_are_refused(lib):
    """ops.resample hands raw pointers to the kernel: tensors that are not on the GPU never reach it."""
    from speech_transcript_embeddings_amd import ops
    wav, lens = torch.zeros(2, 10), torch.tensor([10, 10], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.resample(wav, lens, 48000)
    y, n = ops.resample(wav, lens, 16000)          # same rate: returned as they are, no launch
    assert y is wav and n is lens


def test_fake_op_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import speech_transcript_embeddings_amd  # noqa: F401  (registers torch.ops.ste.*)
    from speech_transcript_embeddings_amd import torch_ops
    assert "resample" in torch_ops.OPS
    assert torch.ops.ste.resample.default._schema.name == "ste::resample"
    with FakeTensorMode():
        for sr, N in ((48000, 3073), (44100, 3071), (8000, 100), (16000, 77)):
            M, L, _ = kr.plan(sr)[:3]
            y, n = torch.ops.ste.resample(torch.empty(3, N), torch.empty(3, dtype=torch.int32), sr)
            assert y.shape == (3, -(-N * L // M)) and y.dtype == torch.float32
            assert n.shape == (3,) and n.dtype == torch.int32


@pytest.mark.parametrize("sr,expected", [(48000, [0, 1, 1, 1, 34, 1024, 1024, 1025]),
                                         (44100, [0, 1, 1, 2, 37, 1115, 1115, 1115]),
                                         (8000, [0, 2, 4, 6, 200, 6142, 6144, 6146])])
def test_resampled_length(lib, sr, expected):
    from speech_transcript_embeddings_amd import ops
    ns = [0, 1, 2, 3, 100, 3071, 3072, 3073]
    assert [ops.resampled_length(n, sr, 16000) for n in ns] == expected
    assert [ops.resampled_length(n, sr) for n in ns] == expected
    M, L = kr.plan(sr)[:2]
    assert [kr.n_out(n, M, L) for n in ns] == expected
    assert [ops.resampled_length(n, 16000, 16000) for n in ns] == ns


# ----------------------------------------------------------- properties of the definition (fp64)
def _tone(sr, f, seconds=0.25):
    return np.sin(2 * np.pi * f * np.arange(int(sr * seconds)) / sr)


def _mid(y):
    n = len(y)
    return y[n // 4: n - n // 4]


def _db(x):
    return 20 * np.log10(max(x, 1e-300))


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def _tone_gain_db(y, f, sr_out=16000):
    """Least-squares amplitude of a unit-amplitude tone at f in y, in dB."""
    t = np.arange(len(y)) / sr_out
    A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    a, b = np.linalg.lstsq(A, y, rcond=None)[0]
    return _db(float(np.hypot(a, b)))


@pytest.fixture(scope="module")
def tones():
    """(sr_in, f) -> middle half of the fp64 restatement's output for a 0.25 s unit tone."""
    out = {}
    for sr, fs in ((48000, (1000, 7000, 8500, 10000, 15000, 20000)), (44100, (1000, 7000, 8500, 10000, 15000, 20000)),
                   (8000, (1000, 3000, 3400))):
        for f in fs:
            out[sr, f] = _mid(kr.resample(_tone(sr, f), sr)[0])
    return out


@pytest.mark.parametrize("sr", [48000, 44100])
def test_passband_and_stopband_of_the_definition(tones, sr):
    for f in (1000, 7000):
        y = tones[sr, f]
        g = _tone_gain_db(y, f)
        print(f"{sr} Hz in, {f} Hz tone: gain {g:.2e} dB")
        assert abs(g) <= 1e-3
    for f in (8500, 10000, 15000, 20000):
        y = tones[sr, f]
        r = _db(_rms(y))
        print(f"{sr} Hz in, {f} Hz tone: output rms {r:.1f} dB")
        assert r <= -120.0


def test_upsampling_images_of_the_definition(tones):
    for f in (1000, 3000, 3400):
        y = tones[8000, f]
        g = _tone_gain_db(y, f)
        assert abs(g) <= 1e-3, (f, g)
        spec = np.abs(np.fft.rfft(y * np.blackman(len(y))))
        freqs = np.fft.rfftfreq(len(y), 1 / 16000)
        line = spec[np.argmin(np.abs(freqs - f)) - 2: np.argmin(np.abs(freqs - f)) + 3].max()
        image = spec[freqs > 4300].max()
        print(f"8000 Hz in, {f} Hz tone: gain {g:.2e} dB, largest line above 4.3 kHz {_db(image / line):.1f} dB")
        assert _db(image / line) <= -120.0


@pytest.mark.parametrize("sr", sorted(PLANS))
def test_dc_gain_of_every_phase(sr):
    dc = kr.table(sr).sum(0)
    assert dc.shape == (PLANS[sr][1],)
    assert np.abs(dc - 1.0).max() <= 1e-7


# ---------------------------------------------------------------------------------- data path
class _Tok:
    def __call__(self, text, max_length, padding, truncation, return_tensors):
        ids = ([0] + [5 + len(w) for w in text.split()] + [2])[:max_length]
        mask = [1] * len(ids) + [0] * (max_length - len(ids))
        return {"input_ids": torch.tensor([ids + [1] * (max_length - len(ids))]), "attention_mask": torch.tensor([mask])}


def _dataset(rates):
    from speech_transcript_embeddings_amd.data import CommonVoiceDataset
    rng = np.random.default_rng(3)
    items = []
    for k, r in enumerate(rates):
        audio = {"array": rng.standard_normal(500 + 100 * k).astype(np.float32)}
        if r is not None:
            audio["sampling_rate"] = r
        items.append({"audio": audio, "sentence": "duas palavras"})
    return CommonVoiceDataset(items, _Tok(), None, max_text_length=8, raw_audio=True)


def test_collate_unchanged_without_rate_information():
    from speech_transcript_embeddings_amd.data import waveform_collate_fn
    expect = {"input_ids_pos", "attention_mask_pos", "input_ids_neg", "attention_mask_neg", "waveform", "lengths",
              "is_corrupted"}
    for rates in ([None, None, None], [16000, 16000, 16000], [None, 16000, None]):
        ds = _dataset(rates)
        items = [ds[i] for i in range(3)]
        assert all("sampling_rate" not in it for it in items)
        assert all(set(it) == {"input_ids_pos", "attention_mask_pos", "input_ids_neg", "attention_mask_neg",
                               "waveform"} for it in items)
        out = waveform_collate_fn(items)
        assert set(out) == expect
        assert out["lengths"].tolist() == [500, 600, 700] and out["waveform"].shape == (3, 700)


def test_collate_carries_rates():
    from speech_transcript_embeddings_amd.data import waveform_collate_fn
    ds = _dataset([48000, None, 44100])
    items = [ds[i] for i in range(3)]
    assert [it.get("sampling_rate") for it in items] == [48000, None, 44100]
    out = waveform_collate_fn(items)
    assert out["sampling_rates"] == [48000, 16000, 44100]
    assert out["lengths"].tolist() == [500, 600, 700]
    plain = waveform_collate_fn([{k: v for k, v in it.items() if k != "sampling_rate"} for it in items])
    for k, v in plain.items():
        assert torch.equal(v, out[k]), k
