"""ste_resample on the GPU against the fp64 restatement of its definition (tests/kref_resample.py;
no bit-level reference exists for this step), and the routes that call it: the custom op,
to_model_batch, TrainStep and process_audio_array.

Parity bound, derived and not measured: an fp32 sum of K products in any order is within
gamma_K ~ K·2^-24 of the exact sum relative to Σ|h·x|; one more rounding each for the coefficient
(the table is rounded once to fp32), the product and the conversion gives
|y_gpu - y| <= (K + 3)·2^-24·Σ_m |h·x[m]| for every output."""
import numpy as np
import pytest
import torch

import kref_resample as kr

pytestmark = pytest.mark.gpu

# 48000, 44100, 24000, 8000: the decimation kernel (M = 3), the cached-table kernel, and the LDS-table
# kernel down and up; 32000: the decimation kernel's other instantiation (M = 2)
RATES = [48000, 44100, 24000, 8000, 32000]
EPS = 2.0 ** -24


def _ops():
    from speech_transcript_embeddings_amd import ops
    return ops


def _lengths(sr):
    """{the shortest clip that spills one output past the kernel's tile, 100, 1}."""
    M, L = kr.plan(sr)[:2]
    T = _ops().resample_tile(sr)
    assert T > 0 and T % L == 0
    n = T * M // L + 1              # 48 k: 3·T + 1
    assert kr.n_out(n, M, L) > T >= kr.n_out(n - 1, M, L)
    assert n <= 0.3 * sr
    return [n, 100, 1]


_CASES = {}


def _case(sr):
    """Clips, their NaN-padded batch and the fp64 reference, computed once per rate and shared."""
    if sr not in _CASES:
        rng = np.random.default_rng(sr)
        lens = _lengths(sr)
        clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
        ld = max(lens) + 37         # a row stride larger than the longest clip
        wav = np.full((len(lens), ld), np.nan, np.float32)
        for b, c in enumerate(clips):
            wav[b, : len(c)] = c
        ref = [kr.resample(c, sr) for c in clips]
        _CASES[sr] = dict(lens=lens, clips=clips, wav=wav, ref=ref)
    return _CASES[sr]


def _check_row(sr, got_row, n_valid, y, bound, tag):
    K = kr.plan(sr)[2]
    got = got_row.astype(np.float64)
    assert np.isfinite(got).all(), tag
    assert len(y) == n_valid
    err = np.abs(got[:n_valid] - y)
    lim = (K + 3) * EPS * bound
    worst = float(np.max(err / np.maximum(lim, 1e-300))) if n_valid else 0.0
    print(f"{tag}: worst error / bound = {worst:.3f}")
    assert (err <= lim).all(), tag
    assert (got_row[n_valid:] == 0.0).all(), tag          # exactly zero past the clip


@pytest.mark.parametrize("sr", RATES)
def test_parity_with_restatement(sr):
    ops = _ops()
    c = _case(sr)
    M, L = kr.plan(sr)[:2]
    wav = torch.from_numpy(c["wav"]).cuda()
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    out, out_lens = ops.resample(wav, lens, sr)
    assert out.shape == (3, kr.n_out(wav.shape[1], M, L)) and out.dtype == torch.float32
    expect = [kr.n_out(n, M, L) for n in c["lens"]]
    assert out_lens.dtype == torch.int32 and out_lens.tolist() == expect
    assert max(expect) > ops.resample_tile(sr)            # more than one workgroup per clip
    got = out.cpu().numpy()
    for b, (y, bound) in enumerate(c["ref"]):
        _check_row(sr, got[b], expect[b], y, bound, f"{sr} row {b}")


@pytest.mark.parametrize("sr", RATES)
def test_rows_do_not_depend_on_the_batch(sr):
    ops = _ops()
    c = _case(sr)
    wav = torch.from_numpy(c["wav"]).cuda()
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    out, _ = ops.resample(wav, lens, sr)
    again, _ = ops.resample(wav, lens, sr)
    assert torch.equal(out, again)                        # run to run
    for b, clip in enumerate(c["clips"]):
        one = torch.from_numpy(clip).cuda().reshape(1, -1)   # alone, tight stride
        y, n = ops.resample(one, torch.tensor([len(clip)], dtype=torch.int32, device="cuda"), sr)
        assert y.shape[1] == int(n.item())
        assert torch.equal(y[0], out[b, : y.shape[1]]), (sr, b)


@pytest.mark.parametrize("sr", [48000, 44100, 8000])
def test_degenerate_lengths_and_guards(sr):
    ops = _ops()
    M, L, K, hw, _ = kr.plan(sr)
    rng = np.random.default_rng(7)
    lens = [0, 1, hw - 1]
    N = hw + 10
    wav = np.full((3, N), np.nan, np.float32)
    clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
    for b, cl in enumerate(clips):
        wav[b, : len(cl)] = cl
    n_max = kr.n_out(N, M, L)
    expect = [kr.n_out(n, M, L) for n in lens]
    assert n_max > max(expect)
    G, ld, SENT = 64, n_max + 5, 12345.0
    buf = torch.full((2 * G + 3 * ld,), SENT, device="cuda")
    out = buf[G: G + 3 * ld].view(3, ld)[:, :n_max]
    got, out_lens = ops.resample(torch.from_numpy(wav).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"), sr,
                                 out=out)
    assert got.data_ptr() == out.data_ptr() and out_lens.tolist() == expect
    flat = buf.cpu().numpy()
    assert (flat[:G] == SENT).all() and (flat[G + 3 * ld:] == SENT).all()
    rows = flat[G: G + 3 * ld].reshape(3, ld)
    assert (rows[:, n_max:] == SENT).all()                # the gap between rows is never written
    for b, cl in enumerate(clips):
        y, bound = kr.resample(cl, sr)
        _check_row(sr, rows[b, :n_max], expect[b], y, bound, f"{sr} length {lens[b]}")


def test_identity_returns_the_inputs():
    ops = _ops()
    wav = torch.randn(2, 50, device="cuda")
    lens = torch.tensor([50, 20], dtype=torch.int32, device="cuda")
    y, n = ops.resample(wav, lens, 16000, 16000)
    assert y is wav and n is lens
    y, n = ops.resample(wav, lens, 16000)
    assert y is wav and n is lens


def test_alias_rejection_on_the_device():
    """A 10 kHz tone at 48 kHz lies above the 8 kHz Nyquist of the output: what is left is fp32
    rounding, <= (K + 3)·2^-24·Σ|h| = -81.9 dB for K = 406, Σ|h| = 2.34 in the worst case."""
    ops = _ops()
    sr, f = 48000, 10000
    x = np.sin(2 * np.pi * f * np.arange(sr // 4) / sr).astype(np.float32)
    y, n = ops.resample(torch.from_numpy(x).cuda().reshape(1, -1), torch.tensor([len(x)], dtype=torch.int32,
                                                                               device="cuda"), sr)
    y = y[0].cpu().numpy().astype(np.float64)
    assert int(n.item()) == len(y) == 4000
    mid = y[len(y) // 4: len(y) - len(y) // 4]
    db = 20 * np.log10(max(np.sqrt(np.mean(mid ** 2)), 1e-300) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print(f"10 kHz tone, 48 k -> 16 k: output rms {db:.1f} dB relative to the input")
    assert db <= -80.0


# ------------------------------------------------------------------------------------ routes
def test_custom_op_equals_ops():
    import speech_transcript_embeddings_amd  # noqa: F401  (registers torch.ops.ste.*)
    ops = _ops()
    c = _case(44100)
    wav = torch.from_numpy(np.nan_to_num(c["wav"])).cuda()
    lens = torch.tensor(c["lens"], dtype=torch.int32, device="cuda")
    a, an = ops.resample(wav, lens, 44100)
    b, bn = torch.ops.ste.resample(wav, lens, 44100)
    assert torch.equal(a, b) and torch.equal(an, bn)
    b, bn = torch.ops.ste.resample(wav, lens.long(), 44100, 16000)
    assert torch.equal(a, b) and torch.equal(an, bn)
    same, sn = torch.ops.ste.resample(wav, lens, 16000)
    assert torch.equal(same, wav) and torch.equal(sn, lens)


class _Tok:
    def __call__(self, text, max_length, padding, truncation, return_tensors):
        ids = ([0] + [5 + len(w) for w in text.split()] + [2])[:max_length]
        mask = [1] * len(ids) + [0] * (max_length - len(ids))
        return {"input_ids": torch.tensor([ids + [1] * (max_length - len(ids))]), "attention_mask": torch.tensor([mask])}


def _collated(lens, rates):
    from speech_transcript_embeddings_amd.data import CommonVoiceDataset, waveform_collate_fn
    rng = np.random.default_rng(11)
    items = []
    for n, r in zip(lens, rates):
        audio = {"array": (0.1 * rng.standard_normal(n)).astype(np.float32)}
        if r is not None:
            audio["sampling_rate"] = r
        items.append({"audio": audio, "sentence": "o gato subiu no telhado"})
    ds = CommonVoiceDataset(items, _Tok(), None, max_text_length=8, raw_audio=True)
    return waveform_collate_fn([ds[i] for i in range(len(items))])


def test_to_model_batch_resamples_first():
    from speech_transcript_embeddings_amd.data import to_model_batch
    from speech_transcript_embeddings_amd.features import num_frames
    ops = _ops()
    lens48 = [14400, 9000, 12345]                         # 0.3 s, 0.19 s, 0.26 s at 48 kHz
    batch = _collated(lens48, [48000] * 3)
    assert batch["sampling_rates"] == [48000] * 3
    got = to_model_batch(batch)
    wav16, len16 = ops.resample(batch["waveform"].cuda(), batch["lengths"].cuda(), 48000)
    host16 = [-(-n // 3) for n in lens48]
    assert len16.tolist() == host16
    T = max(num_frames(n) for n in host16)
    feats, mask = ops.fbank(wav16, len16, T, pad_value=1.0, mask_mode=0)
    assert torch.equal(got["input_values"], feats) and torch.equal(got["attention_mask_audio"], mask)
    assert got["audio_lengths"] == mask.sum(1).tolist() == [num_frames(n) for n in host16]
    assert "sampling_rates" not in got and "waveform" not in got
    assert torch.isfinite(feats).all() and T == 14


def test_mixed_rates_keep_the_row_order():
    from speech_transcript_embeddings_amd.data import resample_batch, to_model_batch
    from speech_transcript_embeddings_amd.features import num_frames
    ops = _ops()
    lens, rates = [14400, 13000, 9000, 4000, 12001], [48000, 44100, 48000, None, 44100]
    batch = _collated(lens, rates)
    assert batch["sampling_rates"] == [48000, 44100, 48000, 16000, 44100]
    wav, dl = batch["waveform"].cuda(), batch["lengths"].cuda()
    w16, l16, host = resample_batch(wav, dl, lens, batch["sampling_rates"])
    assert l16.tolist() == host == [ops.resampled_length(n, r) for n, r in zip(lens, batch["sampling_rates"])]
    for i, (n, r) in enumerate(zip(lens, batch["sampling_rates"])):
        one, _ = ops.resample(wav[i: i + 1, :n].contiguous(), dl[i: i + 1].contiguous(), r)
        assert torch.equal(w16[i, : host[i]], one[0, : host[i]]), i
        assert (w16[i, host[i]:] == 0).all(), i
    got = to_model_batch(batch)
    T = max(num_frames(n) for n in host)
    feats, mask = ops.fbank(w16, l16, T, pad_value=1.0, mask_mode=0)
    assert torch.equal(got["input_values"], feats) and torch.equal(got["attention_mask_audio"], mask)
    assert got["audio_lengths"] == mask.sum(1).tolist()


def test_train_step_with_a_native_rate():
    from test_model_gpu import load, mini_model

    from speech_transcript_embeddings_amd.train import TrainStep, synthetic_batch
    ops = _ops()
    meta, _ = load("noalign")

    def build():
        m = mini_model(meta, spec_augment=False)
        m.dropout = 0.0
        m.audio_cfg.conformer_conv_dropout = 0.0
        m.audio_cfg.layerdrop = 0.0
        m.text_cfg.hidden_dropout_prob = 0.0
        m.text_cfg.attention_probs_dropout_prob = 0.0
        return m

    wav, lengths, *text = synthetic_batch(2, 14400, 12, vocab=meta["mini"]["text"]["vocab_size"], seed=3)
    lengths = torch.tensor([14400, 10001], dtype=torch.int32)            # on the host, as a DataLoader gives them
    a = TrainStep(build(), lr=1e-3, warmup=1, total_steps=10)
    loss_a = a(wav, lengths, *text, sampling_rate=48000)
    b = TrainStep(build(), lr=1e-3, warmup=1, total_steps=10)
    w16, l16 = ops.resample(wav, lengths.cuda(), 48000)
    assert w16.shape[1] == 4800 and l16.tolist() == [4800, 3334]
    feats, amask = b.features(w16, l16)
    loss_b = b.step_batch({"input_ids_pos": text[0], "attention_mask_pos": text[1], "input_ids_neg": text[2],
                           "attention_mask_neg": text[3], "input_values": feats, "attention_mask_audio": amask,
                           "audio_lengths": amask.sum(1).tolist()})
    assert torch.isfinite(loss_a).all()
    assert torch.equal(loss_a, loss_b)
    c = TrainStep(build(), lr=1e-3, warmup=1, total_steps=10)             # 16000 and None leave the clips alone
    d = TrainStep(build(), lr=1e-3, warmup=1, total_steps=10)
    l16h = torch.tensor([4800, 3334], dtype=torch.int32)
    assert torch.equal(c(w16, l16h, *text, sampling_rate=16000), d(w16, l16h, *text))


def test_process_audio_array():
    from speech_transcript_embeddings_amd.features import SeamlessM4TFeatureExtractor, process_audio_array
    ops = _ops()
    rng = np.random.default_rng(2)
    n = 12000                                                             # 0.25 s at 48 kHz -> 4000 samples
    x = (2.0 * np.sin(2 * np.pi * 1000 * np.arange(n) / 48000) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    x *= 2.0 / np.abs(x).max()                                            # peak 2.0
    fe = SeamlessM4TFeatureExtractor()
    got = process_audio_array(x, 48000, extractor=fe, max_audio_length=3000)
    y, _ = ops.resample(torch.from_numpy(x).cuda().reshape(1, -1), torch.tensor([n], dtype=torch.int32, device="cuda"),
                        48000)
    assert y.shape[1] == 4000
    peak = y.abs().max()
    assert peak.item() > 1.5
    y = (y / peak)[0, :3000]
    want = fe(y.cpu().numpy(), sampling_rate=16000, return_tensors="pt")
    assert torch.equal(got["input_features"], want["input_features"])
    assert torch.equal(got["attention_mask_audio"], want["attention_mask"])
    assert got["input_features"].shape[0] == 1 and got["input_features"].shape[2] == 160
    longer = process_audio_array(x, 48000, extractor=fe)                  # untrimmed: more frames
    assert longer["input_features"].shape[1] > got["input_features"].shape[1]
    quiet = process_audio_array(0.25 * x, 48000, extractor=fe)             # peak 0.5: no scaling, no trim
    y2, _ = ops.resample(torch.from_numpy(0.25 * x).cuda().reshape(1, -1),
                         torch.tensor([n], dtype=torch.int32, device="cuda"), 48000)
    want2 = fe(y2[0].cpu().numpy(), sampling_rate=16000, return_tensors="pt")
    assert torch.equal(quiet["input_features"], want2["input_features"])
    same = process_audio_array(y2[0].cpu().numpy(), 16000, extractor=fe)   # already at 16 kHz: no resampling
    assert torch.equal(same["input_features"], want2["input_features"])
    with pytest.raises(ValueError):
        fe(x, sampling_rate=48000)                                         # the extractor itself still refuses
