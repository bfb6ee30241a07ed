"""Data path: transcript corruption, the dataset wrapper, a raw-waveform
collate for the on-GPU fbank, and length-bucketed batching.

Reference behaviour mirrored (training/trainer_unfreeze.py):
  * create_corrupted_transcript (:784-829): one of replace / shuffle / drop / add / partial,
    drawn from Python's `random` with the same sequence of calls, so a seeded run produces
    the reference's exact corrupted transcripts (tests/golden/corruption_golden.json, made
    by the reference itself);
  * CommonVoiceDataset (:745-875): same constructor, same item dict (clean and corrupted
    transcripts tokenised to max_length with padding="max_length", audio features +
    attention mask).  Like the reference, the negative transcript is always corrupted
    (corruption_probability is recorded but not applied);
  * custom_collate_fn (:880-921) is features.custom_collate_fn.

MI355X additions, not in the reference:
  * `raw_audio=True` makes the dataset return the waveform instead of CPU features, and
    `waveform_collate_fn` pads a batch of waveforms into one [B, Nmax] float32 tensor +
    lengths.  `to_model_batch` then runs the batched fbank kernel on the GPU and returns the
    reference's batch schema (input_values / attention_mask_audio exactly as
    custom_collate_fn over per-clip features).  This removes the reference's 12 CPU
    feature-extraction workers (20.5 ms per 10 s clip per core).
  * `LengthBucketBatchSampler` groups clips of similar length.  The encoders run on the
    padded T of each batch, so with real Common Voice lengths bucketing removes most
    padding work.  The reference's `--bucket` flag (:1898) is accepted but unused.
"""
from __future__ import annotations

import math
import random

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from .features import custom_collate_fn, num_frames  # noqa: F401  (re-exported: the reference's collate)

# word lists of the "replace" and "add" strategies (ref:797, :815)
REPLACE_WORDS = ("sim", "não", "e", "o", "de", "um", "uma", "tua", "qualquer", "coisa", "deveria", "gostaria",
                 "imaginemos")
INSERT_WORDS = ("sim", "não", "e", "o", "de", "um", "uma")
STRATEGIES = ("replace", "shuffle", "drop", "add", "partial")
TARGET_RATE = 16000   # what every audio entry point expects; other rates are resampled on the GPU


def create_corrupted_transcript(text: str, rng=random) -> str:
    """ref:784-829.  Texts of <= 1 word come back unchanged (no random draw)."""
    words = text.split()
    n = len(words)
    if n <= 1:
        return text
    kind = rng.choice(STRATEGIES)
    if kind == "replace":
        at = rng.randint(0, n - 1)
        words[at] = rng.choice(REPLACE_WORDS)
    elif kind == "shuffle":
        if n > 2:
            lo = rng.randint(0, n - 2)
            hi = rng.randint(lo + 1, n - 1)
            seg = words[lo:hi + 1]
            rng.shuffle(seg)
            words[lo:hi + 1] = seg
    elif kind == "drop":
        del words[rng.randint(0, n - 1)]
    elif kind == "add":
        at = rng.randint(0, n)
        words.insert(at, rng.choice(INSERT_WORDS))
    else:  # partial: first or second half
        half = n // 2
        words = words[:half] if rng.random() < 0.5 else words[half:]
    return " ".join(words)


class CommonVoiceDataset(torch.utils.data.Dataset):
    """ref:745-875.  `dataset[i]` must provide {"audio": {"array": 1-D float}, "sentence": str}
    (a Hugging Face Common Voice split).  With raw_audio=True the item carries "waveform"
    (float32 [n]) instead of "input_values" / "attention_mask_audio" and feature_extractor
    may be None."""

    def __init__(self, dataset, tokenizer, feature_extractor=None, max_text_length=128, sampling_rate=16000,
                 max_audio_length=160000, add_corrupted_examples=True, corruption_probability=0.2,
                 raw_audio=False):
        if feature_extractor is None and not raw_audio:
            raise ValueError("feature_extractor is required unless raw_audio=True")
        self.dataset = dataset
        self.tokenizer = tokenizer
        self.feature_extractor = feature_extractor
        self.max_text_length = max_text_length
        self.sampling_rate = sampling_rate
        self.max_audio_length = max_audio_length
        self.add_corrupted_examples = add_corrupted_examples
        self.corruption_probability = corruption_probability
        self.raw_audio = raw_audio

    def __len__(self):
        return len(self.dataset)

    def create_corrupted_transcript(self, text):
        return create_corrupted_transcript(text)

    def _tok(self, text):
        enc = self.tokenizer(text, max_length=self.max_text_length, padding="max_length", truncation=True,
                             return_tensors="pt")
        return enc["input_ids"].squeeze(0), enc["attention_mask"].squeeze(0)

    def __getitem__(self, idx):
        item = self.dataset[idx]
        speech = item["audio"]["array"]
        clean = item["sentence"]
        corrupt = self.create_corrupted_transcript(clean)
        ids_p, m_p = self._tok(clean)
        ids_n, m_n = self._tok(corrupt)
        out = {"input_ids_pos": ids_p, "attention_mask_pos": m_p, "input_ids_neg": ids_n, "attention_mask_neg": m_n}
        if self.raw_audio:
            out["waveform"] = torch.as_tensor(np.asarray(speech, dtype=np.float32)).reshape(-1)
            # a clip at its native rate (Common Voice: 48 kHz) is resampled on the GPU by to_model_batch
            sr = item["audio"].get("sampling_rate") if hasattr(item["audio"], "get") else None
            if sr is not None and int(sr) != self.sampling_rate:
                out["sampling_rate"] = int(sr)
            return out
        feats = self.feature_extractor(speech, sampling_rate=self.sampling_rate, return_tensors="pt")
        x = feats["input_features"] if "input_features" in feats else feats["input_values"]
        mask = feats.get("attention_mask", None)
        out["input_values"] = x.squeeze(0)
        out["attention_mask_audio"] = mask.squeeze(0) if mask is not None else None
        return out


def waveform_collate_fn(batch):
    """Raw-audio items -> {text tensors padded as custom_collate_fn does, "waveform" [B, Nmax]
    float32 (zeros past each clip), "lengths" [B] int32, "is_corrupted" zeros}; None if the
    batch is empty after dropping None items."""
    batch = [b for b in batch if b is not None]
    if not batch:
        return None
    out = {}
    for key in ("input_ids_pos", "attention_mask_pos", "input_ids_neg", "attention_mask_neg"):
        out[key] = pad_sequence([b[key] for b in batch], batch_first=True, padding_value=0)
    waves = [b["waveform"] for b in batch]
    lens = torch.tensor([w.numel() for w in waves], dtype=torch.int32)
    wav = torch.zeros(len(waves), int(lens.max()), dtype=torch.float32)
    for i, w in enumerate(waves):
        wav[i, : w.numel()] = w
    out["waveform"] = wav
    out["lengths"] = lens
    out["is_corrupted"] = torch.zeros(len(waves), dtype=torch.long)
    # host list of the clips' native rates, only when some item carries one (the dataset adds
    # "sampling_rate" to items that differ from its target rate)
    if any("sampling_rate" in b for b in batch):
        out["sampling_rates"] = [int(b.get("sampling_rate", TARGET_RATE)) for b in batch]
    return out


def resample_batch(wav, lens, host_lens, rates, sr_out=TARGET_RATE):
    """wav [B, N] / lens int32 [B] on the GPU with per-clip native rates (host list) -> (wav at
    sr_out [B, N'], lens [B], host lengths): one ops.resample launch per distinct rate over the
    rows of that rate, written back to their rows of one zero-padded batch.  The row selections
    are built from host lists, so nothing is read back from the device."""
    from . import ops
    new_host = [ops.resampled_length(n, r, sr_out) for n, r in zip(host_lens, rates)]
    distinct = sorted(set(rates))
    if distinct == [sr_out]:
        return wav, lens, new_host
    if len(distinct) == 1:
        w, l = ops.resample(wav, lens, distinct[0], sr_out)
        return w, l, new_host
    B, N = wav.shape
    width = max(ops.resampled_length(N, r, sr_out) for r in distinct)
    out = torch.zeros(B, width, device=wav.device, dtype=torch.float32)
    out_lens = torch.empty(B, device=wav.device, dtype=torch.int32)
    for r in distinct:
        rows = torch.tensor([i for i, x in enumerate(rates) if x == r], device=wav.device)
        w, l = ops.resample(wav.index_select(0, rows), lens.index_select(0, rows).contiguous(), r, sr_out)
        out[rows, : w.shape[1]] = w
        out_lens[rows] = l
    return out, out_lens, new_host


def to_model_batch(batch, device="cuda", pad_value=1.0, non_blocking=True):
    """A waveform_collate_fn batch -> the reference's model batch on `device`: the text
    tensors moved, input_values [B, T, 160] / attention_mask_audio [B, T] from the batched
    fbank kernel with custom_collate_fn's semantics (per-clip features, zero rows and mask 0
    past each clip's frames).  A batch with "sampling_rates" is resampled to 16 kHz on the GPU
    first (ops.resample), where the reference's workers resample on the CPU (ref:1927)."""
    from . import ops
    dev = torch.device(device)
    skip = ("waveform", "lengths", "sampling_rates")
    out = {k: v.to(dev, non_blocking=non_blocking) for k, v in batch.items() if k not in skip}
    wav = batch["waveform"].to(dev, non_blocking=non_blocking)
    lens = batch["lengths"].to(dev, non_blocking=non_blocking)
    host = [int(n) for n in batch["lengths"].tolist()]
    if "sampling_rates" in batch:
        wav, lens, host = resample_batch(wav, lens, host, batch["sampling_rates"])
    T = max(1, max(num_frames(n) for n in host))
    feats, mask = ops.fbank(wav, lens, T, pad_value=pad_value, mask_mode=0)
    out["input_values"] = feats
    out["attention_mask_audio"] = mask
    # host-known frame counts: SpecAugment's span sampling reads these instead of the device mask
    out["audio_lengths"] = [num_frames(n) for n in host]
    return out


class LengthBucketBatchSampler(torch.utils.data.Sampler):
    """Length-bucketed batches: each epoch permutes the indices (seed + epoch), cuts the
    permutation into pools of `pool_batches` batches, sorts every pool by length (longest
    first) and cuts it into batches, then shuffles the batch order.  Every index appears
    once per epoch; clips in a batch have similar lengths, so the padded T (the encoders'
    work) follows the batch's own clips instead of the longest clip in a random batch."""

    def __init__(self, lengths, batch_size, *, pool_batches=50, shuffle=True, drop_last=False, seed=0):
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.batch_size, self.pool_batches = int(batch_size), max(1, int(pool_batches))
        self.shuffle, self.drop_last, self.seed = shuffle, drop_last, int(seed)
        self.epoch = 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def _batches(self):
        n = len(self.lengths)
        rng = np.random.default_rng(self.seed + self.epoch)
        order = rng.permutation(n) if self.shuffle else np.arange(n)
        pool = self.batch_size * self.pool_batches
        batches = []
        for s in range(0, n, pool):
            chunk = order[s:s + pool]
            chunk = chunk[np.argsort(-self.lengths[chunk], kind="stable")]
            for b in range(0, len(chunk), self.batch_size):
                batches.append(chunk[b:b + self.batch_size].tolist())
        if self.drop_last:
            batches = [b for b in batches if len(b) == self.batch_size]
        if self.shuffle:
            batches = [batches[i] for i in rng.permutation(len(batches))]
        return batches

    def __iter__(self):
        return iter(self._batches())

    def __len__(self):
        n = len(self.lengths)
        if not self.drop_last:
            pools, rem = divmod(n, self.batch_size * self.pool_batches)
            return pools * self.pool_batches + math.ceil(rem / self.batch_size)
        return len(self._batches())
