"""ste_resample at the data path's batch: 64 clips x 10 s at 48000 -> 16000 and 44100 -> 16000,
with ops.fbank on the 64 x 10 s batch it feeds as the in-project yardstick (DESIGN §"Resampling").

    python profiles/resample_probe.py [--clips 64] [--seconds 10] [--iters 30] [--out FILE]

HIP events on the current stream around every launch, after a warm-up; the median over --iters
launches.  The inputs rotate over three buffers (3 x 123 MB at 48 kHz, more than the 256 MB Infinity
Cache) so a launch does not find its samples cached by the previous one.  Floors: outputs·K·2 FLOP
against the fp32 vector peak (157.3 TFLOP/s) and the bytes read + written against the HBM peak
(8.0 TB/s, spec); the achieved fraction is floor / measured.  One JSON line."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from speech_transcript_embeddings_amd import ops  # noqa: E402

FP32_PEAK = 157.3e12   # FLOP/s, vector fp32 (spec)
HBM_PEAK = 8.0e12      # B/s (spec)


def timed(launches, iters, warmup=5):
    """Median / min / max microseconds per launch; launches[i % len] is launch i."""
    for i in range(warmup):
        launches[i % len(launches)]()
    torch.cuda.synchronize()
    evs = []
    for i in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches[i % len(launches)]()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in evs]
    return dict(median_us=round(statistics.median(us), 1), min_us=round(min(us), 1), max_us=round(max(us), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    assert torch.cuda.is_available(), "resample_probe.py measures on the GPU only"
    B = a.clips
    res = dict(clips=B, seconds=a.seconds, iters=a.iters, device=torch.cuda.get_device_name(0))
    for sr in (48000, 44100):
        M, L, K = ops.resample_plan(sr)
        N = int(sr * a.seconds)
        n_out = ops.resampled_length(N, sr)
        wavs = [torch.rand(B, N, device="cuda") * 2 - 1 for _ in range(3)]
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        out = torch.empty(B, n_out, device="cuda")
        t = timed([lambda w=w: ops.resample(w, lens, sr, out=out) for w in wavs], a.iters)
        flop = 2.0 * B * n_out * K
        nbytes = 4.0 * B * (N + n_out)
        t.update(M=M, L=L, K=K, tile=ops.resample_tile(sr), outputs=B * n_out, gflop=round(flop / 1e9, 2),
                 mbytes=round(nbytes / 1e6, 1), flop_floor_us=round(flop / FP32_PEAK * 1e6, 1),
                 hbm_floor_us=round(nbytes / HBM_PEAK * 1e6, 1))
        t["fraction_of_fp32_peak"] = round(t["flop_floor_us"] / t["median_us"], 3)
        t["fraction_of_hbm_peak"] = round(t["hbm_floor_us"] / t["median_us"], 3)
        res[f"resample_{sr}"] = t
        print(json.dumps({f"resample_{sr}": t}), flush=True)
        del wavs, out
    # the launch it feeds: fbank of the same 64 x 10 s batch at 16 kHz
    N16 = int(16000 * a.seconds)
    T = ((1 + (N16 - 400) // 160) + 1) // 2
    wavs = [torch.rand(B, N16, device="cuda") * 2 - 1 for _ in range(3)]
    lens = torch.full((B,), N16, dtype=torch.int32, device="cuda")
    feats = torch.empty(B, T, 160, device="cuda")
    mask = torch.empty(B, T, device="cuda", dtype=torch.int64)
    work = torch.empty(B * 2 * T * 80 + B * 160, device="cuda")
    res["fbank_16000"] = timed([lambda w=w: ops.fbank(w, lens, T, feats=feats, mask=mask, work=work) for w in wavs],
                               a.iters)
    for sr in (48000, 44100):
        res[f"resample_{sr}"]["times_fbank"] = round(res[f"resample_{sr}"]["median_us"] / res["fbank_16000"]["median_us"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
