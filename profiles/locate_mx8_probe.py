"""MX-fp8 alignment rows timed against the bf16 ones they replace, by the method of
profiles/locate_probe.py.

    python profiles/locate_mx8_probe.py [--out profiles/locate_mx8_probe.json] [--rounds 5]

Q = 64 text queries, k = 10 candidate clips each, P = 768, 4 alignment heads, L = 64 tokens, clips of
T = 500 (10 s) and 1500 (30 s) frames.  Two draws of the candidate lists: "distinct" (640 different
clips) and "skewed" (one hub clip in every list, the other 576 candidates different clips).

(a) kernel: one ops.align_matrix_seg_fwd(scales=...) launch (matrix, emit and out) over the e4m3 bytes and E8M0
    scales of 640 clips against one ops.align_matrix_seg_fwd launch over the bf16 rows of the same clips
    (the dequantised bytes, so the two launches compute the same bits: bits_equal).
(b) end to end at T = 500, full-size model with random weights: model.locate_clips on a store built with
    align_dtype="mx8" against one built with align_dtype="bf16", both fed by ONE encoder pass per 64
    clips (AudioStateStore.add(audio_encoded=...)); add of 64 clips into either store; nbytes of the
    640-clip stores for all four (kv_dtype, align_dtype) combinations.

Each step runs in a fresh process under its own time limit; the driver itself never opens the GPU
and stops at the first step that fails.  Inside a step the variants are warmed up, then timed with
device events in interleaved rounds; the JSON holds the median, the minimum and the maximum over
rounds.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q, K, L, P, NH = 64, 10, 64, 768, 4
N = Q * K                                                        # clips in the corpus
STEPS = [("kernel", 500, 20, 300), ("kernel", 1500, 10, 300), ("end_to_end", 500, 2, 400)]  # (kind, T, iters, limit s)


def _timed(variants, iters, rounds):
    import torch

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in variants.values():     # warm-up: code objects, allocator, clocks
        window(fn)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(window(fn))
    return {name: {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
            for name, ts in times.items()}


def _draws(dev):
    """The two candidate draws, int32 [Q, K] of clip ids in [0, N)."""
    import torch
    g = torch.Generator().manual_seed(11)
    distinct = torch.randperm(N, generator=g).view(Q, K)
    skewed = torch.cat([torch.zeros(Q, 1, dtype=torch.int64), 1 + torch.randperm(Q * (K - 1), generator=g).view(Q, K - 1)], 1)
    return {"distinct": distinct.to(dev, torch.int32), "skewed": skewed.to(dev, torch.int32)}


def kernel_step(T, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import ops
    dev, bf16 = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(T)
    q = (torch.randn(Q * L, P, device=dev, generator=g) * 0.5).to(bf16)
    kv8 = torch.empty(N * T, 2 * P, device=dev, dtype=torch.uint8)
    sc8 = torch.empty(N * T, 2 * P // 32, device=dev, dtype=torch.uint8)
    kv = torch.empty(N * T, 2 * P, device=dev, dtype=bf16)
    for i in range(0, N * T, 64 * T):                              # filled in slices: no fp32 copy of the whole store
        rows = torch.randn(64 * T, 2 * P, device=dev, generator=g).to(bf16)
        ops.mx8_quant(rows, kv8[i:i + 64 * T], sc8[i:i + 64 * T])
        ops.mx8_dequant(kv8[i:i + 64 * T], sc8[i:i + 64 * T], kv[i:i + 64 * T])
    seg_row = torch.arange(N, device=dev, dtype=torch.int64) * T
    seg_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    R = Q * K
    qblk = (torch.arange(R, device=dev) // K).to(torch.int32)
    new = (torch.empty(R, L, T, device=dev), torch.empty(R, T, L, device=dev), torch.empty(R * L, P, device=dev, dtype=bf16))
    old = tuple(torch.empty_like(t) for t in new)
    for draw, idx in _draws(dev).items():
        pseg = idx.reshape(-1).contiguous()

        def mx8():
            ops.align_matrix_seg_fwd(q, qblk, pseg, kv8, seg_row, seg_len, L, T, NH, scales=sc8, matrix=new[0],
                                     emit=new[1], out=new[2])

        def bf():
            ops.align_matrix_seg_fwd(q, qblk, pseg, kv, seg_row, seg_len, L, T, NH, matrix=old[0], emit=old[1],
                                     out=old[2])

        mx8()
        bf()
        torch.cuda.synchronize()
        res = {"step": "kernel", "draw": draw, "Q": Q, "k": K, "T": T, "L": L, "P": P, "heads": NH, "pairs": R,
               "distinct_clips": int(torch.unique(pseg).numel()), "iters_per_window": iters, "rounds": rounds,
               "row_bytes_bf16": 4 * P, "row_bytes_mx8": 2 * P + 2 * P // 32,
               "bits_equal": all(bool(torch.equal(a, b)) for a, b in zip(new, old))}
        res.update(_timed({"align_matrix_seg_mx8_fwd": mx8, "align_matrix_seg_fwd": bf}, iters, rounds))
        res["mx8_over_bf16"] = res["align_matrix_seg_mx8_fwd"]["ms_median"] / res["align_matrix_seg_fwd"]["ms_median"]
        print(json.dumps(res), flush=True)


def end_to_end_step(T, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame, kv_bytes_per_frame
    dev = "cuda"
    model = EnhancedAudioTextModel(use_word_alignment=True, device="cuda:0", spec_augment=False)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(7)
    CH = 64                                                         # clips per audio-encoder pass
    amask = torch.ones(CH, T, device=dev, dtype=torch.int64)
    ids = torch.randint(5, 250000, (Q, L), device=dev, generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    tmask = torch.ones(Q, L, device=dev, dtype=torch.int64)
    combos = [("bf16", "bf16"), ("mx8", "bf16"), ("bf16", "mx8"), ("mx8", "mx8")]     # (kv_dtype, align_dtype)
    stores = {c: AudioStateStore(model, dev, reserve_frames=N * T, kv_dtype=c[0], align_rows=True, align_dtype=c[1])
              for c in combos}
    enc = None
    for _ in range(N // CH):                                        # ONE encoder pass feeds every store
        with torch.no_grad():
            enc = model.encode_audio(torch.randn(CH, T, 160, device=dev, generator=g), amask)
        for st in stores.values():
            st.add(None, amask, audio_encoded=enc)
    torch.cuda.synchronize()
    nbytes = {f"kv_{c[0]}_align_{c[1]}": st.nbytes for c, st in stores.items()}
    per_frame = {f"kv_{c[0]}_align_{c[1]}": kv_bytes_per_frame(P, c[0]) + align_bytes_per_frame(P, c[1]) for c in combos}
    s_bf, s_mx = stores[("mx8", "bf16")], stores[("mx8", "mx8")]
    del stores

    def add_into(align_dtype):
        def add():
            st = AudioStateStore(model, dev, reserve_frames=CH * T, kv_dtype="mx8", align_rows=True,
                                 align_dtype=align_dtype)
            st.add(None, amask, audio_encoded=enc)
        return add

    adds = _timed({"add_64_clips_align_mx8": add_into("mx8"), "add_64_clips_align_bf16": add_into("bf16")}, iters, rounds)
    for draw, idx in _draws(dev).items():
        def mx8():
            return model.locate_clips(ids, tmask, s_mx, idx)

        def bf():
            return model.locate_clips(ids, tmask, s_bf, idx)

        a, b = mx8(), bf()
        res = {"step": "end_to_end", "draw": draw, "Q": Q, "k": K, "T": T, "L": L, "P": model.projection_dim,
               "distinct_clips": int(torch.unique(idx).numel()), "store_bytes": nbytes, "row_bytes_per_frame": per_frame,
               "iters_per_window": iters, "rounds": rounds,
               "spans_equal_fraction": float((a["token_spans"] == b["token_spans"]).all(-1).all(-1).float().mean()),
               "max_abs_confidence_diff": float((a["scores"] - b["scores"]).abs().max())}
        res.update(_timed({"locate_clips_align_mx8": mx8, "locate_clips_align_bf16": bf}, iters, rounds))
        res.update(adds)
        res["locate_mx8_over_bf16"] = res["locate_clips_align_mx8"]["ms_median"] / res["locate_clips_align_bf16"]["ms_median"]
        res["add_mx8_over_bf16"] = adds["add_64_clips_align_mx8"]["ms_median"] / adds["add_64_clips_align_bf16"]["ms_median"]
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_mx8_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=None, help="internal: run step i in this process")
    a = ap.parse_args()
    if a.step is not None:
        kind, T, iters, _ = STEPS[a.step]
        (kernel_step if kind == "kernel" else end_to_end_step)(T, iters, a.rounds)
        return 0
    results = []
    for i, (kind, T, _, limit) in enumerate(STEPS):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(i),
               "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"step {kind} T={T} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        for line in r.stdout.strip().splitlines():
            if line.startswith("{"):
                results.append(json.loads(line))
                print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
