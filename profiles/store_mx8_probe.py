"""The MX-fp8 audio-state store timed against the bf16 one on the same clips.

    python profiles/store_mx8_probe.py [--out profiles/store_mx8_probe.json] [--rounds 5]

The shapes and draws of clip_rerank_probe.py: Q = 64 text queries, k = 10 candidate clips each,
P = 768, 8 heads, L = 64 tokens, clips of T = 500 (10 s) and 1500 (30 s) frames; "distinct" (640
different clips) and "skewed" (one hub clip in every list).

(a) kernel: one ops.xattn_seg_fwd(ks=, vs=) launch over the e4m3 bytes and E8M0 scales against one
    ops.xattn_seg_fwd launch over the bf16 rows those bytes were quantised from, in ms and in TB/s of
    the bytes each one reads (the K and V head slices of the distinct segments: G·T·4P for bf16,
    G·T·(2P + P/16) for mx8).
(b) model.score_clips at T = 500 on a bf16 and on an mx8 store of the same clips (full-size model,
    random weights).  THE GATE: the mx8 time is at most 1.10 x the bf16 time of the same run; the
    attention kernel is 0.27 of score_clips (§18 c), so the kernel may be nearly 3 x slower before
    the gate trips.  The driver returns 1 if it does.
(c) AudioStateStore.add of 64 clips on both (the audio encoder pass included, as in §18).
(d) nbytes of both stores.

Each step runs in a fresh process under its own time limit; the driver never opens the GPU and stops
at the first step that fails.  Inside a step the variants are warmed up, then timed with device events
in interleaved rounds; the JSON holds the median, the minimum and the maximum over rounds.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_rerank_probe import K, L, N, NH, P, Q, _draws, _timed  # noqa: E402

STEPS = [("kernel", 500, 50, 300), ("kernel", 1500, 20, 300), ("end_to_end", 500, 2, 600)]  # (kind, T, iters, limit s)
GATE = 1.10


def kernel_step(T, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.retrieval import kv_bytes_per_frame, plan_clip_pairs
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(T)
    q = torch.randn(Q, P, device=dev, generator=g) * 0.5
    kv = torch.empty(N * T, 2 * P, device=dev, dtype=torch.bfloat16)
    kq = torch.empty(N * T, 2 * P, device=dev, dtype=torch.uint8)
    ksc = torch.empty(N * T, 2 * P // 32, device=dev, dtype=torch.uint8)
    for i in range(0, N * T, 64 * T):                              # filled in slices: no fp32 copy of the whole store
        kv[i:i + 64 * T] = torch.randn(64 * T, 2 * P, device=dev, generator=g).to(torch.bfloat16)
        ops.mx8_quant(kv[i:i + 64 * T], kq[i:i + 64 * T], ksc[i:i + 64 * T])
    seg_row = torch.arange(N, device=dev, dtype=torch.int64) * T
    seg_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    for draw, idx in _draws(dev).items():
        plan = plan_clip_pairs(idx)
        clips = plan["unique"].long()
        G, R = clips.numel(), Q * K
        srow, slen = seg_row[clips].contiguous(), seg_len[clips].contiguous()
        out_bf, out_mx = torch.empty(R, P, device=dev), torch.empty(R, P, device=dev)

        def bf():
            ops.xattn_seg_fwd(q, plan["qrow"], plan["pseg"], kv[:, :P], kv[:, P:], srow, slen, plan["tile_first"],
                              plan["tile_cnt"], NH, out_bf)

        def mx():
            ops.xattn_seg_fwd(q, plan["qrow"], plan["pseg"], kq[:, :P], kq[:, P:], srow, slen, plan["tile_first"],
                              plan["tile_cnt"], NH, out_mx, ks=ksc[:, :P // 32], vs=ksc[:, P // 32:])

        bf()
        mx()
        torch.cuda.synchronize()
        by = {kd: G * T * kv_bytes_per_frame(P, kd) for kd in ("bf16", "mx8")}
        res = {"step": "kernel", "draw": draw, "Q": Q, "k": K, "T": T, "P": P, "heads": NH, "pairs": R,
               "distinct_clips": G, "tiles": int(plan["tile_first"].numel()), "iters_per_window": iters,
               "rounds": rounds, "bytes_read_bf16": by["bf16"], "bytes_read_mx8": by["mx8"],
               "max_abs_diff_mx8_vs_bf16_rows": float((out_mx - out_bf).abs().max())}
        res.update(_timed({"xattn_seg_fwd": bf, "xattn_seg_mx8_fwd": mx}, iters, rounds))
        res["mx8_over_bf16"] = res["xattn_seg_mx8_fwd"]["ms_median"] / res["xattn_seg_fwd"]["ms_median"]
        res["bf16_TBps"] = by["bf16"] / (res["xattn_seg_fwd"]["ms_median"] * 1e-3) / 1e12
        res["mx8_TBps"] = by["mx8"] / (res["xattn_seg_mx8_fwd"]["ms_median"] * 1e-3) / 1e12
        print(json.dumps(res), flush=True)


def end_to_end_step(T, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    dev = "cuda"
    model = EnhancedAudioTextModel(use_word_alignment=False, device="cuda:0", spec_augment=False)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(7)
    CH = 64                                                         # clips per audio-encoder pass
    amask = torch.ones(CH, T, device=dev, dtype=torch.int64)
    ids = torch.randint(5, 250000, (Q, L), device=dev, generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    tmask = torch.ones(Q, L, device=dev, dtype=torch.int64)
    stores = {kd: AudioStateStore(model, dev, reserve_frames=N * T, kv_dtype=kd) for kd in ("bf16", "mx8")}
    for _ in range(N // CH):                                        # one encoder pass feeds both stores
        feats = torch.randn(CH, T, 160, device=dev, generator=g)
        with torch.no_grad():
            enc = model.encode_audio(feats, amask)
        for st in stores.values():
            st.add(feats, amask, audio_encoded=enc)
    torch.cuda.synchronize()
    for draw, idx in _draws(dev).items():
        variants = {f"score_clips_{kd}": (lambda st=st: model.score_clips(ids, tmask, st, idx)) for kd, st in stores.items()}
        variants.update({f"store_add_64_clips_{kd}": (lambda kd=kd: AudioStateStore(
            model, dev, reserve_frames=CH * T, kv_dtype=kd).add(feats, amask)) for kd in stores})
        s = {kd: variants[f"score_clips_{kd}"]() for kd in stores}
        res = {"step": "end_to_end", "draw": draw, "Q": Q, "k": K, "T": T, "L": L, "P": model.projection_dim,
               "clips": len(stores["bf16"]), "frames": stores["bf16"].rows, "iters_per_window": iters, "rounds": rounds,
               "store_bytes_bf16": stores["bf16"].nbytes, "store_bytes_mx8": stores["mx8"].nbytes,
               "store_bytes_mx8_over_bf16": stores["mx8"].nbytes / stores["bf16"].nbytes,
               "max_abs_score_diff_mx8_vs_bf16": float((s["mx8"] - s["bf16"]).abs().max()),
               "score_range_bf16": [float(s["bf16"].min()), float(s["bf16"].max())]}
        res.update(_timed(variants, iters, rounds))
        res["score_clips_mx8_over_bf16"] = res["score_clips_mx8"]["ms_median"] / res["score_clips_bf16"]["ms_median"]
        res["gate"] = GATE
        res["gate_ok"] = res["score_clips_mx8_over_bf16"] <= GATE
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_mx8_probe.json"))
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
    return 0 if all(r.get("gate_ok", True) for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
