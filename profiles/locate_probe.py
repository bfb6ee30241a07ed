"""Timestamped search hits timed against the only routes the tree had before them.

    python profiles/locate_probe.py [--out profiles/locate_probe.json] [--rounds 5]

Q = 64 text queries, k = 10 candidate clips each, P = 768, 4 alignment heads, L = 64 tokens, clips of
T = 500 (10 s) and 1500 (30 s) frames.  Two draws of the candidate lists: "distinct" (640 different
clips) and "skewed" (one hub clip in every list, the other 576 candidates different clips).

(a) kernel: one ops.align_matrix_seg_fwd launch (matrix, emit and out) over the store's alignment rows
    in place, against what ste_align_matrix_fwd allows: it pairs clip b with transcript b, so every
    PAIR's rows are gathered into a dense [R, T, 2P] copy (index_select) and every pair's query block
    into [R·L, P], then one ops.align_matrix_fwd call with an all-ones mask.  The gathers and the
    kernel are also timed apart; max_abs_diff is over all three outputs.
(b) end to end at T = 500, full-size model with random weights: model.locate_clips against the store
    (one text pass, no audio pass) against re-encoding the candidate clips, the only way the earlier
    code had: one text pass, then per 64 distinct clips one audio-encoder pass and Engine.align_pairs
    on the (query, clip) pairs of those clips.

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
STEPS = [("kernel", 500, 20, 300), ("kernel", 1500, 10, 300), ("end_to_end", 500, 2, 900)]  # (kind, T, iters, limit s)


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
    kv = torch.empty(N * T, 2 * P, device=dev, dtype=bf16)
    for i in range(0, N * T, 64 * T):                              # filled in slices: no fp32 copy of the whole store
        kv[i:i + 64 * T] = torch.randn(64 * T, 2 * P, device=dev, generator=g).to(bf16)
    seg_row = torch.arange(N, device=dev, dtype=torch.int64) * T
    seg_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    R = Q * K
    qblk = (torch.arange(R, device=dev) // K).to(torch.int32)
    new = (torch.empty(R, L, T, device=dev), torch.empty(R, T, L, device=dev), torch.empty(R * L, P, device=dev, dtype=bf16))
    old = tuple(torch.empty_like(t) for t in new)
    mask = torch.ones(R * T, device=dev, dtype=torch.int32)
    for draw, idx in _draws(dev).items():
        pseg = idx.reshape(-1).contiguous()

        def seg():
            ops.align_matrix_seg_fwd(q, qblk, pseg, kv, seg_row, seg_len, L, T, NH, matrix=new[0], emit=new[1],
                                     out=new[2])

        rows = (seg_row[pseg.long()].view(R, 1) + torch.arange(T, device=dev).view(1, T)).reshape(-1)
        qrows = (qblk.long().view(R, 1) * L + torch.arange(L, device=dev).view(1, L)).reshape(-1)
        dense = {}

        def gather():
            dense["kv"] = kv.index_select(0, rows)
            dense["q"] = q.index_select(0, qrows)

        def matrix():
            ops.align_matrix_fwd(dense["q"], dense["kv"], mask, R, L, T, NH, matrix=old[0], emit=old[1], out=old[2])

        def route():
            gather()
            matrix()

        seg()
        route()
        torch.cuda.synchronize()
        res = {"step": "kernel", "draw": draw, "Q": Q, "k": K, "T": T, "L": L, "P": P, "heads": NH, "pairs": R,
               "distinct_clips": int(torch.unique(pseg).numel()), "iters_per_window": iters, "rounds": rounds,
               "dense_copy_bytes": R * T * 2 * P * 2,
               "max_abs_diff_vs_dense": max(float((a.float() - b.float()).abs().max()) for a, b in zip(new, old))}
        res.update(_timed({"align_matrix_seg_fwd": seg, "dense_gather_plus_matrix": route, "dense_gather": gather,
                           "align_matrix_on_dense": matrix}, iters, rounds))
        res["dense_over_seg"] = res["dense_gather_plus_matrix"]["ms_median"] / res["align_matrix_seg_fwd"]["ms_median"]
        res["seg_ms_per_64_pairs"] = res["align_matrix_seg_fwd"]["ms_median"] * 64 / R
        print(json.dumps(res), flush=True)
        dense.clear()


def end_to_end_step(T, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.retrieval import align_bytes_per_frame
    dev = "cuda"
    model = EnhancedAudioTextModel(use_word_alignment=True, device="cuda:0", spec_augment=False)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(7)
    CH = 64                                                         # clips per audio-encoder pass
    feats = [torch.randn(CH, T, 160, device=dev, generator=g) for _ in range(N // CH)]
    amask = torch.ones(CH, T, device=dev, dtype=torch.int64)
    ids = torch.randint(5, 250000, (Q, L), device=dev, generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    tmask = torch.ones(Q, L, device=dev, dtype=torch.int64)
    store = AudioStateStore(model, dev, reserve_frames=N * T, align_rows=True)
    for f in feats:
        store.add(f, amask)
    torch.cuda.synchronize()
    for draw, idx in _draws(dev).items():
        # the earlier route's plan: per 64 distinct clips, the (query, clip) pairs that name them
        flat = idx.reshape(-1).long()
        clips = torch.unique(flat)
        chunks = []
        for lo in range(0, clips.numel(), CH):
            cl = clips[lo:lo + CH]
            fv = torch.stack([feats[int(c) // CH][int(c) % CH] for c in cl.tolist()])
            pair = torch.isin(flat, cl).nonzero().view(-1)                     # flat slots q·K + c
            chunks.append((fv, amask[:cl.numel()], pair, pair // K, torch.searchsorted(cl, flat[pair])))

        def new():
            return model.locate_clips(ids, tmask, store, idx)

        def old(keep=None):
            with torch.no_grad():
                th = model.encode_text(ids, tmask)[1]
                for fv, am, pair, qq, cc in chunks:
                    ah = model.encode_audio(fv, am)[1]
                    r = model.engine.align_pairs(th.index_select(0, qq), tmask.index_select(0, qq),
                                                 ah.index_select(0, cc), am.index_select(0, cc))
                    if keep is not None:
                        keep.append((pair, r))

        r_new, kept = new(), []
        old(kept)
        spans = torch.empty(Q * K, L, 2, device=dev, dtype=torch.int32)
        conf = torch.empty(Q * K, L, device=dev)
        for pair, r in kept:
            spans[pair], conf[pair] = r["token_spans"], r["scores"]
        res = {"step": "end_to_end", "draw": draw, "Q": Q, "k": K, "T": T, "L": L, "P": model.projection_dim,
               "distinct_clips": int(clips.numel()), "audio_passes_old": len(chunks), "store_bytes": store.nbytes,
               "align_bytes_per_frame": align_bytes_per_frame(model.projection_dim),
               "iters_per_window": iters, "rounds": rounds,
               "spans_equal_fraction": float((spans == r_new["token_spans"].view(Q * K, L, 2)).all(-1).all(-1).float().mean()),
               "max_abs_confidence_diff": float((conf - r_new["scores"].view(Q * K, L)).abs().max())}
        res.update(_timed({"locate_clips": new, "reencode_and_align_pairs": old}, iters, rounds))
        res["old_over_new"] = res["reencode_and_align_pairs"]["ms_median"] / res["locate_clips"]["ms_median"]
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_probe.json"))
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
