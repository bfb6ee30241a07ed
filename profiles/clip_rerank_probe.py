"""Text -> clip reranking timed against the only routes the tree had before it.

    python profiles/clip_rerank_probe.py [--out profiles/clip_rerank_probe.json] [--rounds 5]

Q = 64 text queries, k = 10 candidate clips each, P = 768, 8 heads, L = 64 tokens, clips of T = 500
(10 s) and 1500 (30 s) frames.  Two draws of the candidate lists: "distinct" (640 different clips) and
"skewed" (one hub clip in every list, the other 576 candidates different clips).

(a) kernel: one ops.xattn_seg_fwd launch over the store's K/V buffer in place, against what the
    earlier kernels allow: gather the candidates' rows into a dense padded [G, T, 2P] copy
    (index_select) with a mask, then ops.xattn_mq_fwd on it (one launch for the clips retrieved once,
    one per clip retrieved more often).  The gather and the kernel are also timed apart.
(b) achieved bytes/s of (a): the K and V head slices of the distinct segments, G·T·2P·2 bytes, over
    the kernel's time.
(c) end to end at T = 500, full-size model with random weights: model.score_clips against the
    store (one text pass, no audio pass) against re-encoding the candidate clips, the only way the
    earlier code had: one text pass, then per 64 distinct clips one audio-encoder pass and
    Engine.score_pairs with the queries that retrieved them.  The one-time cost of building the
    store (AudioStateStore.add of 64 clips) is reported beside it.

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
Q, K, L, P, NH = 64, 10, 64, 768, 8
N = Q * K                                                        # clips in the corpus
STEPS = [("kernel", 500, 50, 300), ("kernel", 1500, 20, 300), ("end_to_end", 500, 2, 900)]  # (kind, T, iters, limit s)


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
    from speech_transcript_embeddings_amd.retrieval import plan_clip_pairs
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(T)
    q = torch.randn(Q, P, device=dev, generator=g) * 0.5
    kv = torch.empty(N * T, 2 * P, device=dev, dtype=torch.bfloat16)
    for i in range(0, N * T, 64 * T):                              # filled in slices: no fp32 copy of the whole store
        kv[i:i + 64 * T] = torch.randn(64 * T, 2 * P, device=dev, generator=g).to(torch.bfloat16)
    seg_row = torch.arange(N, device=dev, dtype=torch.int64) * T
    seg_len = torch.full((N,), T, device=dev, dtype=torch.int32)
    for draw, idx in _draws(dev).items():
        plan = plan_clip_pairs(idx)
        clips = plan["unique"].long()
        G, R = clips.numel(), Q * K
        srow, slen = seg_row[clips].contiguous(), seg_len[clips].contiguous()
        out_seg = torch.empty(R, P, device=dev)

        def seg():
            ops.xattn_seg_fwd(q, plan["qrow"], plan["pseg"], kv[:, :P], kv[:, P:], srow, slen, plan["tile_first"],
                              plan["tile_cnt"], NH, out_seg)

        # the dense route: rows of the G distinct clips gathered into [G, T, 2P], all-ones mask, and per
        # group of clips with the same number of queries one xattn_mq_fwd launch
        rows = (srow.view(G, 1) + torch.arange(T, device=dev).view(1, T)).reshape(-1)
        mask = torch.ones(G * T, device=dev, dtype=torch.int32)
        counts = torch.bincount(plan["pseg"].long(), minlength=G)
        first = torch.cumsum(counts, 0) - counts
        launches = []                                               # (first clip of dense, clips, C, qrow [n*C], pairs, out)
        once = (counts == 1).nonzero().view(-1)
        if once.numel() and not bool((once == torch.arange(int(once[0]), int(once[0]) + once.numel(), device=dev)).all()):
            raise RuntimeError("the clips retrieved once are not one run of the dense copy")   # the hub is clip 0
        for grp in ([once] if once.numel() else []) + [c.view(1) for c in (counts > 1).nonzero().view(-1)]:
            C = int(counts[grp[0]])
            pr = (first[grp].view(-1, 1) + torch.arange(C, device=dev).view(1, C)).reshape(-1)   # sorted pairs
            launches.append((int(grp[0]), grp.numel(), C, plan["qrow"][pr].contiguous(), pr,
                             torch.empty(pr.numel(), P, device=dev)))
        dense = {}

        def gather():
            dense["kv"] = kv.index_select(0, rows)

        def mq():
            d = dense["kv"].view(G, T, 2 * P)
            for lo, n, C, qrow, _, o in launches:
                blk = d[lo:lo + n].reshape(n * T, 2 * P)
                ops.xattn_mq_fwd(q, qrow, blk[:, :P], blk[:, P:], mask[:n * T], n, C, T, NH, o)

        def route():
            gather()
            mq()

        seg()
        route()
        torch.cuda.synchronize()
        old = torch.empty(R, P, device=dev)
        for _, _, _, _, pr, o in launches:
            old[pr] = o
        kv_bytes = G * T * 2 * P * 2
        res = {"step": "kernel", "draw": draw, "Q": Q, "k": K, "T": T, "P": P, "heads": NH, "pairs": R,
               "distinct_clips": G, "tiles": int(plan["tile_first"].numel()), "mq_launches": len(launches),
               "iters_per_window": iters, "rounds": rounds, "kv_bytes_distinct": kv_bytes,
               "max_abs_diff_vs_dense": float((old - out_seg).abs().max())}
        res.update(_timed({"xattn_seg_fwd": seg, "dense_gather_plus_mq": route, "dense_gather": gather,
                           "xattn_mq_on_dense": mq}, iters, rounds))
        res["dense_over_seg"] = res["dense_gather_plus_mq"]["ms_median"] / res["xattn_seg_fwd"]["ms_median"]
        res["seg_GBps"] = kv_bytes / (res["xattn_seg_fwd"]["ms_median"] * 1e-3) / 1e9
        res["mq_on_dense_GBps"] = kv_bytes / (res["xattn_mq_on_dense"]["ms_median"] * 1e-3) / 1e9
        print(json.dumps(res), flush=True)


def end_to_end_step(T, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import AudioStateStore
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.retrieval import plan_candidates
    dev = "cuda"
    model = EnhancedAudioTextModel(use_word_alignment=False, device="cuda:0", spec_augment=False)
    model.eval()
    g = torch.Generator(device=dev).manual_seed(7)
    CH = 64                                                         # clips per audio-encoder pass
    feats = [torch.randn(CH, T, 160, device=dev, generator=g) for _ in range(N // CH)]
    amask = torch.ones(CH, T, device=dev, dtype=torch.int64)
    ids = torch.randint(5, 250000, (Q, L), device=dev, generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    tmask = torch.ones(Q, L, device=dev, dtype=torch.int64)
    store = AudioStateStore(model, dev, reserve_frames=N * T)
    for f in feats:
        store.add(f, amask)
    torch.cuda.synchronize()

    def build_64():
        AudioStateStore(model, dev, reserve_frames=CH * T).add(feats[0], amask)

    for draw, idx in _draws(dev).items():
        # the earlier route's plan: per distinct clip, the queries that retrieved it
        clips, slots = plan_candidates(idx)
        G = clips.numel()
        counts = torch.bincount(slots.view(-1).long(), minlength=G)
        Cmax = int(counts.max())
        order = torch.sort(slots.view(-1).long(), stable=True)[1]
        col = torch.arange(order.numel(), device=dev) - (torch.cumsum(counts, 0) - counts)[slots.view(-1).long()[order]]
        table = torch.full((G, Cmax), -1, device=dev, dtype=torch.int32)      # [clip, c] -> query
        table[slots.view(-1).long()[order], col] = (order // K).to(torch.int32)
        chunks = []
        for lo in range(0, G, CH):
            cl = clips[lo:lo + CH].long()
            fv = torch.stack([feats[int(c) // CH][int(c) % CH] for c in cl.tolist()])
            tb = table[lo:lo + CH]
            width = max(int((tb >= 0).sum(1).max()), 1)
            chunks.append((fv, amask[:cl.numel()], tb[:, :width].contiguous()))

        def new():
            return model.score_clips(ids, tmask, store, idx)

        def old():
            with torch.no_grad():
                tproj, th = model.encode_text(ids, tmask)
                for fv, am, tb in chunks:
                    aproj, ah = model.encode_audio(fv, am)
                    model.engine.score_pairs(tproj, th, tmask, aproj, ah, am, tb)

        # the two routes give the same pair scores
        s_new = new()
        with torch.no_grad():
            tproj, th = model.encode_text(ids, tmask)
            s_old = torch.cat([torch.nn.functional.pad(
                model.engine.score_pairs(tproj, th, tmask, *model.encode_audio(fv, am), am, tb),
                (0, Cmax - tb.shape[1]), value=float("-inf")) for fv, am, tb in chunks])
        back = torch.full((Q, K), float("nan"), device=dev)
        live = table >= 0
        qq = table[live].long()
        cc = clips.view(G, 1).expand(G, Cmax)[live]
        pos = (idx[qq] == cc.view(-1, 1).to(idx.dtype)).to(torch.int8).argmax(1)
        back[qq, pos] = s_old[live]
        res = {"step": "end_to_end", "draw": draw, "Q": Q, "k": K, "T": T, "L": L, "P": model.projection_dim,
               "distinct_clips": G, "audio_passes_old": len(chunks), "store_bytes": store.nbytes,
               "iters_per_window": iters, "rounds": rounds, "max_abs_diff_vs_reencoding": float((back - s_new).abs().max())}
        res.update(_timed({"score_clips": new, "reencode_and_score_pairs": old, "store_add_64_clips": build_64},
                          iters, rounds))
        res["old_over_new"] = res["reencode_and_score_pairs"]["ms_median"] / res["score_clips"]["ms_median"]
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_rerank_probe.json"))
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
