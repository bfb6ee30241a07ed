"""Long recordings in the AudioStateStore timed, by the method of profiles/locate_probe.py.

    python profiles/recording_probe.py [--out profiles/recording_probe.json] [--rounds 5]

One recording of F = 30,000 frames (10 minutes), windows of 1500 frames every 750: W = 39 windows.

(a) kernel, H = 1024, Hh = 512, fp32: ops.attn_pool_seg_fwd over the 39 overlapping windows of the one
    buffer against the only route there was before it: index_select of every window's rows of t and h
    into dense [W, 1500, .] copies, then ops.attn_pool_fwd_f32 (the last window, 1500 frames here too).
    bits_equal says that both give the same pooled rows.
(b) AudioStateStore.add_recording of that recording into a fresh store, full-size model with random
    weights, use_word_alignment, bf16 rows, split with device events around its three parts: the
    encoder chunks, the row projections and writes, pooling + projection.
(c) search_recordings against search_clips on the same store (8 such recordings: 312 windows) at
    Q = 64, k = 10, L = 16 tokens, free_ends=True, with and without the neighbour windows.

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
F, WIN, HOP = 30000, 1500, 750
STEPS = [("kernel", 20, 300), ("add_recording", 1, 500), ("search", 2, 500)]  # (kind, iters per window, limit s)


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


def kernel_step(iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.retrieval import plan_recording
    dev, H, Hh = "cuda", 1024, 512
    g = torch.Generator(device=dev).manual_seed(23)
    t = torch.rand(F, Hh, device=dev, generator=g) * 2 - 1
    h = torch.randn(F, H, device=dev, generator=g)
    w2 = torch.randn(Hh, device=dev, generator=g) * (4.0 / Hh ** 0.5)
    b2 = torch.zeros(1, device=dev)
    plan = plan_recording(F, WIN, HOP, 1000, 250)
    W = len(plan["window_start"])
    assert set(plan["window_len"]) == {WIN}
    seg_row = torch.tensor(plan["window_start"], dtype=torch.int64, device=dev)
    seg_len = torch.tensor(plan["window_len"], dtype=torch.int32, device=dev)
    rows = (seg_row.view(W, 1) + torch.arange(WIN, device=dev).view(1, WIN)).reshape(-1)
    new, old = torch.empty(W, H, device=dev), torch.empty(W, H, device=dev)
    weights = torch.empty(W * WIN, device=dev)

    def seg():
        ops.attn_pool_seg_fwd(t, w2, b2, h, seg_row, seg_len, new)

    def gather_dense():
        ops.attn_pool_fwd_f32(t.index_select(0, rows), w2, b2, h.index_select(0, rows), None, W, WIN, weights, old)

    tg, hg = t.index_select(0, rows), h.index_select(0, rows)

    def dense_only():
        ops.attn_pool_fwd_f32(tg, w2, b2, hg, None, W, WIN, weights, old)

    seg()
    gather_dense()
    torch.cuda.synchronize()
    copy_bytes = W * WIN * (H + Hh) * 4
    res = {"step": "kernel", "F": F, "H": H, "Hh": Hh, "window": WIN, "hop": HOP, "windows": W, "dtype": "fp32",
           "iters_per_window": iters, "rounds": rounds, "bits_equal": bool(torch.equal(new, old)),
           "gather_copy_bytes": copy_bytes, "buffer_bytes": F * (H + Hh) * 4}
    res.update(_timed({"attn_pool_seg_fwd": seg, "index_select_then_attn_pool_fwd_f32": gather_dense,
                       "attn_pool_fwd_f32_on_the_copies": dense_only}, iters, rounds))
    seg_ms = res["attn_pool_seg_fwd"]["ms_median"]
    res["seg_over_gather_dense"] = seg_ms / res["index_select_then_attn_pool_fwd_f32"]["ms_median"]
    # the segmented route reads t once (score) and every window's rows of h (wsum): its share of 8 TB/s
    res["seg_bytes_read"] = F * Hh * 4 + W * WIN * H * 4
    res["seg_share_of_8TBps"] = res["seg_bytes_read"] / (seg_ms * 1e-3) / 8e12
    # the dense route writes the copies, reads them back, and read the rows to make them
    res["gather_dense_bytes_moved"] = 3 * copy_bytes
    res["gather_dense_share_of_8TBps"] = (3 * copy_bytes / (res["index_select_then_attn_pool_fwd_f32"]["ms_median"] * 1e-3)
                                          / 8e12)
    print(json.dumps(res), flush=True)


def _model():
    import torch  # noqa: F401
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    model = EnhancedAudioTextModel(use_word_alignment=True, device="cuda:0", spec_augment=False)
    model.eval()
    return model


def add_recording_step(iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import AudioStateStore, ops
    from speech_transcript_embeddings_amd.align import audio_kv
    from speech_transcript_embeddings_amd.retrieval import plan_recording
    dev = "cuda"
    model = _model()
    eng = model.engine
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(F, 160, device=dev, generator=g)

    def add():
        st = AudioStateStore(model, dev, reserve_frames=F, align_rows=True)
        st.add_recording(x)
        return st

    st = add()
    res = {"step": "add_recording", "F": F, "window": WIN, "hop": HOP, "chunk": 1000, "context": 250, "chunk_batch": 8,
           "windows": len(st), "rows": st.rows, "store_bytes": st.nbytes, "iters_per_window": iters, "rounds": rounds,
           "encoder_frames_run": sum(b - a for a, b in plan_recording(F, WIN, HOP, 1000, 250)["input"])}
    # the three parts, by hand with add_recording's own calls
    plan = plan_recording(F, WIN, HOP, 1000, 250)
    chunks = list(zip(plan["keep"], plan["input"]))
    D = eng.acfg.hidden_size
    h = torch.empty(F, D, device=dev)
    hs = torch.empty(F, 2 * D, device=dev, dtype=torch.bfloat16)
    seg_row = torch.tensor(plan["window_start"], dtype=torch.int64, device=dev)
    seg_len = torch.tensor(plan["window_len"], dtype=torch.int32, device=dev)
    bank = AudioStateStore(model, dev, reserve_frames=F, align_rows=True)

    @torch.no_grad()
    def encoder():
        for c0 in range(0, len(chunks), 8):
            part = chunks[c0:c0 + 8]
            T = max(b - a for _, (a, b) in part)
            feats = x.new_zeros(len(part), T, 160)
            mask = torch.zeros(len(part), T, dtype=torch.int64, device=dev)
            for j, (_, (a, b)) in enumerate(part):
                feats[j, :b - a] = x[a:b]
                mask[j, :b - a] = 1
            ctx = {}
            hc, _ = eng.audio_forward(feats, mask, False, 0, ctx, save=False)
            for j, ((ka, kb), (a, _)) in enumerate(part):
                h[ka:kb] = hc[j * T + ka - a:j * T + kb - a]
                hs[ka:kb] = ctx["a_hs"][j * T + ka - a:j * T + kb - a]

    @torch.no_grad()
    def rows():
        hb = ops.cast_bf16(h, torch.empty(F, D, device=dev, dtype=torch.bfloat16))
        bank.kv_bank.write(0, eng._kv("text_to_audio_attention", "audio_seq_to_projection", hb)[0], [F], F)
        bank.align_bank.write(0, audio_kv(eng, hb), [F], F)

    @torch.no_grad()
    def pool_project():
        pooled = eng._pool_seg_fwd("audio_pooling", h, hs, seg_row, seg_len)
        eng._proj_fwd("audio_projection", pooled, len(plan["window_start"]), False, 0, {})

    model.store.sync_shadow()
    encoder()
    res.update(_timed({"add_recording": add, "encoder_chunks": encoder, "row_projections_and_writes": rows,
                       "pooling_and_projection": pool_project}, iters, rounds))
    print(json.dumps(res), flush=True)


def search_step(iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import AudioStateStore, search_clips, search_recordings
    dev, Q, K, L, NREC = "cuda", 64, 10, 16, 8
    model = _model()
    g = torch.Generator(device=dev).manual_seed(9)
    st = AudioStateStore(model, dev, reserve_frames=NREC * F, align_rows=True)
    for _ in range(NREC):
        st.add_recording(torch.randn(F, 160, device=dev, generator=g))
    ids = torch.randint(5, 250000, (Q, L), device=dev, generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    tmask = torch.ones(Q, L, device=dev, dtype=torch.int64)

    def clips():
        return search_clips(model, st, ids, tmask, K, free_ends=True)

    def recs():
        return search_recordings(model, st, ids, tmask, K)

    def recs_centre():
        return search_recordings(model, st, ids, tmask, K, neighbours=False)

    r = recs()
    res = {"step": "search", "Q": Q, "k": K, "L": L, "recordings": NREC, "windows": len(st), "rows": st.rows,
           "window": WIN, "hop": HOP, "windows_searched": min(4 * K, 128, len(st)), "iters_per_window": iters,
           "rounds": rounds, "distinct_recordings_per_query": float((r[1] >= 0).sum(1).float().mean())}
    res.update(_timed({"search_clips_k10": clips, "search_recordings_k10": recs,
                       "search_recordings_k10_no_neighbours": recs_centre}, iters, rounds))
    res["recordings_over_clips"] = res["search_recordings_k10"]["ms_median"] / res["search_clips_k10"]["ms_median"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recording_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=None, help="internal: run step i in this process")
    a = ap.parse_args()
    fns = {"kernel": kernel_step, "add_recording": add_recording_step, "search": search_step}
    if a.step is not None:
        kind, iters, _ = STEPS[a.step]
        fns[kind](iters, a.rounds)
        return 0
    results = []
    for i, (kind, _, limit) in enumerate(STEPS):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(i),
               "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"step {kind} failed with status {r.returncode}; stopping", file=sys.stderr)
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
