"""The heads' fp32 GEMMs (ste_gemm_f32) of one training step, timed in isolation (HIP events) under
three plans of the same library — the per-launch numbers of DESIGN §16:

  tile64   every launch on 64x64 tiles, no split (ste_gemm_f32_plan_small_tiles(0))
  planned  the library's default: 32x32 tiles for launches with few tiles and no column sums
  split    the default plus the optional few-tile split-K (ste_gemm_f32_plan_max_tiles(64))

    python profiles/heads_gemm_probe.py [--batches 64,32] [--iters 200] [--warmup 20] [--repeats 3]
                                        [--graph] [--out profiles/heads_gemm_probe.json]

The launches are taken by tracing ops.gemm over one step of the bench workload (bench.py's c2
model and synthetic batch at each per-GPU batch), then replayed on the operands of that step, which
stay resident.  Per launch and plan: the median, minimum and maximum over --repeats of (--iters
launches between two events) / --iters, the slab count S and the tile; whether the default plan's
output equals the 64x64 tiling's bit for bit, and how far the split's is from it
(max |difference| / max |value|).

Under the A/B build (STE_LIB=.../libste_ab.so) the plan constants read STE_F32_MAX_TILES,
STE_F32_SMALL_TILES, STE_F32_SPLIT_WGS and STE_F32_SLAB_MIN_K; the output records them.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_FEATURES = (("B", "bias"), ("C2", "pre_out"), ("Z", "z"), ("R", "residual"), ("CS", "colsum"), ("RS", "row_scale"),
             ("C3", "out_bf16_copy"))


def trace_step(ops, step, data):
    """The fp32 ops.gemm calls of one step: (a, b, kwargs with out= the tensor the call wrote)."""
    calls = []
    real = ops.gemm

    def spy(a, b, **kw):
        out = real(a, b, **kw)
        if kw.get("mx8") is None and a.dtype == torch.float32:
            calls.append((a, b, dict(kw, out=out)))
        return out

    ops.gemm = spy
    try:
        step(*data)
        torch.cuda.synchronize()
    finally:
        ops.gemm = real
    return calls


def describe(ops, a, b, kw):
    a_kc, b_kc = kw.get("a_kc", True), kw.get("b_kc", True)
    M = kw.get("M") or (a.shape[-2] if a_kc else a.shape[-1])
    K = kw.get("K") or (a.shape[-1] if a_kc else a.shape[-2])
    N = kw.get("N") or (b.shape[-2] if b_kc else b.shape[-1])
    epi = "".join(f for f, k in _FEATURES if kw.get(k) is not None)
    epi += ("D" if kw.get("drop_p", 0.0) > 0 else "") + ("beta" if kw.get("beta", 0.0) != 0 else "")
    return {"M": M, "N": N, "K": K, "a_kc": int(a_kc), "b_kc": int(b_kc), "act": int(kw.get("act", 0)),
            "epilogue": epi or "plain", "caller_ws": kw.get("ws") is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,32")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--graph", action="store_true",
                    help="time one captured graph of the --iters launches (GPU time and launch gaps only) "
                         "instead of launching them from the host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_gemm_probe.json"))
    args = ap.parse_args()
    from speech_transcript_embeddings_amd import _lib, ops
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.train import TrainStep, synthetic_batch

    set_max, set_small = _lib.fn("ste_gemm_f32_plan_max_tiles"), _lib.fn("ste_gemm_f32_plan_small_tiles")
    default_small = set_small(0)
    set_small(default_small)
    # plan -> (small-tile threshold, split threshold): every launch on 64x64 tiles; the library's
    # default (32x32 tiles for few-tile launches, no split); the optional few-tile split on
    modes = {"tile64": (0, 0), "planned": (default_small, 0), "split": (default_small, 64)}

    def set_mode(mode):
        set_small(modes[mode][0])
        set_max(modes[mode][1])
    model = EnhancedAudioTextModel(use_word_alignment=False, text_layers_to_unfreeze=3, audio_layers_to_unfreeze=3,
                                   freeze_encoders="partial", device="cuda:0", spec_augment=False)
    model.audio_cfg.layerdrop = 0.0

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        graph = None
        if args.graph:   # the same launches replayed from one captured graph: no host time between them
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(args.iters):
                    fn()
            graph.replay()
            torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if graph is not None:
                graph.replay()
            else:
                for _ in range(args.iters):
                    fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / args.iters)
        return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    result = {"small_tiles": default_small, "timing": "graph replay" if args.graph else "host launches", "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
              "ab_env": {k: os.environ[k] for k in ("STE_F32_MAX_TILES", "STE_F32_SMALL_TILES", "STE_F32_SPLIT_WGS",
                                                          "STE_F32_SLAB_MIN_K")
                         if k in os.environ and _lib.AB_BUILD},
              "batches": {}}
    for b in [int(x) for x in args.batches.split(",")]:
        step = TrainStep(model, warmup=100, total_steps=100000, accumulation_steps=1, micro_batch=b,
                         max_text_length=64)
        data = synthetic_batch(b, 160000, 64, device="cuda:0", seed=0, rank=0)
        step(*data)                      # warm-up: caches, workspaces
        calls = trace_step(ops, step, data)
        rows = []
        for a, bm, kw in calls:
            d = describe(ops, a, bm, kw)
            # accumulating launches (beta, column sums) keep adding into their resident output: the
            # values drift, the time does not depend on them; compare the plans on a fresh copy
            out = kw["out"]
            keep = out.clone()
            cs = kw.get("colsum")
            cs_keep = None if cs is None else cs.clone()

            def once(mode, out=out, keep=keep, cs=cs, cs_keep=cs_keep, a=a, bm=bm, kw=kw):
                set_mode(mode)
                out.copy_(keep)
                if cs is not None:
                    cs.copy_(cs_keep)
                ops.gemm(a, bm, **kw)
                return out.float().clone()

            ref = once("tile64")
            d["planned_bitwise_equal"] = bool(torch.equal(once("planned"), ref))
            d["split_rel_diff"] = float((once("split") - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            # the timed launches go straight to the C ABI with the argument block ops.gemm built
            # under each plan (the workspace it chose included): no Python between the launches
            f32 = _lib.fn("ste_gemm_f32")
            for mode in modes:
                margs, S, tile = _gemm_args(_lib, ops, a, bm, kw, set_mode, mode)
                set_mode(mode)
                d[mode] = timed(lambda: f32(C.byref(margs), torch.cuda.current_stream().cuda_stream))
                d[mode].update(S=S, tile=tile)
            set_mode("planned")
            d["speedup"] = round(d["tile64"]["us"] / d["planned"]["us"], 2)
            out.copy_(keep)
            if cs is not None:
                cs.copy_(cs_keep)
            rows.append(d)
            print(json.dumps(d), flush=True)
        result["batches"][str(b)] = {
            "launches": len(rows), "launches_list": rows,
            **{"sum_%s_us" % m: round(sum(r[m]["us"] for r in rows), 1) for m in modes}}
        del step, calls
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "launches_list"}
                      for k, v in result["batches"].items()}))


def _gemm_args(_lib, ops, a, b, kw, set_mode, mode):
    """(the ste_gemm_args ops.gemm passes for this launch under the plan `mode`, its S, its tile)."""
    seen = {}
    real = ops.call

    def spy(name, *args):
        if name == "ste_gemm_f32":
            seen["args"] = _lib.GemmArgs.from_buffer_copy(args[0]._obj)
            seen["S"] = int(_lib.fn("ste_gemm_f32_plan")(args[0]))
            seen["tile"] = int(_lib.fn("ste_gemm_f32_plan_tile")(args[0]))
        return real(name, *args)

    set_mode(mode)
    ops.call = spy
    try:
        ops.gemm(a, b, **kw)
    finally:
        ops.call = real
    return seen["args"], seen["S"], seen["tile"]


if __name__ == "__main__":
    main()
