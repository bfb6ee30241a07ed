"""EmbeddingIndex.search timed against the only route the tree had before it.

    python profiles/retrieval_probe.py [--out profiles/retrieval_probe.json] [--rounds 5]

Q = 1024 queries, P = 256, k = 10, unit-norm random rows (seeded), N = 2^16 and 2^20, fp32 and
bf16 storage.  Baseline: ops.similarity into a materialised S, chunked over N (65,536 rows: a
256 MiB S) so that it fits, torch.topk per chunk, then a topk over the chunks' candidates.

Each N runs as a step in a fresh process under its own time limit; the driver itself never opens
the GPU and stops at the first step that fails.  Inside a step the three variants (fused fp32,
fused bf16, baseline) are warmed up, then timed with device events in interleaved rounds; the
JSON holds the median and the minimum over rounds, the fused path's share of the 157.3 TF f32
matrix peak (2·Q·N·P flop over the search time: a whole-call rate, merge and launches included)
and the baseline / fused ratio.  The step also checks that both routes return the same values.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q, P, K = 1024, 256, 10
PEAK_F32_MATRIX = 157.3e12
HBM_BYTES_PER_S = 6.0e12
STEPS = [(1 << 16, 300, 300), (1 << 20, 20, 600)]   # (N, searches per timed window, time limit in s)
BASE_CHUNK = 1 << 16


def step(N, iters, rounds):
    import torch
    from speech_transcript_embeddings_amd import EmbeddingIndex, ops
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(N)
    unit = lambda r: torch.nn.functional.normalize(torch.randn(r, P, device=dev, generator=g), dim=1)  # noqa: E731
    q, c = unit(Q), unit(N)
    ix32, ix16 = EmbeddingIndex(P, torch.float32, dev), EmbeddingIndex(P, torch.bfloat16, dev)
    ix32.add(c)
    ix16.add(c)
    assert N % BASE_CHUNK == 0
    S = torch.empty(Q, BASE_CHUNK, device=dev)

    def baseline():
        vs, js = [], []
        for lo in range(0, N, BASE_CHUNK):
            hi = min(N, lo + BASE_CHUNK)
            ops.similarity(q, c[lo:hi], S)
            v, j = torch.topk(S, K, dim=1)
            vs.append(v)
            js.append(j + lo)
        if len(vs) == 1:
            return vs[0], js[0]
        v, sel = torch.topk(torch.cat(vs, 1), K, dim=1)
        return v, torch.gather(torch.cat(js, 1), 1, sel)

    variants = {"fused_fp32": lambda: ix32.search(q, K), "fused_bf16": lambda: ix16.search(q, K), "baseline": baseline}
    # same values from both routes (the same MFMA chain scores a pair wherever it runs)
    vf, jf = variants["fused_fp32"]()
    vb, jb = baseline()
    torch.cuda.synchronize()
    assert torch.equal(vf, vb), "fused and baseline top-k values differ"
    same_idx = float((jf.long() == jb).float().mean())

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
    flop = 2.0 * Q * N * P
    out = {"N": N, "Q": Q, "P": P, "k": K, "iters_per_window": iters, "rounds": rounds,
           "splits": ops.topk_sim_plan(Q, N, P, K)[0], "indices_equal_fraction": same_idx}
    for name, ts in times.items():
        out[name] = {"ms_median": statistics.median(ts), "ms_min": min(ts)}
    for name, bytes_per_el in (("fused_fp32", 4), ("fused_bf16", 2)):
        t = out[name]["ms_median"] * 1e-3
        floor = max(flop / PEAK_F32_MATRIX, N * P * bytes_per_el / HBM_BYTES_PER_S)
        out[name].update(tflops=flop / t / 1e12, fraction_of_f32_matrix_peak=flop / t / PEAK_F32_MATRIX,
                         floor_ms=floor * 1e3,
                         floor_bound="f32 matrix rate" if floor == flop / PEAK_F32_MATRIX else "HBM",
                         baseline_over_fused=out["baseline"]["ms_median"] / out[name]["ms_median"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=None, help="internal: run step i in this process")
    a = ap.parse_args()
    if a.step is not None:
        N, iters, _ = STEPS[a.step]
        step(N, iters, a.rounds)
        return 0
    results = []
    for i, (N, _, limit) in enumerate(STEPS):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(i),
               "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"step N={N} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"peak_f32_matrix_tflops": PEAK_F32_MATRIX / 1e12, "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
