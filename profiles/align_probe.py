"""Word timestamps timed against what a user has without the two kernels.

    python profiles/align_probe.py [--out profiles/align_probe.json] [--rounds 5]

B = 64 pairs, L = 64 tokens, P = 768, 4 alignment heads; T = 500 (10 s) and T = 1500 (30 s) frames;
ragged pairs (ntok in [L/2, L], nfrm in [T/2, T]; the decode step keeps nfrm = T, its longest chain).

(a) decode: ops.align_decode (one launch) against the same recurrence as a torch loop on the device,
    T steps of elementwise ops on [B, L] (shift, compare, select, add; the advance bits kept in a
    preallocated [T, B, L] tensor).  The loop does the forward pass only: its walk back would add
    T more gather steps, so the comparison favours the loop.
(b) the same against a device->host copy of the emissions plus the numpy reference of
    tests/kref_align.py (forward pass and walk back).
(c) matrix: ops.align_matrix_fwd (matrix + emit + out) against ops.align_attn_fwd (per-head
    probabilities to HBM) plus the head mean, clamp, log and transpose in torch.
(d) end to end, full-size model with random weights: model.align and its parts, the two encoders,
    the head (align.align_infer) and the decode.

Each step runs in a fresh process under its own time limit; the driver itself never opens the GPU
and stops at the first step that fails.  Inside a step the variants are warmed up, then timed with
device events in interleaved rounds; the JSON holds the median, the minimum and the maximum over
rounds.  The host variant of (b) ends in a device synchronise by construction (the copy).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B, L, P, NH = 64, 64, 768, 4
STEPS = [("decode", 500, 300), ("decode", 1500, 400), ("matrix", 500, 300), ("matrix", 1500, 300),
         ("end_to_end", 500, 600), ("end_to_end", 1500, 900)]                      # (kind, T, limit s)


def _timed(variants, rounds):
    """variants: name -> (fn, iterations per window)."""
    import torch

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn, iters in variants.values():     # warm-up: code objects, allocator, clocks
        window(fn, iters)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (fn, iters) in variants.items():
            times[name].append(window(fn, iters))
    return {name: {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts),
                   "iters_per_window": variants[name][1]} for name, ts in times.items()}


def _ragged(T, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    ntok = torch.randint(L // 2, L + 1, (B,), device=dev, generator=g).to(torch.int32)
    nfrm = torch.randint(T // 2, T + 1, (B,), device=dev, generator=g).to(torch.int32)
    return ntok, nfrm


def decode_step(T, rounds):
    import numpy as np
    import torch
    from kref_align import viterbi_batch_ref
    from speech_transcript_embeddings_amd import ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(T)
    emit = torch.log_softmax(torch.randn(B, T, L, device=dev, generator=g) * 2, dim=1).contiguous()
    ntok = _ragged(T, dev, T + 1)[0]
    nfrm = torch.full((B,), T, dtype=torch.int32, device=dev)      # every frame valid: the kernel's longest chain
    neg = torch.full((B, 1), float("-inf"), device=dev)
    adv = torch.empty(T, B, L, dtype=torch.bool, device=dev)
    out = {}

    def kernel():
        out["k"] = ops.align_decode(emit, ntok, nfrm)

    def loop():
        D = torch.full((B, L), float("-inf"), device=dev)
        D[:, 0] = emit[:, 0, 0]
        for t in range(1, T):
            left = torch.cat([neg, D[:, :-1]], 1)
            torch.gt(left, D, out=adv[t])
            D = torch.where(adv[t], left, D) + emit[:, t]
        out["l"] = D

    def host():
        e = emit.cpu().numpy()
        out["h"] = viterbi_batch_ref(e, ntok.cpu().numpy(), nfrm.cpu().numpy(), L)

    kernel(), loop(), host()
    torch.cuda.synchronize()
    spans, score = out["k"]
    loop_score = out["l"].gather(1, (ntok.long() - 1).view(B, 1)).view(B)
    res = {"step": "decode", "B": B, "L": L, "T": T, "rounds": rounds,
           "spans_equal_numpy": bool(np.array_equal(spans.cpu().numpy(), out["h"][0])),
           "score_equal_numpy": bool(np.array_equal(score.cpu().numpy(), out["h"][1])),
           "score_equal_torch_loop": bool(torch.equal(score, loop_score)),
           "torch_loop_launches": 4 * (T - 1) + 2}        # cat, gt, where, add per step
    res.update(_timed({"align_decode": (kernel, 200), "torch_loop_forward_only": (loop, 3), "host_numpy": (host, 1)},
                      min(rounds, 3) if T > 1000 else rounds))
    res["ns_per_frame"] = res["align_decode"]["ms_median"] * 1e6 / T
    res["loop_over_kernel"] = res["torch_loop_forward_only"]["ms_median"] / res["align_decode"]["ms_median"]
    res["host_over_kernel"] = res["host_numpy"]["ms_median"] / res["align_decode"]["ms_median"]
    print(json.dumps(res), flush=True)


def matrix_step(T, rounds):
    import torch
    from speech_transcript_embeddings_amd import ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(T)
    q = (torch.randn(B * L, P, device=dev, generator=g)).to(torch.bfloat16)
    kv = torch.randn(B * T, 2 * P, device=dev, generator=g).to(torch.bfloat16)
    _, nfrm = _ragged(T, dev, T + 2)
    mask = (torch.arange(T, device=dev).view(1, T) < nfrm.view(B, 1)).to(torch.int32).reshape(-1).contiguous()
    matrix, emit = torch.empty(B, L, T, device=dev), torch.empty(B, T, L, device=dev)
    att = torch.empty(B * L, P, device=dev, dtype=torch.bfloat16)
    probs = torch.empty(B * NH * L * T, device=dev)
    tiny = torch.finfo(torch.float32).tiny
    out = {}

    def new():
        ops.align_matrix_fwd(q, kv, mask, B, L, T, NH, matrix=matrix, emit=emit, out=att)

    def new_emit_out():
        ops.align_matrix_fwd(q, kv, mask, B, L, T, NH, emit=emit, out=att)

    def old():
        ops.align_attn_fwd(q, kv, mask, B, L, T, NH, probs, att)
        m = probs.view(B, NH, L, T).mean(1)
        out["m"], out["e"] = m, m.clamp_min(tiny).log().transpose(1, 2).contiguous()

    new(), old()
    torch.cuda.synchronize()
    res = {"step": "matrix", "B": B, "L": L, "T": T, "P": P, "heads": NH, "rounds": rounds,
           "max_abs_diff_matrix_vs_old": float((out["m"] - matrix).abs().max()),
           "max_abs_diff_emit_vs_old": float((out["e"] - emit).abs().max()),
           "probs_bytes_not_written": B * NH * L * T * 4}
    res.update(_timed({"align_matrix_fwd": (new, 50), "align_matrix_fwd_emit_out_only": (new_emit_out, 50),
                       "align_attn_fwd_plus_torch_mean_log": (old, 50)}, rounds))
    res["old_over_new"] = res["align_attn_fwd_plus_torch_mean_log"]["ms_median"] / res["align_matrix_fwd"]["ms_median"]
    print(json.dumps(res), flush=True)


def end_to_end_step(T, rounds):
    import torch
    from speech_transcript_embeddings_amd import ops
    from speech_transcript_embeddings_amd.align import align_infer
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    dev = "cuda"
    model = EnhancedAudioTextModel(use_word_alignment=True, device="cuda:0", spec_augment=False)
    model.eval()
    eng = model.engine
    g = torch.Generator(device=dev).manual_seed(7)
    feats = torch.randn(B, T, 160, device=dev, generator=g)
    ntok, nfrm = _ragged(T, dev, T + 3)
    amask = (torch.arange(T, device=dev).view(1, T) < nfrm.view(B, 1)).to(torch.int64)
    tmask = (torch.arange(L, device=dev).view(1, L) < ntok.view(B, 1)).to(torch.int64)
    ids = torch.randint(5, 250000, (B, L), device=dev, generator=g)
    ids[:, 0] = 0
    enc, hd = {}, {}

    def encoders():
        with torch.no_grad():
            enc["a"] = model.encode_audio(feats, amask)
            enc["t"] = model.encode_text(ids, tmask)

    def head():
        th, ah = enc["t"][1], enc["a"][1]
        thf = th.reshape(B * L, -1)
        thb = ops.cast_bf16(thf, torch.empty(thf.shape, device=dev, dtype=torch.bfloat16))
        ahf = ah.reshape(B * T, -1)
        ahb = ops.cast_bf16(ahf, torch.empty(ahf.shape, device=dev, dtype=torch.bfloat16))
        ctx = {"a_mask32": amask.to(torch.int32).reshape(-1), "_tmask_i64": tmask}
        hd["emit"] = align_infer(eng, thf, thb, ahb, B, L, T, ctx, want_matrix=False, want_emit=True)[2]

    def decode():
        ops.align_decode(hd["emit"], ntok, nfrm)

    def whole():
        model.align(feats, amask, ids, tmask)

    def reuse():
        model.align(feats, amask, ids, tmask, audio_encoded=enc["a"], text_encoded=enc["t"])

    encoders(), head()
    iters = 2 if T <= 500 else 1
    res = {"step": "end_to_end", "B": B, "L": L, "T": T, "P": model.projection_dim, "rounds": rounds}
    res.update(_timed({"model_align": (whole, iters), "encoders": (encoders, iters), "head_align_infer": (head, 10),
                       "decode": (decode, 50), "model_align_encoded_reuse": (reuse, 10)}, min(rounds, 3)))
    res["decode_share_of_align"] = res["decode"]["ms_median"] / res["model_align"]["ms_median"]
    res["head_share_of_align"] = res["head_align_infer"]["ms_median"] / res["model_align"]["ms_median"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_probe.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", type=int, default=None, help="internal: run step i in this process")
    a = ap.parse_args()
    if a.step is not None:
        kind, T, _ = STEPS[a.step]
        {"decode": decode_step, "matrix": matrix_step, "end_to_end": end_to_end_step}[kind](T, a.rounds)
        return 0
    results = []
    for i, (kind, T, limit) in enumerate(STEPS):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(i),
               "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"step {kind} T={T} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
