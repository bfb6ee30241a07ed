"""Time the layer-norm wav2vec2 feature-encoder kernels at XLSR shapes with HIP events (GPU probe).

    python profiles/w2v2_ln_probe.py kernels     # the four new kernels per conv layer, and
                                                 # ste_layernorm_fwd/bwd at the same rows x 512
    python profiles/w2v2_ln_probe.py step        # full XLSR-dims training step, b = 64 x 10 s, 3 + 3

B = 64 clips of 10 s: rows = 64·31,999 after conv0, halving per layer, C = 512.  Bytes are
algorithmic (what the kernel must read and write once), the rate is bytes / time.
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_transcript_embeddings_amd import _lib, ops  # noqa: E402
from speech_transcript_embeddings_amd._lib import ptr  # noqa: E402
from speech_transcript_embeddings_amd.modules import W2V2Config  # noqa: E402

BF16 = torch.bfloat16
DEV = "cuda"


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def report(out, name, us, nbytes):
    out[name] = dict(us=round(us, 1), gbytes=round(nbytes / 1e9, 3), tb_per_s=round(nbytes / us / 1e6, 3))
    print(f"{name}: {us:.1f} us, {nbytes / 1e9:.3f} GB, {nbytes / us / 1e6:.2f} TB/s", flush=True)


def kernels():
    c = W2V2Config(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
    B, N, C = 64, 160000, 512
    Ts = c.frames(N)
    s = _lib.stream_ptr()
    out = {}
    g, b = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.1
    Z = lambda: torch.zeros(C, device=DEV)  # noqa: E731
    # ---- conv0 + bias + LayerNorm + GELU
    K0, S0, T0 = c.conv_kernel[0], c.conv_stride[0], Ts[1]
    rows = B * T0
    wave = torch.randn(B, N, device=DEV)
    w0, bias = torch.randn(C, K0, device=DEV) * 0.3, torch.randn(C, device=DEV) * 0.1
    h = torch.empty(rows, C, device=DEV, dtype=BF16)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    us = timeit(lambda: _lib.call("ste_w2v_conv0_ln_fwd", ptr(wave), N, ptr(w0), ptr(bias), ptr(g), ptr(b), B, N, T0, C,
                                  K0, S0, 1e-5, ptr(h), ptr(mean), ptr(rstd), s))
    report(out, f"conv0_ln_fwd rows={rows}", us, 4 * B * N + rows * (2 * C + 8))
    dh = torch.randn(rows, C, device=DEV)
    nwork = int(_lib.fn("ste_w2v_conv0_ln_work")(B, T0, C, K0))
    work = torch.empty(nwork, device=DEV)
    dw0, dg, db, dbi = torch.zeros(C, K0, device=DEV), Z(), Z(), Z()
    us = timeit(lambda: _lib.call("ste_w2v_conv0_ln_bwd", ptr(dh), ptr(wave), N, ptr(mean), ptr(rstd), ptr(w0), ptr(bias),
                                  ptr(g), ptr(b), B, N, T0, C, K0, S0, ptr(dg), ptr(db), ptr(dbi), ptr(dw0), ptr(work),
                                  nwork, s))
    report(out, f"conv0_ln_bwd rows={rows}", us, 4 * B * N + rows * (4 * C + 8))
    del h, dh, work
    # ---- LayerNorm + GELU of layers 1.., and the existing LayerNorm kernels at the same shape
    for l in range(1, len(c.conv_dim)):
        rows = B * Ts[l + 1]
        z = torch.randn(rows, C, device=DEV).bfloat16()
        hb = torch.empty(rows, C, device=DEV, dtype=BF16)
        mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        us = timeit(lambda: _lib.call("ste_w2v_ln_gelu_fwd", ptr(z), ptr(g), ptr(b), rows, C, 1e-5, ptr(hb), 0,
                                      ptr(mean), ptr(rstd), s))
        report(out, f"L{l} ln_gelu_fwd rows={rows}", us, rows * (4 * C + 8))
        dhb = torch.randn(rows, C, device=DEV).bfloat16()
        dz = torch.empty(rows, C, device=DEV, dtype=BF16)
        nwork = int(_lib.fn("ste_w2v_ln_gelu_work")(rows, C))
        work = torch.empty(nwork, device=DEV)
        dg, db, dbi = Z(), Z(), Z()
        us = timeit(lambda: _lib.call("ste_w2v_ln_gelu_bwd", ptr(dhb), 1, ptr(z), ptr(mean), ptr(rstd), ptr(g), ptr(b),
                                      rows, C, ptr(dz), ptr(dg), ptr(db), ptr(dbi), ptr(work), nwork, s))
        report(out, f"L{l} ln_gelu_bwd (dh bf16) rows={rows}", us, rows * (6 * C + 8))
        # yardstick: ste_layernorm_fwd (fp32 in -> bf16) and ste_layernorm_bwd (dy bf16, x fp32 -> dxb bf16
        # + dgamma / dbeta / dsum) of the parent commit, same rows x 512
        x = torch.randn(rows, C, device=DEV)
        st = ops.layernorm_fwd(x, g, b, 1e-5, yb=hb)
        us = timeit(lambda: ops.layernorm_fwd(x, g, b, 1e-5, yb=hb, mean=st[0], rstd=st[1]))
        report(out, f"L{l} ste_layernorm_fwd (fp32 -> bf16) rows={rows}", us, rows * (6 * C + 8))
        dg, db, dbi = Z(), Z(), Z()
        us = timeit(lambda: ops.layernorm_bwd(dhb, x, st[0], st[1], g, beta=b, dxb=dz, dgamma=dg, dbeta=db, dsum=dbi))
        report(out, f"L{l} ste_layernorm_bwd (dy bf16, x fp32 -> bf16) rows={rows}", us, rows * (8 * C + 8))
        del z, hb, dhb, dz, work, x
    return out


def step():
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.train import TrainStep, synthetic_batch
    torch.manual_seed(0)
    B, nsamp, L = 64, 160000, 64
    model = EnhancedAudioTextModel(text_layers_to_unfreeze=3, audio_layers_to_unfreeze=3, freeze_encoders="partial",
                                   spec_augment=False, audio_model_name="facebook/wav2vec2-xls-r-300m",
                                   audio_embedding_dim=1024)
    model.audio_cfg.layerdrop = 0.0
    ts = TrainStep(model, warmup=100, total_steps=100000, micro_batch=B, max_text_length=L)
    data = synthetic_batch(B, nsamp, L, device=DEV, seed=0, rank=0)
    for _ in range(3):
        ts(*data)
    torch.cuda.synchronize()
    n = 8
    t0 = time.perf_counter()
    for _ in range(n):
        ts(*data)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    loss = float(ts.last["loss"].item())
    print(f"XLS-R 300m dims, b = {B} x 10 s, 3 + 3 unfrozen: {ms:.1f} ms/step, {B / ms * 1e3:.0f} pairs/s, loss {loss:.4f}, "
          f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
    return dict(ms_per_step=round(ms, 2), pairs_per_s=round(B / ms * 1e3, 1), loss=loss,
                peak_gib=round(torch.cuda.max_memory_allocated() / 2**30, 1))


if __name__ == "__main__":
    res = {sys.argv[1]: globals()[sys.argv[1]]()}
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
