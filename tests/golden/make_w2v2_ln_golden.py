"""Golden vectors for the layer-norm wav2vec2 architecture (feat_extract_norm="layer",
conv_bias=True, do_stable_layer_norm=True: XLSR-53, XLS-R, the -lv60 family).

    python tests/golden/make_w2v2_ln_golden.py     (CPU, this container)

writes w2v2_ln_golden.npz (the parameters), w2v2_ln_golden_<case>.npz (one case's inputs and
expected outputs; three files so that each stays under the 1 MiB limit for committed files) and
w2v2_ln_golden.json (the config and cases).

The recipe of make_w2v2_golden.py (whose helpers this script uses) on the other architecture:
the in-container transformers Wav2Vec2Model at mini dims in float64, training mode with every
dropout / layerdrop / SpecAugment probability 0, LayerNorm affines and all biases randomised,
the same two cases (a ragged batch with a sample mask, a batch without one); forward
last_hidden_state and the gradient of Σ(last_hidden_state · cot) w.r.t. every parameter.
conv_dim = (64, 96, 64): the in- and out-channel counts of a conv layer differ.  Data only.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

import make_w2v2_golden as base

HERE = Path(__file__).resolve().parent
MINI = dict(base.MINI, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, conv_dim=(64, 96, 64))
CASES = base.CASES
NAME = "w2v2_ln_golden"


def build(seed=0):
    """make_w2v2_golden.build on this script's mini config."""
    saved = base.MINI
    base.MINI = MINI
    try:
        return base.build(seed)
    finally:
        base.MINI = saved


def main():
    m = build()
    np.savez_compressed(HERE / f"{NAME}.npz", **{"param/" + k: v.float().numpy() for k, v in m.state_dict().items()})
    for ci, (name, case) in enumerate(CASES.items()):
        x, mask = base.waves(case, 10 + ci)
        m.zero_grad(set_to_none=True)
        h = m(input_values=torch.from_numpy(x).double(),
              attention_mask=None if mask is None else torch.from_numpy(mask)).last_hidden_state
        cot = torch.randn(h.shape, generator=torch.Generator().manual_seed(100 + ci), dtype=torch.float64)
        (h * cot).sum().backward()
        out = {f"{name}/wave": x}
        if mask is not None:
            out[f"{name}/mask"] = mask
        out[f"{name}/hidden"] = h.detach().float().numpy()
        out[f"{name}/cot"] = cot.float().numpy()
        for n, p in m.named_parameters():
            assert p.grad is not None, n
            out[f"{name}/grad/{n}"] = p.grad.float().numpy()
        np.savez_compressed(HERE / f"{NAME}_{name}.npz", **out)
        print("wrote", HERE / f"{NAME}_{name}.npz", sum(v.size for v in out.values()), "values")
    (HERE / f"{NAME}.json").write_text(json.dumps({"config": MINI, "cases": CASES}, indent=1) + "\n")


def load():
    """Every array of the fixture as one dict (keys as in w2v2_golden.npz)."""
    z = {}
    for f in [NAME] + [f"{NAME}_{c}" for c in CASES]:
        with np.load(HERE / f"{f}.npz") as d:
            z.update({k: d[k] for k in d.files})
    return z


if __name__ == "__main__":
    main()
