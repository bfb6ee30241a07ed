"""bench.py's launcher and batch plan, without a GPU (STE_BENCH_PLAN_ONLY=1 stops each rank after
a gloo rendezvous and prints its plan).  `--gpus N` alone must start N ranks; under torchrun
WORLD_SIZE must match --gpus; the default global batch is c2's 64 at N=1 and c3's 256 at N>1,
split 256/N per rank in micro-batches of at most 64 (BASELINE configs)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(args, extra_env=None):
    env = dict(os.environ, STE_BENCH_PLAN_ONLY="1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, env=env,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


@pytest.mark.parametrize("n,local,micro,acc", [(1, 64, 64, 1), (2, 128, 64, 2), (4, 64, 64, 1)])
def test_launcher_spawns_ranks_and_plans_c3(n, local, micro, acc):
    plans = _run(["--gpus", str(n)])
    assert sorted(p["rank"] for p in plans) == list(range(n))
    for p in plans:
        assert p["world"] == n and p["local_rank"] == p["rank"]
        assert (p["local_batch"], p["micro_batch"], p["accumulation_steps"]) == (local, micro, acc)
        assert p["global_batch"] == (64 if n == 1 else 256)
        assert p["scaling"] == "strong"


def test_plan_c3_eight_ranks_and_overrides():
    from importlib import util
    spec = util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    b = util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.batch_plan(b.parse(["--gpus", "8"]), 8) == (256, 32, 32, 1, "strong")       # c3: 8 x 32
    assert b.batch_plan(b.parse(["--global-batch", "256"]), 1) == (256, 256, 64, 4, "strong")
    assert b.batch_plan(b.parse(["--batch", "64", "--gpus", "8"]), 8) == (512, 64, 64, 1, "weak")
    with pytest.raises(SystemExit):
        b.batch_plan(b.parse(["--global-batch", "100"]), 8)


def _bench_module():
    from importlib import util
    spec = util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    b = util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_full_and_dump_outputs_are_off_by_default():
    b = _bench_module()
    a = b.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 1)
    a = b.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_arrays_and_a_fixed_sample(tmp_path):
    """--dump-outputs: every array of the step's `last` dict plus the same seeded sample of the flat
    parameter and gradient buffers on every call, as float32 .npy files."""
    import types

    import numpy as np
    import torch
    b = _bench_module()
    n = 5000
    store = types.SimpleNamespace(n_grad=n, device=torch.device("cpu"),
                                  master=torch.arange(2 * n, dtype=torch.float32),
                                  grad=-torch.arange(n, dtype=torch.float32))
    model = types.SimpleNamespace(store=store)
    synced = []
    step = types.SimpleNamespace(sync=lambda: synced.append(1),
                                 last={"loss": torch.tensor([0.5]), "s_pos": torch.ones(4, dtype=torch.float64),
                                       "s_neg": torch.zeros(4)})
    b.dump_outputs(str(tmp_path / "a"), step, model, False)
    b.dump_outputs(str(tmp_path / "b"), step, model, False)
    assert synced
    names = {"loss", "s_pos", "s_neg", "params_sample", "grads_sample"}
    assert {p.stem for p in (tmp_path / "a").glob("*.npy")} == names
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].tolist() == [0.5] and got["s_pos"].tolist() == [1.0] * 4
    p, g = got["params_sample"], got["grads_sample"]
    assert p.shape == g.shape == (min(b.DUMP_SAMPLE, n),)
    assert (p < n).all() and np.array_equal(g, -p) and len(np.unique(p)) > n // 4   # trained entries, same indices
    for k in names:
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))
    # an evaluation step leaves no state behind: only what it returned
    b.dump_outputs(str(tmp_path / "e"), step, model, True)
    assert {p.stem for p in (tmp_path / "e").glob("*.npy")} == {"loss", "s_pos", "s_neg"}


def test_world_size_must_match_gpus():
    env = dict(os.environ, STE_BENCH_PLAN_ONLY="1", WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)
