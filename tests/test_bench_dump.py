"""bench.py's plain run and `--dump-outputs`: the budgeted, seeded writer on
stand-in fields (CPU), and one tiny plain run end to end (GPU): the line
carries the headline keys with everything behind `--full` left null, and the
last timed step's KL value, gradient and samples land in DIR as float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


class _F:
    def __init__(self, a):
        import torch
        self.val = torch.from_numpy(np.asarray(a, dtype=np.float64))


class _MF(dict):
    pass


class _Samples:
    def __init__(self, items, lo):
        self._items = items
        self.local_indices = range(lo, lo + len(items))

    def local_item(self, i):
        return self._items[i]


class _KL:
    def __init__(self, seed, lo=0):
        rng = np.random.default_rng(seed)
        self.value = float(rng.normal())
        self.gradient = _MF(xi=_F(rng.normal(size=(70, 50))), slope=_F(rng.normal(size=2)))
        self.samples = _Samples([_MF(xi=_F(rng.normal(size=(70, 50))), slope=_F(rng.normal(size=2)))
                                 for _ in range(2)], lo)


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_budget_and_seed(tmp_path, monkeypatch):
    kl = _KL(1)
    bench.dump_outputs(str(tmp_path / "whole"), kl, 0, 1)
    w = _load(tmp_path / "whole")
    assert sorted(w) == ["kl_gradient_slope", "kl_gradient_xi", "kl_value", "sample0_slope", "sample0_xi",
                         "sample1_slope", "sample1_xi"]
    assert all(a.dtype == np.float64 for a in w.values())
    assert w["kl_value"].tolist() == [kl.value]
    assert np.array_equal(w["kl_gradient_xi"], kl.gradient["xi"].val.numpy())
    assert np.array_equal(w["sample1_xi"], kl.samples.local_item(1)["xi"].val.numpy())
    # a budget the three 28000-byte arrays do not fit: the small ones whole,
    # the large ones cut to equal shares of what is left, the same entries of
    # each (and of a second run, also with other values)
    monkeypatch.setattr(bench, "DUMP_SMALL", 1000)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)
    bench.dump_outputs(str(tmp_path / "cut"), kl, 0, 1)
    c = _load(tmp_path / "cut")
    assert sorted(c) == sorted(w)
    assert sum(a.nbytes for a in c.values()) <= 20000
    n = c["kl_gradient_xi"].size
    assert n == (20000 - 8 - 3 * 16) // (8 * 3) and c["sample0_xi"].size == n and c["sample1_xi"].size == n
    assert np.array_equal(c["sample0_slope"], w["sample0_slope"])
    idx = np.sort(np.random.default_rng(3500).integers(0, 3500, n))
    for k in ("kl_gradient_xi", "sample0_xi", "sample1_xi"):
        assert np.array_equal(c[k], w[k].reshape(-1)[idx])
    # another rank of two: its own samples under their global indices, half
    # the budget, no KL value / gradient
    bench.dump_outputs(str(tmp_path / "r1"), _KL(2, lo=2), 1, 2)
    r = _load(tmp_path / "r1")
    assert sorted(r) == ["sample2_slope", "sample2_xi", "sample3_slope", "sample3_xi"]
    assert sum(a.nbytes for a in r.values()) <= 10000


@pytest.mark.gpu
def test_plain_run_line_and_dump(dev, tmp_path):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--backend", "none", "--size", "128",
           "--nlos", "500", "--samples-per-gpu", "1", "--lin-iters", "10", "--newton-iters", "1",
           "--newton-cg-max", "5", "--steps", "3", "--warmup", "1", "--dump-outputs", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    # 2 samples per step: value and ms_per_step are the same measurement
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(2e3 / d["ms_per_step"], rel=1e-4)
    assert d["cg_iters"] > 0
    for k in ("roofline", "cpu_baseline", "demo_controllers", "cg_iteration", "kernels", "distributed"):
        assert d[k] is None, k
    a = _load(out)
    keys = sorted(k[len("kl_gradient_"):] for k in a if k.startswith("kl_gradient_"))
    assert "xi" in keys and len(keys) >= 5
    assert sorted(a) == sorted(["kl_value"] + [f"{p}_{k}" for p in ("kl_gradient", "sample0", "sample1")
                                               for k in keys])
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in a.values())
    assert a["kl_value"].shape == (1,)
    for p in ("kl_gradient", "sample0", "sample1"):
        assert a[p + "_xi"].shape == (128, 128)
    # a mirrored pair: the two samples lie opposite each other about the
    # expansion point, so they differ
    assert np.any(a["sample0_xi"] != a["sample1_xi"])
