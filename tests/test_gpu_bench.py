"""bench.py's command line at config 3 (200 images x 5k tie points), one fresh process per run.

A plain run prints the headline line only (`value`, `ms_per_step`, ...: no per-phase breakdown, roofline or
CPU baseline, which take runs of their own and come with --full), and --dump-outputs writes the xhat the
last timed step left: the same steps on a context in this process give the same xhat.  Both run the same
kernels on the same seeded scene, so they can differ only where a sum is taken in another order: held to
the bars the two-process run is held to against one context (tests/test_gpu_multiprocess.py), 1e-9 per
element and 1e-10 per parameter group.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, dist_scaling_of, elem_rel_err, group_rel_err

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("phase_ms", "roofline", "phase_roofline", "cpu_baseline", "gpu_vs_cpu")


@pytest.fixture(scope="module")
def bench_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bench")


def _bench(bench_dir, *args):
    env = dict(os.environ, FBA_BENCH_DIR=str(bench_dir / "scenes"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "3", *args],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_xhat(fba, bench_dir):
    steps, warmup = 2, 1
    dump = bench_dir / "dump"
    d = _bench(bench_dir, "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(dump))
    assert all(k in d for k in HEADLINE), sorted(d)
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    assert d["steps"] == steps and d["warmup"] == warmup and d["unit"] == "iter/s" and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    assert sorted(os.listdir(dump)) == ["xhat.npy"]
    x = np.load(dump / "xhat.npy")
    assert x.dtype == np.float64 and x.shape == (d["config"]["u"],) and np.all(np.isfinite(x))

    folder = str(bench_dir / "scenes" / "c3")  # the scene the run generated (seeded: synth.make_config)
    ds = fba.load_folder(folder)
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))
    try:
        dsum = [ctx.step() for _ in range(warmup + steps)]
        x_here = ctx.get_xhat()
    finally:
        ctx.close()
    assert abs(d["deltasum_last"] - dsum[-1]) <= 1e-9 * dsum[0], (d["deltasum_last"], dsum)
    names = fba.xhat_names(ds)
    dsc = dist_scaling_of(__import__("fba_oracle").load_folder(folder))
    err = group_rel_err(x, x_here, names, dsc)
    assert max(err.values()) <= 1e-10, err
    err = elem_rel_err(x, x_here, names, dsc)
    assert max(err.values()) <= 1e-9, err


def test_full_run_adds_the_breakdown_and_the_roofline(bench_dir):
    d = _bench(bench_dir, "--steps", "2", "--warmup", "1", "--full", "--no-cpu")
    assert all(k in d for k in HEADLINE), sorted(d)
    assert all(k in d for k in ("phase_ms", "roofline", "phase_roofline")), sorted(d)
    assert "cpu_baseline" not in d  # --no-cpu
    assert d["phase_ms"]["total"] > 0 and d["roofline"]["launches"] >= 1
