"""ms per Gauss-Newton step with prior observations of unknowns, the "priors cost ..." lines of
profiles/priors_ab_bench.log:   python scripts/priors_time.py

Config 4 with position priors (sigma 20) on all its images against config 4 without (one k_prior_cam launch, and
k_border_weights as a launch of its own); the routing of prior-carrying tie points to the general-point kernels at
its extreme, sigma = 1e30 on every tie coordinate, against the chunked run of the same scene (the 20-image scene of
tests/test_gpu_priors.py and config 3).  bench.py's measurement (warm-up steps, then the wall time around K steps of
one context, device synchronised before and after) on a fresh context per variant in one process.  ONE measurement
per figure: compare the figures of a line with each other, not with another session's."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fba_import  # noqa: E402
fba = fba_import.load()
from fba_amd import synth  # noqa: E402


def ms_per_step(ds, priors, warmup=2, steps=10):
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), priors=priors)
    try:
        for _ in range(warmup):
            ctx.step()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.step()
        ctx.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps
    finally:
        ctx.close()

root = tempfile.mkdtemp()
ds = fba.load_folder(synth.make_config(4, os.path.join(root, "c4")))
names = fba.xhat_names(ds)
idx = np.array([i for i, nm in enumerate(names) if nm.split("_")[0] in ("Xc", "Yc", "Zc")], dtype=np.int64)
x0 = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings)).buildxhat()
pri = (idx, x0[idx] + np.random.default_rng(1).normal(0, 20.0, len(idx)), np.full(len(idx), 20.0))
runs = {"plain": [], "priors": []}
for _ in range(3):
    runs["plain"].append(ms_per_step(ds, None))
    runs["priors"].append(ms_per_step(ds, pri))
print(f"priors cost config 4 ({ds.numImg} images, {len(idx)} position priors): ms_per_step without {sorted(runs['plain'])[1]:.4f} "
      f"with {sorted(runs['priors'])[1]:.4f} (medians of 3 alternating runs; all: {runs})")
sc = synth.generate(20, 300, seed=9, obs_per_point=6)
ds = fba.load_folder(synth.write_folder(sc, os.path.join(root, "u129"), nk=4))
u = len(fba.xhat_names(ds))
tidx = np.arange(u - 3 * ds.numtie, u, dtype=np.int64)
x0 = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings)).buildxhat()
allgen = (tidx, x0[tidx], np.full(len(tidx), 1e30))
runs = {"chunked": [], "general": []}
for _ in range(3):
    runs["chunked"].append(ms_per_step(ds, None))
    runs["general"].append(ms_per_step(ds, allgen))
print(f"priors cost all-general ({ds.numImg} images x {ds.numtie} points, {ds.n_pts} image points): ms_per_step chunked "
      f"{sorted(runs['chunked'])[1]:.4f} all points general {sorted(runs['general'])[1]:.4f} (medians of 3 alternating runs; all: {runs})")
# the same routing at config 3's size, where the general path's one-wave-per-point kernels have work to do
ds = fba.load_folder(synth.make_config(3, os.path.join(root, "c3")))
u = len(fba.xhat_names(ds))
tidx = np.arange(u - 3 * ds.numtie, u, dtype=np.int64)
x0 = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings)).buildxhat()
allgen = (tidx, x0[tidx], np.full(len(tidx), 1e30))
a, b = ms_per_step(ds, None), ms_per_step(ds, allgen)
print(f"priors cost all-general config 3 ({ds.numImg} images x {ds.numtie} points, {ds.n_pts} image points): ms_per_step chunked {a:.4f} "
      f"all points general {b:.4f}")
