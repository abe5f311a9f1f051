"""ms per damped trial against ms per plain Gauss-Newton step, the "damping cost ..." lines of
profiles/damping_ab_bench.log:   python scripts/lm_time.py

Config 4, one context, one process: a plain fba_step; fba_cost alone; a damped trial EMULATED from Python, call by
call (a blocking device copy of xhat's size through ctypes, fba_set_damping with a new lambda, fba_step, fba_cost: the
figure includes those calls' Python and ctypes round trips, which fba_adjust_lm does not make); and fba_adjust_lm
itself from file values, the whole call divided by its rows (the switch of damping on and off re-captures both
graphs once per call, so this figure lies above a trial's).  bench.py's measurement (warm-up, then the wall time
around K repetitions, device synchronised before and after).  ONE measurement per figure: compare the figures of a
run with each other, not with another session's."""
import ctypes
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fba_import  # noqa: E402
fba = fba_import.load()
from fba_amd import synth  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
hip.hipFree.argtypes = [ctypes.c_void_p]


def timed(ctx, body, warmup=3, reps=20):
    for _ in range(warmup):
        body()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        body()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


tmp = tempfile.mkdtemp()
ds = fba.load_folder(synth.make_config(4, os.path.join(tmp, "c4")))
shutil.rmtree(tmp)
ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))
# the trial's device copy of xhat, on a buffer of the same size (the reduce buffer's head: the size is what counts)
x0 = ctx.get_xhat()
src, n = ctx.reduce_buffer()
save = ctypes.c_void_p()
assert hip.hipMalloc(ctypes.byref(save), 8 * ctx.u) == 0 and n >= ctx.u
lam = [1e-3]


def trial():
    assert hip.hipMemcpy(save, src, 8 * ctx.u, 3) == 0  # device to device
    lam[0] = 1e-3 if lam[0] != 1e-3 else 1e-4           # a new lambda every trial, as the loop sets one
    ctx.set_damping(lam[0])
    ctx.step()
    ctx.cost()


plain = timed(ctx, ctx.step)
cost = timed(ctx, ctx.cost)
ctx.set_damping(1e-3)
damped_step = timed(ctx, ctx.step)
tr = timed(ctx, trial)
ctx.set_damping(0.0)
plain2 = timed(ctx, ctx.step)
assert hip.hipFree(save) == 0
rows = []


def whole():
    ctx.set_xhat(x0)
    nt, npol, _ = ctx.adjust_lm()
    rows[:] = [nt, npol]


lm = timed(ctx, whole, warmup=1, reps=5)
print(f"damping cost config 4 ({ds.numImg} images, {ds.n_pts} image points, u {ctx.u}): ms per plain fba_step {plain:.4f} "
      f"(again after the damped runs: {plain2:.4f}); per damped fba_step {damped_step:.4f}; per damped trial emulated "
      f"from Python (ctypes device copy + set_damping + step + cost) {tr:.4f}; per fba_cost alone {cost:.4f}  "
      f"[one measurement each, 20 repetitions]; fba_adjust_lm from file values, set_xhat included: {lm:.4f} ms per call "
      f"of {rows[0]} trials + {rows[1]} polish passes = {lm / sum(rows):.4f} per row  [one measurement, 5 repetitions]")
ctx.close()
