"""ms per Gauss-Newton step of a benchmark scene without weights, with per-observation weights and with weights
and the Huber loss, the "weights timing ..." line of profiles/weights_gpu_errors.log:
python scripts/weights_time.py [config ...]

bench.py's measurement (warm-up steps, then the wall time around K steps of one context, device synchronised
before and after), once per variant on a fresh context in one process.  ONE measurement per figure: compare the
three figures of a line with each other, not with another session's."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, STEPS = 2, 10


def _ms_per_step(fba, ds, weights, loss):
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))
    try:
        if weights is not None:
            ctx.set_weights(weights)
        if loss:
            ctx.set_loss(loss)
        for _ in range(WARMUP):
            ctx.step()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            ctx.step()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / STEPS
    finally:
        ctx.close()


def main():
    import fba_import
    fba = fba_import.load()
    from fba_amd import synth
    for config in [int(a) for a in sys.argv[1:]] or [4]:
        folder = os.path.join(os.environ.get("FBA_BENCH_DIR", "/tmp/fba_bench"), f"c{config}")
        if not os.path.exists(os.path.join(folder, ".done")):
            synth.make_config(config, folder)
            open(os.path.join(folder, ".done"), "w").close()
        ds = fba.load_folder(folder)
        wt = 10.0 ** np.random.default_rng(1).uniform(-1.0, 1.0, 2 * ds.n_pts)
        plain = _ms_per_step(fba, ds, None, None)
        weighted = _ms_per_step(fba, ds, wt, None)
        huber = _ms_per_step(fba, ds, wt, "huber")
        print(f"weights timing config {config}: n={2 * ds.n_pts} ms_per_step ({WARMUP} warm-up, {STEPS} steps, one "
              f"measurement each) unweighted {plain:.3f}, weights set {weighted:.3f}, weights + Huber(1.345) {huber:.3f}",
              flush=True)


if __name__ == "__main__":
    main()
