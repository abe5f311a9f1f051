"""Time fba_reliability against fba_covariance after two Gauss-Newton iterations of a benchmark scene, the
"reliability timing ..." lines of profiles/reliability_gpu_errors.log:  python scripts/rel_time.py [config ...]

Per entry point: a warm-up call on one context, then the wall time around the call on a second, fresh context of
the same kind (the device synchronise, the copies back and that context's workspace allocation included).  ONE
measurement per figure."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stepped(fba, ds):
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))
    for _ in range(2):
        ctx.step()
    return ctx, ctx.residuals()[2][3]


def _timed(fba, ds, name):
    """(first call on one context, call on a second context) in ms, and the second call's outputs"""
    out, ms = None, []
    for _ in range(2):
        ctx, s02 = _stepped(fba, ds)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = getattr(ctx, name)(s02)
        ms.append((time.perf_counter() - t0) * 1e3)
        ctx.close()
    return ms[0], ms[1], out


def main():
    import fba_import
    fba = fba_import.load()
    from fba_amd import synth
    for config in [int(a) for a in sys.argv[1:]] or [3, 4]:
        folder = os.path.join(os.environ.get("FBA_BENCH_DIR", "/tmp/fba_bench"), f"c{config}")
        if not os.path.exists(os.path.join(folder, ".done")):
            synth.make_config(config, folder)
            open(os.path.join(folder, ".done"), "w").close()
        ds = fba.load_folder(folder)
        c0, c1, (cx, _) = _timed(fba, ds, "covariance")
        r0, r1, (_, _, r, _) = _timed(fba, ds, "reliability")
        n, u = 2 * ds.n_pts, len(cx)
        print(f"reliability timing config {config}: n={n} u={u} fba_covariance {c1:.1f} ms (first call {c0:.1f}), "
              f"fba_reliability {r1:.1f} ms (first call {r0:.1f}); r min/max {r.min():.4f}/{r.max():.4f} "
              f"sum r - (n-u+7) {r.sum() - (n - u + 7):.2e}", flush=True)


if __name__ == "__main__":
    main()
