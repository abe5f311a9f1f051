"""Time fba_vce on a benchmark scene, groups "xy", against the same loop composed from Python on the same build
(fba_adjust, fba_residuals, fba_reliability, numpy sums, fba_set_weights), the lines of
profiles/vce_timing_config4.log:  python scripts/vce_time.py [config] [repetitions]

Per repetition, on fresh contexts: (a) fba_vce with fba_set_timing on -- fba_last_timings[7], the HIP-event time of the
call's own kernels (the reliability part and the group sums of every round), divided by the rounds; (b) fba_vce with
timing off: the wall time of the whole call; (c) the composed loop: the wall time from the first fba_adjust to the last
fba_step.  Medians over the repetitions (default 7), after one warm-up of each."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def composed(ctx, group, ng, sx, sy, max_rounds=10, tol=1e-3, min_redundancy=1.0, clip=100.0):
    """fba_vce's rounds from Python: every round copies r and v (2 n_pts each) to the host and uploads the weights"""
    n = group.size
    sig = np.where(np.arange(n) % 2 == 0, sx, sy)
    wt = np.ones(n)
    comp = np.ones(ng)
    rounds = 0
    for k in range(max_rounds):
        ctx.adjust()
        v, _, st = ctx.residuals()
        _, _, red, _ = ctx.reliability(st[3], corr=False)
        t = wt * (v / sig) ** 2
        R, T = np.bincount(group, red, ng), np.bincount(group, t, ng)
        rounds = k + 1
        ok = R >= min_redundancy
        e = np.clip(np.where(ok, T / np.where(ok, R, 1.0), 1.0), 1.0 / clip, clip)
        clipped = ok & ((T / np.where(ok, R, 1.0) < 1.0 / clip) | (T / np.where(ok, R, 1.0) > clip))
        if (np.abs(e[ok] - 1.0) <= tol).all() and not clipped.any():
            break
        if k == max_rounds - 1:
            break
        wt = wt / e[group]
        comp *= e
        ctx.set_weights(wt)
    ctx.step()
    return rounds, comp


def main():
    import fba_import
    fba = fba_import.load()
    from fba_amd import synth
    config = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    folder = os.path.join(os.environ.get("FBA_BENCH_DIR", "/tmp/fba_bench"), f"c{config}")
    if not os.path.exists(os.path.join(folder, ".done")):
        synth.make_config(config, folder)
        open(os.path.join(folder, ".done"), "w").close()
    ds = fba.load_folder(folder)
    pk, st = ds.pack(), fba.capi.make_settings(ds.settings)
    n = 2 * pk.n_pts
    group = (np.arange(n) % 2).astype(np.int32)
    ev, wall, comp_wall, info = [], [], [], None
    for rep in range(reps + 1):  # (the first of each is the warm-up)
        ctx = fba.capi.Context(pk, st)
        ctx.set_timing(True)
        out = ctx.vce(group, 2)
        ev.append(ctx.timings()[7] / out["rounds"])
        ctx.close()
        ctx = fba.capi.Context(pk, st)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = ctx.vce(group, 2)
        wall.append((time.perf_counter() - t0) * 1e3)
        ctx.close()
        ctx = fba.capi.Context(pk, st)
        ctx.synchronize()
        t0 = time.perf_counter()
        rounds, comp = composed(ctx, group, 2, st.meas_std_x, st.meas_std_y)
        comp_wall.append((time.perf_counter() - t0) * 1e3)
        ctx.close()
        info = (out, rounds, comp)
        print(f"vce timing config {config} rep {rep}: own kernels {ev[-1]:.3f} ms/round, fba_vce wall {wall[-1]:.1f} ms, "
              f"composed wall {comp_wall[-1]:.1f} ms", flush=True)
    out, rounds, comp = info
    f = lambda a: f"{np.median(a[1:]):.3f} ms ({min(a[1:]):.3f} .. {max(a[1:]):.3f})"
    print(f"vce timing config {config}: n={n} groups xy rounds {out['rounds']} iterations {out['iterations']} converged "
          f"{out['converged']} component {out['component'][:2]} (composed: rounds {rounds} component {comp}); median of {reps}: "
          f"own kernels per round {f(ev)}, fba_vce wall {f(wall)}, composed from Python wall {f(comp_wall)}", flush=True)


if __name__ == "__main__":
    main()
