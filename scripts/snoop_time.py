"""Time fba_snoop on a benchmark scene with planted blunders against the same loop composed from Python on the same
build (fba_adjust, fba_residuals, fba_reliability, numpy selection, fba_set_weights), the lines of
profiles/snoop_timing_config4.log:  python scripts/snoop_time.py [config] [repetitions]

The scene: the benchmark configuration's measurements plus blunders of 15 sigma on 0.1 % of the image points, chosen and
signed by numpy.random.default_rng(11), alternately on x and y.

Per repetition, on fresh contexts: (a) fba_snoop with fba_set_timing on -- fba_last_timings[7], the HIP-event time of
the call's own kernels (the reliability part and the selection of every round), divided by the rounds; (b) fba_snoop
with timing off: the wall time of the whole call; (c) the composed loop: the wall time from the first fba_adjust to the
last.  The composed loop eliminates on W alone: an excluded row's W~ needs q, which only the device has, so it has no
back-check.  Medians over the repetitions (default 7), after one warm-up of each."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def select(W, excluded, tie, img, n_tie, n_img, crit=3.29, min_rays=2, min_img_points=6):
    """one round's picks in numpy: include/fba.h's steps 4 and 5"""
    n = W.size
    act = ~excluded
    ct = np.bincount(tie[act & (tie >= 0)], minlength=max(n_tie, 1))
    ci = np.bincount(img[act], minlength=max(n_img, 1))
    cand = act & (W > crit) & (ci[img] - 1 >= min_img_points) & ((tie < 0) | (ct[np.maximum(tie, 0)] - 1 >= min_rays))
    idx = np.nonzero(cand)[0]
    o = idx[np.lexsort((idx, -W[idx]))]  # the best first: the larger W, the lower row
    wt, wi = np.full(max(n_tie, 1), -1), np.full(max(n_img, 1), -1)
    ot = o[tie[o] >= 0]
    u, first = np.unique(tie[ot], return_index=True)
    wt[u] = ot[first]
    u, first = np.unique(img[o], return_index=True)
    wi[u] = o[first]
    rows = np.arange(n)
    return cand & (wi[img] == rows) & ((tie < 0) | (wt[np.maximum(tie, 0)] == rows))


def composed(ctx, tie, img, n_tie, n_img, max_rounds=20):
    """fba_snoop's elimination rounds from Python: every round copies v, r and w (2 n_pts each) to the host and
    uploads the weights"""
    n = tie.size
    excluded = np.zeros(n, dtype=bool)
    rounds = 0
    for k in range(max_rounds):
        ctx.adjust()
        _, _, st = ctx.residuals()
        _, _, _, wst = ctx.reliability(st[3], corr=False)
        W = np.abs(wst).reshape(-1, 2).max(axis=1)
        rounds = k + 1
        pick = select(W, excluded, tie, img, n_tie, n_img)
        if not pick.any() or k == max_rounds - 1:
            break
        excluded |= pick
        ctx.set_weights(np.where(np.repeat(excluded, 2), 1e-12, 1.0))
    return rounds, excluded


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
    n = pk.n_pts
    rng = np.random.default_rng(11)
    rows = np.sort(rng.choice(n, size=max(int(round(0.001 * n)), 1), replace=False))
    sign = rng.choice([-1.0, 1.0], size=rows.size)
    axis = np.arange(rows.size) % 2
    pk.xy[2 * rows + axis] += sign * 15.0 * np.where(axis == 0, st.meas_std_x, st.meas_std_y)
    tie, img = np.asarray(pk.tie, dtype=np.int64), np.asarray(pk.img, dtype=np.int64)
    ev, wall, comp_wall, info = [], [], [], None
    for rep in range(reps + 1):  # (the first of each is the warm-up)
        ctx = fba.capi.Context(pk, st)
        ctx.set_timing(True)
        out = ctx.snoop()
        ev.append(ctx.timings()[7] / out["rounds"])
        ctx.close()
        ctx = fba.capi.Context(pk, st)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = ctx.snoop()
        wall.append((time.perf_counter() - t0) * 1e3)
        ctx.close()
        ctx = fba.capi.Context(pk, st)
        ctx.synchronize()
        t0 = time.perf_counter()
        rounds, excluded = composed(ctx, tie, img, pk.n_tie, pk.n_img)
        comp_wall.append((time.perf_counter() - t0) * 1e3)
        ctx.close()
        info = (out, rounds, excluded)
        print(f"snoop timing config {config} rep {rep}: own kernels {ev[-1]:.3f} ms/round, fba_snoop wall {wall[-1]:.1f} ms, "
              f"composed wall {comp_wall[-1]:.1f} ms", flush=True)
    out, rounds, excluded = info
    ex = out["excluded"] == 1
    f = lambda a: f"{np.median(a[1:]):.3f} ms ({min(a[1:]):.3f} .. {max(a[1:]):.3f})"
    print(f"snoop timing config {config}: n_pts={n} planted {rows.size} rounds {out['rounds']} iterations {out['iterations']} "
          f"converged {out['converged']} excluded {int(ex.sum())} (of the planted: {int(ex[rows].sum())}) re-admitted "
          f"{int((out['excluded'] == 2).sum())} table {out['table'].tolist()} (composed: rounds {rounds} excluded "
          f"{int(excluded.sum())}, the same set: {bool((excluded == ex).all())}); median of {reps}: own kernels per round "
          f"{f(ev)}, fba_snoop wall {f(wall)}, composed from Python wall {f(comp_wall)}", flush=True)


if __name__ == "__main__":
    main()
