"""Dense numpy restatement of fba_vce (include/fba.h) on oracle/fba_oracle.py's functions, and the scenes of the
variance-component tests.

One round: Gauss-Newton from the current xhat with P = oracle.weights x wt (main.m:407-494's loop, at least one step)
-> Cx of the last normal matrix -> r = 1 - P rowsum((A Cx) o A), t = P v^2 -> per group R = sum r, T = sum t,
sigma2 = T / R with the statuses and the clamp of csrc/fba_vce.h -> wt /= sigma2 on the group's rows.  After the last
round one more step.  Two routes: the explicit bordered inverse (oracle.solve_dense) for the step and for Cx, or an LU
solve for the step and a symmetric solve against the identity for Cx (test_gpu_reliability._own_spread_r's pair); their
difference per round and quantity is the restatement's own spread.
"""
import os
from types import SimpleNamespace

import numpy as np

OK, EMPTY, WEAK, CLIPPED = 0, 1, 2, 3
MEAS_STD = 0.3  # synth.write_folder's Meas_std, both axes

# the scenes: synth.generate's arguments, the planted sigma per group, and the grouping.  B and C were first tried with
# the seeds 61 and 3: their restatements pass a deltasum of 1.03e-6 / 1.01e-6, within 1.25x of Threshold_Value (1e-6),
# which the threshold guard of the tests forbids, so the next seeds that pass it were taken: 63 (B; 62 fails the guard
# too) and 8 (C; 4 .. 7 fail it).  C under seed 8 does not reach tol within 10 rounds: it also covers that exit.
SCENES = {
    "A": dict(gen=dict(n_img=12, n_tie=120, seed=3, obs_per_point=6), groups="xy", planted=[0.2, 0.6]),
    "B": dict(gen=dict(n_img=14, n_tie=150, seed=63, obs_per_point=6, n_cam=2), groups="camera", planted=[0.2, 0.5]),
    "C": dict(gen=dict(n_img=12, n_tie=120, seed=8, obs_per_point=6, n_cam=2, n_control=10), groups="camera_xy",
              planted=[0.15, 0.45, 0.3, 0.6]),
    "D": dict(gen=dict(n_img=12, n_tie=120, seed=3, obs_per_point=6), groups="first6", planted=[0.3, 0.3]),
}


def scene_folder(synth, root, name, gen=None):
    """the scene's folder (written once): synth.generate(noise=0) at nk 2, fish-eye, plus N(0, planted sigma) from
    default_rng(7) on every measurement, in the scene's own observation order"""
    folder = os.path.join(str(root), f"vce_{name}")
    if not os.path.isdir(folder):
        spec = SCENES[name]
        sc = dict(synth.generate(noise=0.0, **(gen or spec["gen"])))
        n = len(sc["img"])
        planted = np.asarray(spec["planted"], dtype=np.float64)
        cam = np.asarray(sc["cam"])[sc["img"]]
        if spec["groups"] in ("xy", "first6"):
            sig = np.tile(planted[:2], (n, 1))
        elif spec["groups"] == "camera":
            sig = np.repeat(planted[cam][:, None], 2, axis=1)
        else:
            sig = np.stack([planted[2 * cam], planted[2 * cam + 1]], 1)
        sc["xy"] = sc["xy"] + np.random.default_rng(7).normal(0, 1, (n, 2)) * sig
        synth.write_folder(sc, folder, nk=2)
    return folder


def groups_of(name, cam):
    """(group (2 n_pts) in PHO order, n_groups) of a scene from its PHO rows' cameras"""
    n = len(cam)
    g = np.zeros((n, 2), dtype=np.int32)
    kind = SCENES[name]["groups"]
    if kind == "xy":
        g[:, 1] = 1
    elif kind == "camera":
        g[:] = np.asarray(cam)[:, None]
    elif kind == "camera_xy":
        g[:, 0], g[:, 1] = 2 * np.asarray(cam), 2 * np.asarray(cam) + 1
    else:  # rows 0..5 alone in group 1
        g = g.reshape(-1)
        g[:6] = 1
    return g.reshape(-1), len(SCENES[name]["planted"])


def group_estimate(R, T, n, min_redundancy=1.0, clip=100.0):
    """csrc/fba_vce.h's vce_group in numpy scalars: (sigma2, factor, status)"""
    if n == 0:
        return 1.0, 1.0, EMPTY
    if R < min_redundancy:
        return 1.0, 1.0, WEAK
    e, st = T / R, OK
    if e < 1.0 / clip:
        e, st = 1.0 / clip, CLIPPED
    elif e > clip:
        e, st = clip, CLIPPED
    return e, 1.0 / np.sqrt(e), st


def group_sums(group, r, t, n_groups):
    """[n_groups + 1][3]: R, T, n per group, the last row the ids -1 (np.add.at: index order)"""
    s = np.zeros((n_groups + 1, 3))
    slot = np.where(np.asarray(group) < 0, n_groups, group)
    np.add.at(s[:, 0], slot, r)
    np.add.at(s[:, 1], slot, t)
    np.add.at(s[:, 2], slot, 1.0)
    return s


def _solve_lu(od, A, w, G, P):
    N = A.T @ (P[:, None] * A)
    u_vec = A.T @ (P * w)
    if od.settings["Inner_Constraints"]:
        d = G.shape[1]
        N = np.block([[N, G], [G.T, np.zeros((d, d))]])
        u_vec = np.concatenate([u_vec, np.zeros(d)])
    return -np.linalg.solve(N, u_vec)[: A.shape[1]]


def _cx(oracle, od, A, w, G, P, route):
    if route == 0:
        return oracle.solve_dense(od, A, w, G, P)[1]
    import scipy.linalg as sla
    N = A.T @ (P[:, None] * A)
    u = len(N)
    if od.settings["Inner_Constraints"]:
        d = G.shape[1]
        N = np.block([[N, G], [G.T, np.zeros((d, d))]])
    return sla.solve(N, np.eye(len(N)), assume_a="sym")[:u, :u]


def _gn(oracle, od, x, P, route, one_step=False):
    """main.m:407-494 from x with the weights P: at least one step, until deltasum <= Threshold_Value or the cap"""
    s = od.settings
    dsum, deltasum = [], 100.0
    while deltasum > s["threshold"]:
        A, w, G, dsc = oracle.build_awg(od, x)
        delta = oracle.solve_dense(od, A, w, G, P)[0] if route == 0 else _solve_lu(od, A, w, G, P)
        delta = oracle.descale(od, delta, dsc)
        x = x + delta
        deltasum = float(np.sum(np.abs(delta)))
        dsum.append(deltasum)
        if one_step or len(dsum) >= s["Iteration_Cap"]:
            break
    return SimpleNamespace(xhat=x, A=A, w=w, G=G, delta=delta, v=A @ delta + w, deltasum=dsum, dist_scaling=dsc)


def restate(oracle, od, group, n_groups, max_rounds=10, tol=1e-3, min_redundancy=1.0, clip=100.0, route=0, wt0=None):
    """-> namespace: rounds, table (rounds, n_groups + 1, 4), component (n_groups), status (n_groups + 1), converged,
    wt (2 n_pts) the final weight multipliers, r / t of every round, deltasum (all steps), xhat, v, sigma02 and the
    last step's A, w, G"""
    group = np.asarray(group)
    P0 = oracle.weights(od)
    wt = np.ones(od.n) if wt0 is None else np.array(wt0, dtype=np.float64)
    comp = np.ones(n_groups)
    x = oracle.buildxhat(od)[0]
    table, rs, ts, dsum = [], [], [], []
    conv, status = False, None
    for k in range(max_rounds):
        P = P0 * wt
        g = _gn(oracle, od, x, P, route)
        x = g.xhat
        dsum += g.deltasum
        Cx = _cx(oracle, od, g.A, g.w, g.G, P, route)
        r = 1.0 - P * np.einsum("ij,ij->i", g.A @ Cx, g.A)
        t = P * g.v ** 2
        s = group_sums(group, r, t, n_groups)
        est = [group_estimate(*s[i], min_redundancy, clip) for i in range(n_groups)]
        rest = s[n_groups]
        est.append(((rest[1] / rest[0]) if (rest[2] > 0 and rest[0] > 0) else 1.0, 1.0, EMPTY if rest[2] == 0 else OK))
        table.append(np.column_stack([s, [e[0] for e in est]]))
        status = np.array([e[2] for e in est], dtype=np.int32)
        rs.append(r)
        ts.append(t)
        conv = all(abs(e[0] - 1.0) <= tol for e in est[:n_groups] if e[2] == OK) and not any(e[2] == CLIPPED for e in est[:n_groups])
        if conv or k == max_rounds - 1:
            break
        for i in range(n_groups):
            wt[group == i] /= est[i][0]
            comp[i] *= est[i][0]
    P = P0 * wt
    g = _gn(oracle, od, x, P, route, one_step=True)
    dsum += g.deltasum
    n, u = g.A.shape
    return SimpleNamespace(rounds=len(table), table=np.array(table), component=comp, status=status, converged=conv, wt=wt,
                           r=rs, t=ts, deltasum=dsum, xhat=g.xhat, v=g.v, sigma02=float(g.v @ (P * g.v)) / (n - u),
                           A=g.A, w=g.w, G=g.G, P=P, names=oracle.buildxhat(od)[1], dist_scaling=g.dist_scaling)


_CACHE = {}


def restated(fba, oracle, root, name):
    """a scene's folder, datasets, grouping and both routes of its restatement, computed once per session; asserts
    the two conditions on the inputs: every planted sigma recovered within 15 % by the restatement alone, and no
    deltasum of either route within 1.25x of Threshold_Value"""
    if name not in _CACHE:
        from fba_amd import synth
        folder = scene_folder(synth, root, name)
        od, ds = oracle.load_folder(folder), fba.load_folder(folder)
        grp, ng = groups_of(name, ds.pack().cam)
        a, b = restate(oracle, od, grp, ng), restate(oracle, od, grp, ng, route=1)
        thr = od.settings["threshold"]
        near = [d for d in a.deltasum + b.deltasum if thr / 1.25 <= d <= thr * 1.25]
        assert not near, f"scene {name}: the restatement's deltasum {near} is within 1.25x of Threshold_Value: pick another seed"
        rec = np.sqrt(a.component) * MEAS_STD / np.asarray(SCENES[name]["planted"])
        assert np.all(np.abs(rec - 1.0) <= 0.15), f"scene {name}: planted sigmas recovered to {rec}"
        assert a.rounds == b.rounds and len(a.deltasum) == len(b.deltasum)
        _CACHE[name] = SimpleNamespace(folder=folder, od=od, ds=ds, group=grp, n_groups=ng, a=a, b=b)
    return _CACHE[name]
