"""Dense numpy restatement of fba_snoop (include/fba.h) on oracle/fba_oracle.py's functions, and the scenes of the
data-snooping tests.

One round: Gauss-Newton from the current xhat with P = oracle.weights x wt (vce_ref._gn) -> Cx of the last normal
matrix -> per row qraw = a Cx a' of the unweighted Jacobian row -> per point W = max |v| sqrt(P) / sqrt(1 - P qraw) (0
where r < 1e-10) while active, W~ = max s0 |v| / sqrt(sigma^2 + s0^2 qraw) while excluded -> candidates, the
local-maximum rule, the back-check (select_round) -> wt = (1e-6 s0)^2 / s0^2 on the eliminated points, s0^2 on the
re-admitted.  Two routes as in vce_ref: the explicit bordered inverse, or an LU step and a symmetric solve for Cx;
their difference per round and quantity is the restatement's own spread.
"""
import os
from types import SimpleNamespace

import numpy as np

import vce_ref as vr

ACTIVE, EXCLUDED, READMITTED = 0, 1, 2
EPS = 1e-6
MEAS_STD = vr.MEAS_STD
CRIT = 3.29

# the scenes: vce_ref's geometry (scene A's and scene C's generator arguments), synth.generate's own noise at Meas_std,
# and blunders in units of Meas_std on chosen PHO rows (plant()).  Seeds: the first from 3 (A, P, N) / 8 (C) upwards
# whose restatement passes every condition of restated(): A 15, P 17, N 10, C 21.  Most of the earlier ones fail "exactly
# the planted set": 1440 rows of honest noise hold a |w| > 3.29 more often than not; DESIGN.md 6j lists them all.
SCENES = {
    "A": dict(gen=dict(n_img=12, n_tie=120, seed=15, obs_per_point=6), plant="six"),
    "C": dict(gen=dict(n_img=12, n_tie=120, seed=21, obs_per_point=6, n_cam=2, n_control=10), plant="control"),
    "P": dict(gen=dict(n_img=12, n_tie=120, seed=17, obs_per_point=6), plant="pre"),
    "N": dict(gen=dict(n_img=12, n_tie=120, seed=10, obs_per_point=6), plant="none"),
}
SIZES = (10.0, 20.0, 12.0, 18.0, 14.0, 16.0)  # blunders in sigma, alternately on x and on y


def plant(kind, img, pid, n_control=0):
    """-> (PHO rows of the blunders, PHO rows to pre-exclude) from the PHO-ordered image and point of every row.
    six: two on one tie point in different images, two in one image on different points, two isolated."""
    n = len(img)
    if kind == "none":
        return [], []
    if kind == "control":
        ctl = int(np.nonzero(pid < n_control)[0][3])
        tie = int(np.nonzero((pid >= n_control) & (img != img[ctl]))[0][40])
        return [ctl, tie], []
    rows = []
    t1 = pid[n // 3]
    rows += [int(r) for r in np.nonzero(pid == t1)[0][:2]]
    used_i, used_p = {int(img[r]) for r in rows}, {int(t1)}
    i1 = next(i for i in range(int(img.max()) + 1) if i not in used_i)
    in_i1 = [int(r) for r in np.nonzero(img == i1)[0] if int(pid[r]) not in used_p]
    rows += [in_i1[2], in_i1[len(in_i1) // 2]]
    used_i.add(i1)
    used_p |= {int(pid[r]) for r in rows}
    for r in range(n - 1, -1, -1):
        if int(img[r]) not in used_i and int(pid[r]) not in used_p:
            rows.append(r)
            used_i.add(int(img[r]))
            used_p.add(int(pid[r]))
        if len(rows) == 6:
            break
    if kind == "six":
        return rows, []
    pre = []
    for r in range(0, n, 97):  # three clean points, each with a tie point and an image of its own among the chosen
        if int(img[r]) not in used_i - {i1} and int(pid[r]) not in used_p and len(pre) < 3:
            pre.append(r)
            used_p.add(int(pid[r]))
    return rows[4:], pre


def scene_folder(synth, root, name, gen=None):
    """the scene's folder (written once) -> (folder, planted PHO rows, pre-excluded PHO rows)"""
    spec = SCENES[name]
    g = gen or spec["gen"]
    sc = dict(synth.generate(noise=MEAS_STD, **g))
    order = np.lexsort((sc["pid"], sc["img"]))  # synth.write_folder's PHO order
    rows, pre = plant(spec["plant"], sc["img"][order], sc["pid"][order], g.get("n_control", 0))
    folder = os.path.join(str(root), f"snoop_{name}_{g['seed']}_{g['n_tie']}")
    if not os.path.isdir(folder):
        xy = sc["xy"].copy()
        for k, r in enumerate(rows):
            xy[order[r], k % 2] += (1 if k % 3 else -1) * SIZES[k] * MEAS_STD
        sc["xy"] = xy
        synth.write_folder(sc, folder, nk=2)
    return folder, sorted(rows), sorted(pre)


def point_stat(state, P, qraw, v, s0sq, sigma):
    """(W / W~ per point, the redundancy number r of the row that gives it) from the rows' P (weights in force), qraw,
    v, starting weights s0^2 and sigmas"""
    r = 1.0 - P * qraw
    with np.errstate(invalid="ignore", divide="ignore"):
        wa = np.where(r < 1e-10, 0.0, np.abs(v) * np.sqrt(P) / np.sqrt(np.where(r < 1e-10, 1.0, r)))
        we = np.sqrt(s0sq) * np.abs(v) / np.sqrt(sigma ** 2 + s0sq * qraw)
    w = np.where(np.repeat(state == EXCLUDED, 2), we, wa).reshape(-1, 2)
    return w.max(axis=1), r.reshape(-1, 2)[np.arange(len(w)), w.argmax(axis=1)]


def select_round(W, state, tie, img, crit=CRIT, min_rays=2, min_img_points=6):
    """-> (pick, back) boolean per point: fba.h's steps 4 - 6, ties to the lower index"""
    n = len(W)
    act = state != EXCLUDED
    ct = np.bincount(tie[act & (tie >= 0)], minlength=max(int(tie.max(initial=-1)) + 1, 1))
    ci = np.bincount(img[act], minlength=max(int(img.max(initial=-1)) + 1, 1))
    cand = (state == ACTIVE) & (W > crit) & (ci[img] - 1 >= min_img_points) & ((tie < 0) | (ct[np.maximum(tie, 0)] - 1 >= min_rays))
    pick = np.zeros(n, bool)
    for i in np.nonzero(cand)[0]:
        rivals = cand & (((tie == tie[i]) & (tie[i] >= 0)) | (img == img[i]))
        rivals[i] = False
        j = np.nonzero(rivals)[0]
        pick[i] = not np.any((W[j] > W[i]) | ((W[j] == W[i]) & (j < i)))
    back = (state == EXCLUDED) & (W <= crit) if not pick.any() else np.zeros(n, bool)
    return pick, back


def restate(oracle, od, pre=(), max_rounds=20, crit=CRIT, min_rays=2, min_img_points=6, max_share=0.05, route=0, wt0=None):
    """-> namespace: rounds, W and r (per round; r of the row that gives W), before / state (before / after each round), picks / backs (per round, PHO rows), table,
    converged, bits, deltasum (all steps), iters (per round), xhat, v, wt (2 n_pts) final weights, sigma02"""
    P0 = oracle.weights(od)
    sigma = 1.0 / np.sqrt(P0)
    s0sq = np.ones(od.n) if wt0 is None else np.array(wt0, dtype=np.float64)
    npts = od.n // 2
    tie, img = np.asarray(od.tie_index, dtype=np.int64), np.asarray(od.ext_index, dtype=np.int64)
    state = np.zeros(npts, dtype=np.uint8)
    state[list(pre)] = EXCLUDED
    x = oracle.buildxhat(od)[0]
    Ws, states, picks, backs, table, dsum, iters, rs, before = [], [], [], [], [], [], [], [], []
    conv, bits = False, 0

    def wts():
        low = (EPS * np.sqrt(s0sq)) ** 2
        return np.where(np.repeat(state == EXCLUDED, 2), low, s0sq)

    for k in range(max_rounds):
        P = P0 * wts()
        g = vr._gn(oracle, od, x, P, route)
        x = g.xhat
        dsum += g.deltasum
        iters.append(len(g.deltasum))
        Cx = vr._cx(oracle, od, g.A, g.w, g.G, P, route)
        qraw = np.einsum("ij,ij->i", g.A @ Cx, g.A)
        W, rw = point_stat(state, P, qraw, g.v, s0sq, sigma)
        rs.append(rw)
        before.append(state.copy())
        pick, back = select_round(W, state, tie, img, crit, min_rays, min_img_points)
        n_ex = int((state == EXCLUDED).sum())
        last = k == max_rounds - 1
        stop = pick.any() and (n_ex + pick.sum()) > max_share * npts
        change = (pick.any() or back.any()) and not last and not stop
        Ws.append(W)
        picks.append(np.nonzero(pick)[0])
        backs.append(np.nonzero(back)[0])
        table.append([pick.sum(), back.sum(), n_ex + (pick.sum() - back.sum() if change else 0), W[state != EXCLUDED].max(initial=0.0)])
        if not pick.any() and not back.any():
            conv = True
        if stop:
            bits |= 2
        if change:
            state = state.copy()
            state[pick] = EXCLUDED
            state[back] = READMITTED
        states.append(state.copy())
        if not change:
            break
    P = P0 * wts()
    n, u = g.A.shape
    return SimpleNamespace(rounds=len(Ws), W=Ws, r=rs, before=before, state=states, picks=picks, backs=backs, table=np.array(table, dtype=np.float64),
                           converged=conv, bits=bits, deltasum=dsum, iters=iters, xhat=g.xhat, v=g.v, wt=wts(), P=P,
                           sigma02=float(g.v @ (P * g.v)) / (n - u), A=g.A, w=g.w, G=g.G,
                           names=oracle.buildxhat(od)[1], dist_scaling=g.dist_scaling)


_CACHE = {}


def restated(fba, oracle, root, name):
    """a scene's folder, datasets, planted rows and both routes of its restatement, computed once per session; asserts
    the conditions on the inputs, on the restatement alone: converged; exactly the planted points excluded and exactly
    the pre-excluded ones re-admitted; no W or W~ of any round within 2 % of crit; no deltasum within 1.25x of
    Threshold_Value"""
    if name not in _CACHE:
        from fba_amd import synth
        folder, rows, pre = scene_folder(synth, root, name)
        od, ds = oracle.load_folder(folder), fba.load_folder(folder)
        a, b = restate(oracle, od, pre), restate(oracle, od, pre, route=1)
        thr = od.settings["threshold"]
        near = [d for d in a.deltasum + b.deltasum if thr / 1.25 <= d <= thr * 1.25]
        assert not near, f"scene {name}: the restatement's deltasum {near} is within 1.25x of Threshold_Value: pick another seed"
        for r in (a, b):
            assert r.converged, f"scene {name}: the restatement does not converge"
            assert np.nonzero(r.state[-1] == EXCLUDED)[0].tolist() == rows, (name, np.nonzero(r.state[-1] == EXCLUDED)[0], rows)
            assert np.nonzero(r.state[-1] == READMITTED)[0].tolist() == pre, (name, np.nonzero(r.state[-1] == READMITTED)[0], pre)
            close = [float(w) for W in r.W for w in W if abs(w / CRIT - 1.0) <= 0.02]
            assert not close, f"scene {name}: statistics {close} within 2 % of crit: pick another seed"
        assert a.rounds == b.rounds and a.iters == b.iters
        assert all(p.tolist() == q.tolist() for p, q in zip(a.picks + a.backs, b.picks + b.backs))
        _CACHE[name] = SimpleNamespace(folder=folder, od=od, ds=ds, rows=rows, pre=pre, a=a, b=b)
    return _CACHE[name]
