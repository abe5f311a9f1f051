"""Scenes whose tie points have weakly intersecting rays, and the yardsticks they are judged by (shared by
tests/test_weak_points_host.py and tests/test_gpu_weak_points.py; test infrastructure, no GPU).

Every scene starts from synth.generate(8, 40, seed=3, obs_per_point=5, typ=typ, n_control=8) at nK = 2, where every
tie point's block V = Jp'PJp has cond < 1e3, and adds

    twin images   images 0 and 1 once more, B units along X, same angles: the TRUE pose and the START pose are both the
                  original's plus (B, 0, 0) -- independent start noise would make the base at the linearisation point
                  ~14 units whatever B is.  A twin observes every point its original observes (true model, 0.3 px
                  noise).
    weak points   per pair two tie points seen by the original and its twin only, X Y within +-800 of the image,
                  Z uniform in [0, 1500], start values the truth + N(0, 10): parallax ratio B / 2500, cond(V) of the
                  order (2500 / B)^2.

TIERS: B = 30, 3, 0.3, 0.03 (cond(V) of the weak points 2-4e4 .. 2-4e10), one scene each.  Variants:

    chunk      one camera (k_lin_reduce / k_lin_point), fisheye and pinhole, every tier
    rig        the twins use camera 1: a two-camera rig of base B; every point seen through both cameras is a general
               point (k_gen_point, k_gen_keys, k_gen_backsub).  Tiers 3 and 0.3: at 0.03 the fp64 yardstick itself is
               1.0e-4 off on a weak point's correction and 6.0e-5 per element of the tie points, and 20 x that
               breaks the 1e-3 cap (CAP below), so the rig's hard tier is one step milder than the chunk's
    dup        one image point of each weak point measured twice (fresh noise): the weak points alone are general
               points.  Tier 0.3
    free       no control points, inner constraints (the border path).  Tier 0.3
    excluded   tier 30, and six strong points seen by image 0 or 1 cut to three observations -- the original, its twin
               and the farthest other image; of the three, the observation farthest from the other two (that third
               image's) gets the user weight 1e-12 on both rows, the documented way to exclude a measurement
               (include/fba.h), so V's conditioning comes from the weights (the WH = true kernels)
"""
import numpy as np

BASE = dict(n_img=8, n_tie=40, seed=3, obs_per_point=5)
N_CONTROL = 8
NK = 2
TIERS = (30.0, 3.0, 0.3, 0.03)
DEPTH = 2500.0   # the nominal camera-to-point distance cond(V) is referred to
EXCLUDE = 1e-12
NOISE = 0.3

SCENES = {}
for _typ in ("fisheye", "pinhole"):
    for _b in TIERS:
        SCENES[f"chunk-{_typ}-B{_b:g}"] = dict(variant="chunk", typ=_typ, B=_b)
SCENES["rig-B3"] = dict(variant="rig", typ="fisheye", B=3.0)
SCENES["rig-B0.3"] = dict(variant="rig", typ="fisheye", B=0.3)
SCENES["dup-B0.3"] = dict(variant="dup", typ="fisheye", B=0.3)
SCENES["free-B0.3"] = dict(variant="free", typ="fisheye", B=0.3)
SCENES["excluded-B30"] = dict(variant="excluded", typ="fisheye", B=30.0)


def _observe(synth, sc, i, X, cam, rng):
    """image i's true pose (in sc) observing the points X through camera `cam`: the true model + noise"""
    M = synth._rot(*sc["ang_true"][i])
    UVW = (X - sc["C_true"][i]) @ M.T
    xp, yp, c = synth.camera_params(cam)
    x, y = synth._project(sc["typ"], UVW[:, 0], UVW[:, 1], UVW[:, 2], c, xp, yp, synth.K0, synth.P0)
    assert (UVW[:, 2] < 0).all() and (x > 1).all() and (x < 2047).all() and (y > 1).all() and (y < 2047).all()
    return np.stack([x, y], -1) + rng.normal(0, NOISE, (len(X), 2))


def build(synth, variant, typ, B, base=None, n_control=N_CONTROL, pairs=(0, 1), n_weak=2):
    """-> dict(scene (synth.write_folder's), weights (2 n_pts, PHO order, or None), weak / strong / cut: tie indices
    (TIE order) of the weak points, of the base scene's tie points left as they were, and of `excluded`'s cut points)"""
    base = dict(BASE if base is None else base)
    if variant == "free":
        n_control = 0
    sc = dict(synth.generate(base.pop("n_img"), base.pop("n_tie"), typ=typ, n_control=n_control, **base))
    rng = np.random.default_rng(1000 + int(round(1000 * B)))
    n_img, n_pts = len(sc["C0"]), len(sc["X0"])
    cam = list(sc["cam"])
    img, pid, xy = [sc["img"]], [sc["pid"]], [sc["xy"]]
    weak = []
    for i in pairs:
        tw = n_img + len(cam) - len(sc["cam"])
        for k in ("C_true", "C0"):
            sc[k] = np.concatenate([sc[k], sc[k][i][None] + np.array([[B, 0.0, 0.0]])])
        for k in ("ang_true", "ang0"):
            sc[k] = np.concatenate([sc[k], sc[k][i][None]])
        cam.append(1 if variant == "rig" else 0)
        seen = sc["pid"][sc["img"] == i]
        Xw = np.stack([sc["C_true"][i, 0] + rng.uniform(-800, 800, n_weak),
                       sc["C_true"][i, 1] + rng.uniform(-800, 800, n_weak), rng.uniform(0.0, 1500.0, n_weak)], 1)
        new = n_pts + len(weak) + np.arange(n_weak)
        weak.extend(new.tolist())
        sc["X_true"] = np.concatenate([sc["X_true"], Xw])
        sc["X0"] = np.concatenate([sc["X0"], Xw + rng.normal(0, 10.0, Xw.shape)])
        pts = np.concatenate([seen, new])
        Xall = sc["X_true"][pts]
        img += [np.full(n_weak, i), np.full(len(pts), tw)]
        pid += [new, pts]
        xy += [_observe(synth, sc, i, Xw, cam[i], rng), _observe(synth, sc, tw, Xall, cam[tw], rng)]
        if variant == "dup":
            img.append(np.full(n_weak, i))
            pid.append(new)
            xy.append(_observe(synth, sc, i, Xw, cam[i], rng))
    sc["cam"] = np.array(cam, dtype=np.int64)
    sc["control"] = np.concatenate([sc["control"], np.zeros(len(weak), bool)])
    sc["img"], sc["pid"] = np.concatenate(img).astype(np.int64), np.concatenate(pid).astype(np.int64)
    sc["xy"] = np.concatenate(xy)
    tie_of = np.cumsum(~sc["control"]) - 1   # point -> TIE index (write_folder lists the non-control points in order)
    strong = [j for j in range(n_pts) if not sc["control"][j]]
    cut, weights = [], None
    if variant == "excluded":
        keep = np.ones(len(sc["img"]), bool)
        excl = np.zeros(len(sc["img"]), bool)
        for k, i in enumerate(pairs):
            tw = n_img + k
            got = 0
            for j in strong:
                obs = np.nonzero(sc["pid"] == j)[0]
                if j in cut or i not in sc["img"][obs] or got == 3:
                    continue
                others = [o for o in obs if sc["img"][o] not in (i, tw) and sc["img"][o] < n_img]
                if not others:
                    continue
                far = max(others, key=lambda o: np.linalg.norm(sc["C_true"][sc["img"][o]] - sc["C_true"][i]))
                three = [o for o in obs if sc["img"][o] in (i, tw)] + [far]
                assert len(three) == 3
                keep[obs] = False
                keep[three] = True
                # of the three, the observation farthest from the other two
                c3 = sc["C_true"][sc["img"][three]]
                dist = [sum(np.linalg.norm(c3[a] - c3[b]) for b in range(3) if b != a) for a in range(3)]
                assert three[int(np.argmax(dist))] == far
                excl[far] = True
                cut.append(j)
                got += 1
        assert len(cut) == 6, "six strong points seen by image 0 or 1"
        sc["img"], sc["pid"], sc["xy"], excl = sc["img"][keep], sc["pid"][keep], sc["xy"][keep], excl[keep]
        order = np.lexsort((sc["pid"], sc["img"]))   # write_folder's PHO order
        weights = np.repeat(np.where(excl[order], EXCLUDE, 1.0), 2)
        strong = [j for j in strong if j not in cut]
    return dict(scene=sc, weights=weights, weak=tie_of[weak].tolist(), strong=tie_of[strong].tolist(),
                cut=tie_of[cut].tolist() if cut else [], B=B, variant=variant, typ=typ)


def build_named(synth, name):
    return build(synth, **SCENES[name])


def write(synth, built, folder):
    return synth.write_folder(built["scene"], folder, nk=NK)


# ---- the linearisation and the fp64 yardsticks ------------------------------------------------------------------
def uc_of(oracle, od):
    u_img, u_cam = oracle.counts(od.settings)
    return u_img * od.numImg + u_cam * od.numCam


def point_conds(A, P, uc):
    """cond(V) of every tie point's V = Jp'PJp"""
    nt = (A.shape[1] - uc) // 3
    out = np.zeros(nt)
    for t in range(nt):
        Ap = A[:, uc + 3 * t:uc + 3 * t + 3]
        out[t] = np.linalg.cond(Ap.T @ (P[:, None] * Ap))
    return out


def block_fp64(A, w, P, uc, G=None, lam=0.0):
    """exact_solve.solve restated in plain NumPy fp64 (LAPACK's 3 x 3 inverses and solves of the reduced system): the
    yardstick for the cofactor blocks V^-1 + T C T', for a Cx a' and for the damped pass"""
    n, u = A.shape
    nt = (u - uc) // 3
    Ac = A[:, :uc]
    S = Ac.T @ (P[:, None] * Ac)
    r = Ac.T @ (P * w)
    pts = []
    for t in range(nt):
        rows = np.nonzero(np.any(A[:, uc + 3 * t:uc + 3 * t + 3] != 0, axis=1))[0]
        Ap = A[rows, uc + 3 * t:uc + 3 * t + 3]
        PAp = P[rows, None] * Ap
        V = Ap.T @ PAp
        V = V + lam * np.diag(np.diag(V))
        W = Ac[rows].T @ PAp
        b = Ap.T @ (P[rows] * w[rows])
        Vi = np.linalg.inv(V)
        T = Vi @ W.T
        S -= W @ T
        r -= W @ (Vi @ b)
        pts.append((rows, Ap, Vi, T, W, b))
    S = S + lam * np.diag(np.diag(S))
    d = 0 if G is None else G.shape[1]
    K = np.zeros((uc + d, uc + d))
    K[:uc, :uc] = S
    if d:
        K[:uc, uc:] = G[:uc]
        K[uc:, :uc] = G[:uc].T
    dc = np.linalg.solve(K, np.concatenate([-r, np.zeros(d)]))[:uc]
    C = np.linalg.solve(K, np.eye(uc + d))[:uc, :uc]
    delta = np.zeros(u)
    delta[:uc] = dc
    cx_tie = np.zeros((nt, 3, 3))
    aCa = np.einsum("ij,jk,ik->i", Ac, C, Ac)
    for t, (rows, Ap, Vi, T, W, b) in enumerate(pts):
        delta[uc + 3 * t:uc + 3 * t + 3] = -Vi @ (b + W.T @ dc)
        TC = T @ C
        cx_tie[t] = Vi + TC @ T.T
        aCa[rows] += -2 * np.einsum("ik,kj,ij->i", Ap, TC, Ac[rows]) + np.einsum("ik,km,im->i", Ap, cx_tie[t], Ap)
    return dict(delta=delta, cx_tie=cx_tie, cx_cam_diag=np.diag(C).copy(), aCa=aCa)


def linearise(oracle, od, x, weights=None):
    """the oracle's A, w, G, dist_scaling at x and P with the user weights in"""
    A, w, G, dsc = oracle.build_awg(od, x)
    P = oracle.weights(od) * (1.0 if weights is None else weights)
    return dict(A=A, w=w, G=G, dsc=dsc, P=P, x=np.array(x, dtype=np.float64))


def exact_pass(oracle, od, lin, lam=0.0):
    """the exact solve of one linearisation and the fp64 yardsticks beside it:
    exact  exact_solve.solve (50 digits), x1 = x + descale(delta)
    schur  oracle.solve_schur's delta (undamped) or block_fp64's (damped): the yardstick of the pass
    block  block_fp64: the yardstick of the cofactor blocks, the camera-side diagonal and a Cx a'"""
    import exact_solve
    uc = uc_of(oracle, od)
    A, w, G, P = lin["A"], lin["w"], lin["G"], lin["P"]
    ex = exact_solve.solve(A, w, P, uc, G, lam)
    blk = block_fp64(A, w, P, uc, G, lam)
    d_y = blk["delta"] if lam else oracle.solve_schur(od, A, w, G, P)
    x = lin["x"]
    return dict(uc=uc, exact=ex, block=blk, x1=x + oracle.descale(od, ex["delta"], lin["dsc"]),
                x1_y=x + oracle.descale(od, d_y, lin["dsc"]))


def load(synth, oracle, root, cache, name):
    """the named scene written under root and read by the oracle, its start values and their linearisation (cached)"""
    import os
    if name not in cache:
        b = build_named(synth, name)
        folder = write(synth, b, os.path.join(str(root), name))
        od = oracle.load_folder(folder)
        x0, names = oracle.buildxhat(od)
        cache[name] = dict(b=b, folder=folder, od=od, x0=x0, names=names, lin=linearise(oracle, od, x0, b["weights"]))
    return cache[name]


# ---- the metrics ------------------------------------------------------------------------------------------------
def pass_errors(x1, x1_ref, x0, names, dsc, uc, weak, strong):
    """(a) cam_group / cam_elem and (b) tie_group / tie_elem: conftest's xhat metrics over the camera-side groups and
    over the tie points; (c) weak_delta and (d) strong_delta: per point |d - d_ref|_2 / |d_ref|_2 of d = x1 - x0, the
    worst point"""
    from conftest import SMALL_SCENE_FLOOR, elem_rel_err, group_rel_err
    g = group_rel_err(x1, x1_ref, names, dsc)
    e = elem_rel_err(x1, x1_ref, names, dsc, floor=SMALL_SCENE_FLOOR)
    out = dict(cam_group=max(v for k, v in g.items() if k != "XYZ"),
               cam_elem=max(v for k, v in e.items() if k != "XYZ"), tie_group=g["XYZ"], tie_elem=e["XYZ"])
    d, dr = (x1 - x0)[uc:].reshape(-1, 3), (x1_ref - x0)[uc:].reshape(-1, 3)
    rel = np.linalg.norm(d - dr, axis=1) / np.linalg.norm(dr, axis=1)
    out["weak_delta"] = float(rel[weak].max())
    out["strong_delta"] = float(rel[strong].max()) if len(strong) else 0.0
    return out


def delta_cancellation(x0, x1_ref, uc):
    """what forming d = x1 - x0 in fp64 costs, relative to |d|, the worst tie point: eps |x0| / |d|"""
    x, d = x0[uc:].reshape(-1, 3), (x1_ref - x0)[uc:].reshape(-1, 3)
    return float((np.finfo(np.float64).eps * np.linalg.norm(x, axis=1) / np.linalg.norm(d, axis=1)).max())


def block_errors(blocks, ref, weak, strong):
    """(e): per point max |dC_ij| / max |C_ij| of its 3 x 3 block, the worst weak and the worst strong point"""
    e = np.abs(blocks - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    return dict(weak_block=float(e[weak].max()), strong_block=float(e[strong].max()) if len(strong) else 0.0)


def axes_errors(eig3, blocks, ref, weak, strong):
    """the ellipsoids' semi-axes through the device's own eigen routine run on the host (capi.eig3_host): per point
    max |a_i^2 - ref a_i^2| / ref a_max^2, the worst weak and the worst strong point"""
    a, r = eig3(pack6(blocks))[:, :3], eig3(pack6(ref))[:, :3]
    e = np.abs(a ** 2 - r ** 2).max(axis=1) / r[:, 0] ** 2
    return dict(weak_axes=float(e[weak].max()), strong_axes=float(e[strong].max()) if len(strong) else 0.0)


def yardsticks(s, lin, ep, eig3):
    """every metric of the GPU tests, of the fp64 yardsticks against the exact solve"""
    b = s["b"]
    weak = b["weak"] + b["cut"]
    y = pass_errors(ep["x1_y"], ep["x1"], lin["x"], s["names"], lin["dsc"], ep["uc"], weak, b["strong"])
    ex, blk = ep["exact"], ep["block"]
    y.update(block_errors(blk["cx_tie"], ex["cx_tie"], weak, b["strong"]))
    y.update(axes_errors(eig3, blk["cx_tie"], ex["cx_tie"], weak, b["strong"]))
    y["cam_diag"] = float(np.abs(blk["cx_cam_diag"] / ex["cx_cam_diag"] - 1).max())
    y["redundancy"] = float(np.abs(lin["P"] * (blk["aCa"] - ex["aCa"])).max())
    return y


def pack6(blocks):
    return np.asarray(blocks).reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]


def bar(yardstick, floor=1e-9, extra=0.0):
    """the suite's bar: max(floor, 20 x the yardstick's own error in the same metric) (+ a stated extra term)"""
    return max(floor, 20.0 * yardstick) + extra


LAMBDA = 1e-3   # the damped pass' fba_set_damping value
PASS_METRICS = ("cam_group", "cam_elem", "tie_group", "tie_elem", "weak_delta", "strong_delta")
CAP = 1e-3   # 20 x the yardstick must stay below this on every scene the GPU tests use, in every metric
