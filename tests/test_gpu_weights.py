"""Per-observation weights and the robust loss on the GPU (fba_set_weights / fba_set_loss / fba_get_weights)
against the dense oracle with the weighted P.

The oracle is composed here from oracle/fba_oracle.py's functions: a weighted step is oracle.solve_dense(od, A, w,
G, oracle.weights(od) * wt) on oracle.build_awg's A, w, G; a weighted adjustment oracle.adjust with that solver;
an IRLS step the same with wt recomputed from the step's own misclosure w (_loss_factor, include/fba.h's formulas).
sigma0^2, r and w are recomputed with P * wt the way test_gpu_reliability._oracle_rel does (through _Weighted, which
hands that module's functions the weighted P).

Bars: none of its own.  xhat per group and per element: max(1e-9, 20 x the oracle's own spread), the weighted
oracle's explicit inverse against the LU solve of the same weighted system; sigma0^2 at vtol = max(1e-9, 20 x that
pair's spread on sigma0^2), RMS at vtol, v and RSD at 10 vtol of their largest entry (all
test_gpu_block_shapes._every_pass's).  diag(Cx): test_gpu_parity._check_cov's 1e-8 relative, or where it is larger
20 x the weighted oracle's own spread on diag(Cx), the rule of the xhat and r bars: the larger of
flag_masks.cov_self_spread (its explicit inverse against the symmetric solve of the same bordered matrix) and
the LU variant's diag(Cx), taken at the LU run's own solution and sigma0^2, against the explicit-inverse run's.
Weights spread over six decades put the bordered matrix at a condition number of 1e14-1e15, where the oracle's
two routes differ by 1.7e-8 (pinhole) and its two runs by 6.9e-7 (fish-eye, whose xhat the two runs already
place 1.6e-5 apart in k2).  r and w:
test_gpu_reliability._reference / _check with the weighted P.  Effective weights under a loss: a loss factor is a
function f(t) of the point's standardised misclosure with |f'| <= 1 / k for both losses (Huber: k / t^2 <= 1 / k on
t >= k; Cauchy: 2 t k^2 / (k^2 + t^2)^2 <= 0.65 / k), and t = |misclosure| / sigma carries the v bar, so
|df| <= 10 vtol max|misclosure| / (min(sigma) k).  The measured errors of one run, with the oracle's own spreads
beside them: profiles/weights_gpu_errors.log (the "weights ..." prints of this module).
"""
import dataclasses
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import CAM0

pytestmark = pytest.mark.gpu

HUBER_K, CAUCHY_K = 1.345, 2.385
BLUNDER_ROW, BLUNDER_PX = 100, 6.0  # test_gpu_reliability's planted blunder: +6 px on the x of PHO row 100


# ---- the weighted oracle ----------------------------------------------------------------------------------------
def random_weights(n, seed):
    """log-uniform in [1e-3, 1e3], x and y drawn independently"""
    return 10.0 ** np.random.default_rng(seed).uniform(-3.0, 3.0, n)


def loss_factor(loss, k, P, w):
    """include/fba.h: per image point t^2 = p_x w0^2 + p_y w1^2 (P with the user weights in); Huber 1 | k / t,
    Cauchy 1 / (1 + t^2 / k^2); the same factor on both rows"""
    t2 = P[0::2] * w[0::2] ** 2 + P[1::2] * w[1::2] ** 2
    if loss == "huber":
        t = np.sqrt(t2)
        f = np.where(t <= k, 1.0, k / np.maximum(t, 1e-300))
    else:
        f = 1.0 / (1.0 + t2 / k ** 2)
    return np.repeat(f, 2)


def _Weighted(oracle, Pw):
    """the oracle as test_gpu_reliability's helpers use it, with the weighted P for oracle.weights"""
    return SimpleNamespace(weights=lambda od: Pw, solve_dense=oracle.solve_dense, adjust=oracle.adjust)


def _solvers(oracle, wt):
    from test_gpu_block_shapes import _solve_lu
    return (lambda d, A, w, G, P: oracle.solve_dense(d, A, w, G, P * wt)[0],
            lambda d, A, w, G, P: _solve_lu(d, A, w, G, P * wt))


def _finish(oracle, od, ro, lu, Pw, rel=True):
    """sigma0^2 with the weighted P on both variants, the bars of the module docstring, r / w's reference"""
    from test_gpu_block_shapes import _errors
    from test_gpu_reliability import _reference
    n, u = ro.A.shape
    ro = dataclasses.replace(ro, sigma02=float(ro.v @ (Pw * ro.v)) / (n - u))
    lu = dataclasses.replace(lu, sigma02=float(lu.v @ (Pw * lu.v)) / (n - u))
    s_s02 = abs(lu.sigma02 - ro.sigma02) / ro.sigma02
    out = dict(od=od, ro=ro, lu=lu, Pw=Pw, spread=_errors(lu.xhat, ro.xhat, ro), s_s02=s_s02, vtol=max(1e-9, 20 * s_s02))
    if rel:
        out["rel"] = _reference(_Weighted(oracle, Pw), od, ro, lu)
    return out


def weighted_oracle(oracle, od, wt):
    inv, lu = _solvers(oracle, wt)
    ro, rl = oracle.adjust(od, solver=inv), oracle.adjust(od, solver=lu)
    assert rl.iterations == ro.iterations
    thr = od.settings["threshold"]
    near = [d for d in ro.deltasum if thr / 1.25 <= d <= thr * 1.25]
    assert not near, f"the weighted oracle's deltasum {near} is within 1.25x of Threshold_Value: pick another seed"
    return _finish(oracle, od, ro, rl, oracle.weights(od) * wt)


def oracle_steps(oracle, od, xhat, n_steps, wt=None, loss=None, k=None, lu=False):
    """n_steps Gauss-Newton steps from xhat with P * wt (* the loss factor of each step's own misclosure);
    -> a Result-like namespace of the last step (A, w, G, delta, v, xhat, the last P) for _finish"""
    from test_gpu_block_shapes import _solve_lu
    P0 = oracle.weights(od) * (1.0 if wt is None else wt)
    x = np.array(xhat, dtype=np.float64)
    for _ in range(n_steps):
        A, w, G, dsc = oracle.build_awg(od, x)
        P = P0 * loss_factor(loss, k, P0, w) if loss else P0
        delta = _solve_lu(od, A, w, G, P) if lu else oracle.solve_dense(od, A, w, G, P)[0]
        delta = oracle.descale(od, delta, dsc)
        x = x + delta
    v = A @ delta + w
    names = oracle.buildxhat(od)[1]
    return SimpleNamespace(xhat=x, names=names, A=A, w=w, G=G, dist_scaling=dsc, delta=delta, v=v,
                           rsd=oracle.build_rsd(od, v, x), P=P, eff=P / oracle.weights(od),
                           rms=(float(np.sqrt(np.mean(v[0::2] ** 2))), float(np.sqrt(np.mean(v[1::2] ** 2)))))


def _steps_ref(oracle, od, xhat, n_steps, **kw):
    """oracle_steps with the explicit inverse and with LU, finished like weighted_oracle (no r / w reference)"""
    from test_gpu_block_shapes import _errors
    ro, lu = oracle_steps(oracle, od, xhat, n_steps, **kw), oracle_steps(oracle, od, xhat, n_steps, lu=True, **kw)
    n, u = ro.A.shape
    ro.sigma02, lu.sigma02 = float(ro.v @ (ro.P * ro.v)) / (n - u), float(lu.v @ (lu.P * lu.v)) / (n - u)
    s_s02 = abs(lu.sigma02 - ro.sigma02) / ro.sigma02
    return dict(od=od, ro=ro, lu=lu, Pw=ro.P, spread=_errors(lu.xhat, ro.xhat, ro), s_s02=s_s02,
                vtol=max(1e-9, 20 * s_s02), s_eff=float(np.abs(lu.eff - ro.eff).max()))


def cov_diag(oracle, od, ro, Pw):
    """oracle.covariance's diagonal with the weighted P (main.m:428-444, :460-482, :602)"""
    ns = SimpleNamespace(settings=od.settings)
    _, Cx = oracle.solve_dense(ns, ro.A, ro.w, ro.G, Pw)
    d = np.diag(Cx).copy()
    sc = oracle.descale(od, np.ones(len(d)), ro.dist_scaling)  # 1 / dist_scaling on the distortion entries
    return ro.sigma02 * d * sc ** 2


# ---- checks -----------------------------------------------------------------------------------------------------
def check_solution(tag, ref, xhat, v, rsd, st, ds):
    """xhat, v (raw), rsd, RMS, sigma0^2 at _every_pass's bars; prints the measured figures first"""
    from test_gpu_block_shapes import _errors, _fmt
    ro, spread, vtol = ref["ro"], ref["spread"], ref["vtol"]
    err = _errors(xhat, ro.xhat, ro)
    e_s02 = abs(st[3] - ro.sigma02) / ro.sigma02
    e_v = float(np.abs(v - ro.v).max() / np.abs(ro.v).max())
    e_rsd = float(np.abs(rsd[:, 1:] - ro.rsd[:, 1:]).max() / np.abs(ro.rsd[:, 1:]).max())
    print(f"weights {tag} (error/oracle's own spread): sigma02={e_s02:.1e}/{ref['s_s02']:.1e} v={e_v:.1e} rsd={e_rsd:.1e} "
          + _fmt(err, spread))
    failed = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
    assert not failed, failed
    assert e_s02 <= vtol
    np.testing.assert_allclose(st[:2], ro.rms[:2], rtol=vtol)
    assert e_v <= 10 * vtol and e_rsd <= 10 * vtol
    xptol = 20 * max(spread.get("xp", 0), spread.get("yp", 0)) * np.abs(ds.xy).max()
    np.testing.assert_allclose(rsd[:, 0], ro.rsd[:, 0], rtol=1e-12, atol=max(1e-9, xptol))


def check_adjustment(tag, oracle, ref, res, ds):
    """a whole fba.adjust(..., weights=, reliability=True) against weighted_oracle's reference"""
    from test_gpu_reliability import _check
    ro = ref["ro"]
    assert res.iterations == ro.iterations
    check_solution(tag, ref, res.xhat, res.v, res.rsd, (*res.rms, res.sigma02), ds)
    import flag_masks as fm
    cdo = cov_diag(oracle, ref["od"], ro, ref["Pw"])
    cdl = cov_diag(oracle, ref["od"], ref["lu"], ref["Pw"])
    own = max(fm.cov_self_spread(_Weighted(oracle, ref["Pw"]), ref["od"], ro)[0], float(np.max(np.abs(cdl - cdo) / cdo)))
    e_c = float(np.max(np.abs(res.cx_diag - cdo) / np.abs(cdo)))
    print(f"weights {tag}: diag(Cx) max relative error {e_c:.2e} (bar {max(1e-8, 20 * own):.1e}, oracle's own spread {own:.1e})")
    np.testing.assert_allclose(res.cx_diag, cdo, rtol=max(1e-8, 20 * own), atol=0)
    _check(f"weights {tag}", res, ref["rel"], ref["od"], ro)


def run_ctx(ctx, steps):
    for _ in range(steps):
        ctx.step()
    v, rsd, st = ctx.residuals()
    return SimpleNamespace(xhat=ctx.get_xhat(), v=v, rsd=rsd, st=st, weights=ctx.get_weights())


def _ctx(fba, ds, **kw):
    return fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("weights"), "scenes": {}, "cache": {}}


def blunder_folder(root, name="cam0_blunder"):
    """cam0 with +BLUNDER_PX on the x of PHO row BLUNDER_ROW (the .pho line, three decimals as the file's)"""
    dst = os.path.join(str(root), name)
    if not os.path.isdir(dst):
        shutil.copytree(CAM0, dst)
        path = os.path.join(dst, "cam0.pho")
        lines = open(path).read().splitlines()
        c = lines[BLUNDER_ROW].split("\t")
        c[2] = f"{float(c[2]) + BLUNDER_PX:.3f}"
        lines[BLUNDER_ROW] = "\t".join(c)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return dst


# ---- 1. weighted cam0 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["stage3_pinhole", "stage3_noic_pinhole", "stage3_fisheye"])
def test_weighted_cam0(fba, oracle, cam0_folders, variant):
    """the border on and off, the fish-eye model: xhat, iterations, raw v, RSD, sigma0^2, diag(Cx), r and w"""
    od = oracle.load_folder(cam0_folders[variant])
    wt = random_weights(od.n, 11)
    ref = weighted_oracle(oracle, od, wt)
    ds = fba.load_folder(cam0_folders[variant])
    res = fba.adjust(ds, weights=wt, reliability=True)
    check_adjustment(f"cam0 {variant}", oracle, ref, res, ds)
    # the effective weights without a loss are the user's (the device keeps their square root)
    np.testing.assert_allclose(res.weights, wt, rtol=4e-16)


# ---- 2. weighted small shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["u129-leaf12", "control-leaf12"])
def test_weighted_block_shapes(fba, oracle, work, row, monkeypatch):
    """cross-block observations (k_rel_pts through the rr / cc swap) and control observations (k_rel_ctl) with
    whitened rows"""
    from test_gpu_block_shapes import _scene, _set_leaf, assert_shape
    _set_leaf(monkeypatch, row)
    s = _scene(fba, work, row)
    od = oracle.load_folder(s["folder"])
    wt = random_weights(od.n, 12)
    ref = weighted_oracle(oracle, od, wt)
    assert_shape(fba, s["ds"], row)
    res = fba.adjust(s["ds"], weights=wt, reliability=True)
    check_adjustment(f"block-shapes {row}", oracle, ref, res, s["ds"])


@pytest.mark.parametrize("name", ["dup", "rig2"])
def test_weighted_general_points(fba, oracle, tmp_path, name):
    """the k_gen_* path reading whitened d_J: points measured twice in one image, points seen through two cameras"""
    from test_gpu_general import SCENES, _folder, _general_count
    folder = _folder(tmp_path, name, **SCENES[name])
    od = oracle.load_folder(folder)
    assert _general_count(od) > 0
    # (rig2 under seed 13 has a weighted deltasum of 1.01e-6, at Threshold_Value; under 33 2.3e-6 then 2.2e-8)
    wt = random_weights(od.n, {"dup": 13, "rig2": 33}[name])
    ref = weighted_oracle(oracle, od, wt)
    ds = fba.load_folder(folder)
    res = fba.adjust(ds, weights=wt, reliability=True)
    check_adjustment(f"general {name}", oracle, ref, res, ds)


def test_weighted_partial_flag_set(fba, oracle, work):
    """EOPs not estimated (flag_masks' no_Zc_kappa on its control scene): zero columns stay zero under whitening"""
    import flag_masks as fm
    folder = fm.synth_folder(work["root"], "control", "no_Zc_kappa")
    od = oracle.load_folder(folder)
    wt = random_weights(od.n, 14)
    ref = weighted_oracle(oracle, od, wt)
    ds = fba.load_folder(folder)
    res = fba.adjust(ds, weights=wt, reliability=True)
    check_adjustment("mask no_Zc_kappa", oracle, ref, res, ds)


# ---- 3. constant weights ----------------------------------------------------------------------------------------
def test_constant_weights(fba, oracle, cam0_folders):
    """all weights c = 4: xhat and r are the unweighted run's, sigma0^2 is c times it, and the standardised
    residual -- v s / (sigma sqrt(r)) with s = sqrt(c) -- sqrt(c) times it (P scaled by c is sigma scaled by
    1 / sqrt(c)), all within the unweighted oracle's bars; weights NULL and all ones are bitwise a fresh context"""
    from test_gpu_reliability import _check
    c = 4.0
    folder = cam0_folders["stage3_pinhole"]
    od = oracle.load_folder(folder)
    ref = weighted_oracle(oracle, od, np.ones(od.n))  # the unweighted oracle, with this module's bars
    ds = fba.load_folder(folder)
    res = fba.adjust(ds, weights=np.full(od.n, c), reliability=True)
    assert res.iterations == ref["ro"].iterations
    check_solution("constant c=4", ref, res.xhat, res.v, res.rsd, (*res.rms, res.sigma02 / c), ds)
    np.testing.assert_array_equal(res.weights, np.full(od.n, c))
    _check("weights constant c=4", dataclasses.replace(res, wstat=res.wstat / np.sqrt(c)), ref["rel"], od, ref["ro"])
    outs = []
    for how in ("fresh", "null", "ones"):
        ctx = _ctx(fba, ds)
        try:
            if how == "null":
                ctx.set_weights(random_weights(od.n, 1))
                ctx.set_weights(None)
            elif how == "ones":
                ctx.set_weights(np.ones(od.n))
            o = run_ctx(ctx, 3)
            o.rel = ctx.reliability(o.st[3])
            outs.append(o)
        finally:
            ctx.close()
    for o in outs[1:]:
        for a, b in [(o.xhat, outs[0].xhat), (o.v, outs[0].v), (o.rsd, outs[0].rsd), (o.st, outs[0].st)] + \
                list(zip(o.rel, outs[0].rel)):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(o.weights, np.ones(od.n))


# ---- 4. fba_build_awg -------------------------------------------------------------------------------------------
def test_build_awg_stays_raw(fba, oracle, cam0_folders):
    """with weights set fba_build_awg still returns the reference's raw A, w, bitwise a context's without; the
    step and residuals that follow are the weighted oracle's"""
    folder = cam0_folders["stage3_pinhole"]
    od = oracle.load_folder(folder)
    ds = fba.load_folder(folder)
    wt = random_weights(od.n, 15)
    x0 = oracle.buildxhat(od)[0]
    plain, ctx = _ctx(fba, ds), _ctx(fba, ds)
    try:
        A0, w0, G0, _ = plain.build_awg(x0)
        ctx.set_weights(wt)
        ctx.set_loss("huber", HUBER_K)
        A1, w1, G1, _ = ctx.build_awg(x0)
        np.testing.assert_array_equal(A1, A0)
        np.testing.assert_array_equal(w1, w0)
        np.testing.assert_array_equal(G1, G0)
        ctx.set_loss("none")
        ref = _steps_ref(oracle, od, x0, 1, wt=wt)
        o = run_ctx(ctx, 1)
        check_solution("after build_awg, one step", ref, o.xhat, o.v, o.rsd, o.st, ds)
    finally:
        plain.close()
        ctx.close()


# ---- 5. robust loss ---------------------------------------------------------------------------------------------
def _robust_scene(fba, oracle, work):
    c = work["cache"]
    if "robust" not in c:
        folder = blunder_folder(work["root"])
        od, odc = oracle.load_folder(folder), oracle.load_folder(CAM0)
        c["robust"] = dict(folder=folder, od=od, odc=odc, l2=oracle.adjust(od), clean=oracle.adjust(odc))
    return c["robust"]


def _dist(oracle_result, x, ref_x):
    """the norm of this module's xhat comparisons: the largest per-group relative error"""
    from conftest import group_rel_err
    return max(group_rel_err(x, ref_x, oracle_result.names, oracle_result.dist_scaling).values())


@pytest.mark.parametrize("loss,k", [("huber", HUBER_K), ("cauchy", CAUCHY_K)])
def test_robust_loss_three_irls_steps(fba, oracle, work, loss, k):
    """cam0 with the planted blunder: L2 to convergence, then exactly 3 steps under the loss (fixed counts, so the
    two sides cannot differ by an iteration at the threshold); xhat, raw v, RSD, effective weights, sigma0^2 against
    the oracle's same 3 IRLS steps.

    The qualitative condition, checked with the oracle alone before it was written here.  (a) holds: the blundered
    point has the smallest effective weight of the scene, below 0.5 (Huber 0.066, next 0.25; Cauchy 0.013, next
    0.15).  (b) "the robust xhat lies closer to the clean scene's L2 solution than the blundered L2 solution does"
    does NOT hold on cam0 and is not asserted: cam0 is real data, the loss also down-weights its own large
    residuals (26 / 34 further points below 0.5), and that moves the robust solution away from the clean L2
    solution by more than the blunder moved the L2 solution (largest per-group relative distance 0.105 Huber, 0.118
    Cauchy, against L2's 0.086).  What the loss is for holds and is asserted instead, like against like: the
    blunder moves the robust solution less than it moves the L2 solution -- robust(blundered) against the same 3
    robust steps on the clean scene, 7.0e-3 / 4.8e-3, against L2(blundered) to L2(clean), 8.6e-2."""
    s = _robust_scene(fba, oracle, work)
    od, l2, clean = s["od"], s["l2"], s["clean"]
    ref = _steps_ref(oracle, od, l2.xhat, 3, loss=loss, k=k)
    ro = ref["ro"]
    rc = oracle_steps(oracle, s["odc"], clean.xhat, 3, loss=loss, k=k)  # the clean scene under the same loss
    pt_eff = ro.eff[0::2]
    assert int(np.argmin(pt_eff)) == BLUNDER_ROW and pt_eff[BLUNDER_ROW] < 0.5
    d_l2, d_rob = _dist(clean, l2.xhat, clean.xhat), _dist(clean, ro.xhat, rc.xhat)
    assert d_rob < d_l2, (d_rob, d_l2)
    ds = fba.load_folder(s["folder"])
    ctx = _ctx(fba, ds)
    try:
        it, _ = ctx.adjust()
        assert it == l2.iterations
        ctx.set_loss(loss, k)
        o = run_ctx(ctx, 3)
    finally:
        ctx.close()
    check_solution(f"robust {loss}", ref, o.xhat, o.v, o.rsd, o.st, ds)
    sig = min(od.settings["Meas_std"], od.settings["Meas_std_y"])
    bar_f = 10 * ref["vtol"] * np.abs(ro.w).max() / (sig * k)
    e_f = float(np.abs(o.weights - ro.eff).max())
    print(f"weights robust {loss}: effective weight error {e_f:.2e} (bar {bar_f:.1e}, oracle's own spread {ref['s_eff']:.1e}) "
          f"blunder weight {o.weights[2 * BLUNDER_ROW]:.4f} (oracle {ro.eff[2 * BLUNDER_ROW]:.4f}) the blunder's pull, robust "
          f"{_dist(clean, o.xhat, rc.xhat):.2e} (oracle {d_rob:.2e}) L2 {d_l2:.2e}; to the clean L2 solution "
          f"{_dist(clean, o.xhat, clean.xhat):.2e}")
    assert e_f <= bar_f
    gp = o.weights[0::2]
    np.testing.assert_array_equal(o.weights[0::2], o.weights[1::2])  # one factor per image point
    assert int(np.argmin(gp)) == BLUNDER_ROW and gp[BLUNDER_ROW] < 0.5
    assert _dist(clean, o.xhat, rc.xhat) < d_l2


# ---- 6. bundle.adjust(robust=) end to end -----------------------------------------------------------------------
def test_adjust_robust_end_to_end(fba, oracle, work, tmp_path):
    """the L2-then-robust schedule, .wgt with the blunder starred; a run with weights=None / robust=None writes
    the files of a run without the options, byte for byte"""
    from fba_amd import report
    s = _robust_scene(fba, oracle, work)
    ds = fba.load_folder(s["folder"])
    res = fba.adjust(ds, robust="huber", reliability=True)
    l2_it = s["l2"].iterations
    cap = int(ds.settings["Iteration_Cap"])
    assert l2_it < res.iterations <= cap and len(res.deltasum) == res.iterations
    assert res.deltasum[l2_it - 1] <= ds.settings["threshold"] < res.deltasum[l2_it]  # the loss restarts the loop
    assert res.deltasum[-1] <= ds.settings["threshold"] or res.iterations == cap
    gp = res.weights[0::2]
    assert int(np.argmin(gp)) == BLUNDER_ROW and gp[BLUNDER_ROW] < 0.5
    # sigma0^2 is the re-weighted state's: v'Pv with the effective weights
    P = oracle.weights(s["od"]) * res.weights
    n, u = 2 * ds.n_pts, len(res.xhat)
    assert abs(res.sigma02 - float(res.v @ (P * res.v)) / (n - u)) <= 1e-12 * res.sigma02
    assert res.sigma02 < s["l2"].sigma02
    files = {}
    for tag, r in (("robust", res), ("plain", fba.adjust(ds, reliability=True)),
                   ("none", fba.adjust(ds, weights=None, robust=None, robust_k=None, reliability=True))):
        out = tmp_path / tag
        out.mkdir()
        fba.bundle.write_outputs(ds, dataclasses.replace(r, seconds=1.25), str(out))
        files[tag] = {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}
    stem = os.path.splitext(ds.settings["Output_Filename"])[0]
    assert set(files["robust"]) - set(files["plain"]) == {stem + ".wgt"}
    assert set(files["none"]) == set(files["plain"]) and stem + ".rel" in files["plain"]
    date = lambda b: [ln for ln in b.splitlines() if b"Date" not in ln and b"date" not in ln]  # noqa: E731
    for f, b in files["plain"].items():
        assert date(files["none"][f]) == date(b), f
    rows, tgt, img, w, flag = report.read_wgt(str(tmp_path / "robust" / (stem + ".wgt")))
    assert rows == list(range(1, ds.n_pts + 1)) and flag[BLUNDER_ROW]
    assert (tgt[BLUNDER_ROW], img[BLUNDER_ROW]) == (ds.pho_target[BLUNDER_ROW], ds.pho_image[BLUNDER_ROW])
    np.testing.assert_array_equal(flag, w.min(axis=1) < report.WGT_FLAG)


# ---- 7. two rank contexts ---------------------------------------------------------------------------------------
def test_two_ranks_with_weights_and_huber(fba, work, oracle):
    """world = 2, replicated solve, reduce buffers summed on the host (test_gpu_reliability._step_ranks): every
    rank takes the full-length weights and keeps its own; the ranks' get_weights sum to the single context's
    vector; xhat is the single context's per group at max(1e-10, 20 x the oracle's own spread) --
    test_gpu_parity.test_sharded_ranks_reassemble_single_gpu_result's 1e-10, and this module's rule where the
    oracle's own two solves (explicit inverse / LU) of the same 4 L2 + 2 Huber passes are further apart than
    that: two passes after the loss is switched on, far from its fixed point, they are, by 4.1e-9 in k4 (1.2e-11 to
    6.9e-11 in k2, k3, k5; below 2e-12 elsewhere).  Weights log-uniform in [0.1, 10] here: the test is about the
    PHO-to-local mapping on each rank, and six decades of weights take the oracle's two routes 4e-10 apart on the
    converged scene already (test_weighted_cam0's print)."""
    from test_gpu_reliability import _step_ranks
    s = _robust_scene(fba, oracle, work)
    ds = fba.load_folder(s["folder"])
    n = 2 * ds.n_pts
    wt = random_weights(n, 17) ** (1.0 / 3.0)
    single = _ctx(fba, ds)
    ranks = [_ctx(fba, ds, rank=r, world=2) for r in range(2)]
    try:
        for c in [single] + ranks:
            c.set_weights(wt)
        _step_ranks(single, ranks, 4)
        for c in [single] + ranks:
            c.set_loss("huber", HUBER_K)
        _step_ranks(single, ranks, 2)
        from test_gpu_block_shapes import _errors
        od = s["od"]
        x0 = oracle.buildxhat(od)[0]
        two = [oracle_steps(oracle, od, oracle_steps(oracle, od, x0, 4, wt=wt, lu=lu).xhat, 2, wt=wt, loss="huber",
                            k=HUBER_K, lu=lu) for lu in (False, True)]
        spread = _errors(two[1].xhat, two[0].xhat, two[0])
        from conftest import group_rel_err
        xs, w1 = single.get_xhat(), single.get_weights()
        v1 = single.residuals()[0]
        pk = ds.pack()
        tie_owner, ctl_owner = fba.capi.partition(pk, 2)
        owner = np.where(pk.tie >= 0, tie_owner[np.maximum(pk.tie, 0)], ctl_owner)
        ws = []
        for r, c in enumerate(ranks):
            w = c.get_weights()
            mine = np.repeat(owner == r, 2)
            assert (w[~mine] == 0).all() and (w[mine] > 0).all()
            ws.append(w)
        xr = sum(c.get_xhat(owned_only=True) for c in ranks)
        _, _, _, dsc = single.build_awg(xs)
        err = group_rel_err(xr, xs, fba.xhat_names(ds), dsc)
        # the loss factor f(t), |f'| <= 1 / k, of t = sqrt(weight) |misclosure| / sigma, the ranks' misclosures
        # at 1e-9 of their scale (test_gpu_reliability's two-rank bar on v), times the user weight
        sig = min(ds.settings["Meas_std"], ds.settings["Meas_std_y"])
        wp = np.repeat(wt.reshape(-1, 2).max(axis=1), 2)
        bar = wt * np.sqrt(wp) * 1e-9 * np.abs(v1).max() / (sig * HUBER_K)
        e_w = np.abs(ws[0] + ws[1] - w1)
        print("weights two ranks: xhat (error/oracle's own spread) " + " ".join(f"{g}={e:.1e}/{spread[g]:.1e}" for g, e in err.items())
              + f"; summed effective weights, worst error/bar {e_w.max():.2e}/{bar[int(np.argmax(e_w / bar))]:.2e}, "
              f"{int((w1 < wt * 0.999).sum() // 2)} points down-weighted")
        failed = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-10, 20 * spread[g])]
        assert not failed, failed
        assert (e_w <= bar).all()
        assert (w1 < wt * 0.999).any()  # the loss is in force
    finally:
        for c in [single] + ranks:
            c.close()


# ---- 8. state ---------------------------------------------------------------------------------------------------
def test_state_and_arguments(fba, cam0_folders):
    """a setter after a solve invalidates the factor and the linearisation (FBA_ERR_ARG from fba_covariance,
    fba_reliability, fba_residuals); entries that are 0, negative, NaN or Inf are refused with a message and change
    nothing; two identical weighted runs are bitwise equal"""
    ds = fba.load_folder(cam0_folders["stage3_pinhole"])
    n = 2 * ds.n_pts
    wt = random_weights(n, 18)
    ctxs = []

    def stepped():
        c = _ctx(fba, ds)
        ctxs.append(c)
        c.set_weights(wt)
        for _ in range(3):
            c.step()
        c.set_loss("cauchy", CAUCHY_K)
        return c, run_ctx(c, 2)
    try:
        (a, oa), (b, ob) = stepped(), stepped()
        for x, y in ((oa.xhat, ob.xhat), (oa.v, ob.v), (oa.st, ob.st), (oa.weights, ob.weights)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a.reliability(oa.st[3]), b.reliability(ob.st[3])):
            np.testing.assert_array_equal(x, y)
        for setter in (lambda c: c.set_weights(wt), lambda c: c.set_weights(None), lambda c: c.set_loss("none"),
                       lambda c: c.set_loss("huber")):
            c, o = stepped()
            setter(c)
            for call in (lambda: c.covariance(o.st[3]), lambda: c.reliability(o.st[3]), c.residuals, c.get_weights):
                with pytest.raises(fba.capi.FBAError) as ei:
                    call()
                assert ei.value.code == 1  # FBA_ERR_ARG
            c.step()  # and the context goes on
            c.covariance(c.residuals()[2][3])
        c, o = stepped()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            w = wt.copy()
            w[7] = bad
            with pytest.raises(fba.capi.FBAError) as ei:
                c.set_weights(w)
            assert ei.value.code == 1 and "weight[7]" in str(ei.value)
        c.covariance(o.st[3])  # a refused call left the factor in place
    finally:
        for c in ctxs:
            c.close()
