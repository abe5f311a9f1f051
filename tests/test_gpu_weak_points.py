"""The tie-point elimination on the GPU where a point's rays barely intersect: V = Jp'PJp with cond 1e4 .. 1e10.

Every unknown passes through V twice -- V^-1 by the adjugate (the point table, V^-1 b, T = W V^-1, the back-substitution,
k_cov_pts, fba_rel.hip) and R = L^-T from an unguarded Cholesky (U = W R, the reduced system and its right-hand side) --
in k_lin_reduce phase (B), k_lin_point and k_gen_point.  The scenes are weak_scenes' (twin images of base B = 30, 3, 0.3,
0.03 with weak points seen by a pair only; variants chunk, rig, dup, free, excluded), from the file start values.

The reference is exact_solve.solve, 50-digit mpmath, on the ORACLE's A, w, P at the linearisation point (the device's
linearisation agrees with the oracle's to 1e-12, test_gpu_parity._check_awg's bars, asserted here first); the oracle's
own explicit inverse is 5e-5 .. 3e-2 off at tiers 0.3 and 0.03 and is not used.

Per scene (test_pass_and_postfit): the linearisation; x1 = get_xhat() after one step() against x0 + descale(exact delta);
fba_postfit_outputs(sigma02 = 1, reliability on) -- cx_tie and cx_diag against the exact cofactor blocks V^-1 + T C T'
and the camera-side diagonal, redundancy against 1 - p a Cx a', every redundancy number of a weak point's observations
within [0, 1] (include/fba.h's contract; slack: the yardstick's absolute error), the ellipsoids' semi-axes against
capi.eig3_host of the exact block; everything finite.  The chunk scenes at tier 0.3 also take a second pass from x1
(the weak points move by ~1e4 units in pass one) and a pass under set_damping(1e-3), whose exact reference is the damped
system as include/fba.h defines it (no post-fit output after a damped solve).

Metrics: (a) cam_group / cam_elem, conftest's xhat metrics over the camera-side groups; (b) tie_group / tie_elem, the
same over the tie points; (c) weak_delta, per weak point |d_gpu - d_exact|_2 / |d_exact|_2 with d_gpu = x1 - x0 (the
subtraction costs eps |x0| / |d|, the worst tie point's is added to the bar: <= 1e-11 from the start values,
asserted, 1.5e-11 in the second pass, whose x is 1e4 .. 1e5 units from the block); (d) strong_delta, the same per
well-determined point; (e) weak_block / strong_block, covariance entries relative to their block's largest entry
(cx_diag's tie entries in the same metric), cam_diag relative per entry, weak_axes / strong_axes |d a_i^2| / a_max^2;
(f) redundancy, absolute.

Bars, none from a run: max(1e-9, 20 x the yardstick of the same scene in the same metric), the yardstick being fp64
oracle.solve_schur (the pass) and weak_scenes.block_fp64 (cofactors, a Cx a', the damped pass) against the exact
solve.  The floors: 1e-8 for redundancy (test_gpu_reliability.R_FLOOR), 3e-9 for the axes (Weyl: entries within 1e-9
of the block's largest move an eigenvalue by at most 3e-9 of it).  tests/test_weak_points_host.py holds 20 x every
yardstick below 1e-3.  One run's figures beside the yardsticks: profiles/weak_points_gpu_errors.log (the "weak ..."
prints of this module).
"""
import numpy as np
import pytest

import weak_scenes as ws

pytestmark = pytest.mark.gpu

R_FLOOR = 1e-8   # test_gpu_reliability.R_FLOOR
FLOORS = {"redundancy": R_FLOOR, "weak_axes": 3e-9, "strong_axes": 3e-9}
CANCEL = 1e-11   # eps |x0| / |d|, the cost of d = x1 - x0, from the start values


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("weak_points"), "scenes": {}}


def _scene(fba, oracle, work, name):
    from fba_amd import synth
    s = ws.load(synth, oracle, work["root"], work["scenes"], name)
    if "ds" not in s:
        s["ds"] = fba.load_folder(s["folder"])
    return s


def _ctx(fba, s):
    ctx = fba.capi.Context(s["ds"].pack(), fba.capi.make_settings(s["ds"].settings))
    if s["b"]["weights"] is not None:
        ctx.set_weights(s["b"]["weights"])
    return ctx


def _bars(y, cancel=0.0):
    out = {k: ws.bar(v, FLOORS.get(k, 1e-9)) for k, v in y.items()}
    for k in ("weak_delta", "strong_delta"):
        if k in out:
            out[k] += cancel
    return out


def _report(tag, err, y, bars):
    print()
    for k, e in err.items():
        print(f"weak {tag}: {k:13s} device {e:.2e}  yardstick {y[k]:.2e}  bar {bars[k]:.2e}  device/yardstick "
              f"{e / max(y[k], 1e-300):.2f}")
    bad = {k: (e, bars[k]) for k, e in err.items() if not e <= bars[k]}
    assert not bad, f"{tag}: (device error, bar) {bad}"


def _check_pass(fba, tag, s, lin, ep, y, x_new, first=True):
    assert np.isfinite(x_new).all()
    b, uc = s["b"], ep["uc"]
    weak = b["weak"] + b["cut"]
    cancel = ws.delta_cancellation(lin["x"], ep["x1"], uc)
    assert cancel <= (CANCEL if first else 10 * CANCEL)
    err = ws.pass_errors(x_new, ep["x1"], lin["x"], s["names"], lin["dsc"], uc, weak, b["strong"])
    _report(tag, err, y, _bars(y, cancel))


def _check_postfit(fba, tag, s, lin, ep, y, out):
    cxd, corr, red, wst, blk, ell = out
    for a in out:
        assert np.isfinite(a).all()
    b, uc, ex = s["b"], ep["uc"], ep["exact"]
    weak = b["weak"] + b["cut"]
    nt = len(ex["cx_tie"])
    assert blk.shape == (nt, 6) and ell.shape == (nt, 12) and red.shape == (len(lin["w"]),)
    blocks = fba.capi.tie_blocks(blk)
    err = ws.block_errors(blocks, ex["cx_tie"], weak, b["strong"])
    # cx_diag's tie entries, in the blocks' metric
    e_dg = (np.abs(cxd[uc:].reshape(-1, 3) - np.einsum("tii->ti", ex["cx_tie"])).max(axis=1)
            / np.abs(ex["cx_tie"]).max(axis=(1, 2)))
    err["weak_block"] = max(err["weak_block"], float(e_dg[weak].max()))
    err["strong_block"] = max(err["strong_block"], float(e_dg[b["strong"]].max()))
    sc = s["oracle"].descale(s["od"], np.ones(len(cxd)), lin["dsc"])[:uc]   # 1 / dist_scaling on the distortion entries
    err["cam_diag"] = float(np.abs(cxd[:uc] / (ex["cx_cam_diag"] * sc ** 2) - 1).max())
    ref_ell = fba.capi.eig3_host(ws.pack6(ex["cx_tie"]))
    e_ax = np.abs(ell[:, :3] ** 2 - ref_ell[:, :3] ** 2).max(axis=1) / ref_ell[:, 0] ** 2
    err["weak_axes"], err["strong_axes"] = float(e_ax[weak].max()), float(e_ax[b["strong"]].max())
    r_ref = 1.0 - lin["P"] * ex["aCa"]
    err["redundancy"] = float(np.abs(red - r_ref).max())
    _report(tag, err, y, _bars(y))
    rows = np.nonzero(np.any([np.any(lin["A"][:, uc + 3 * t:uc + 3 * t + 3] != 0, axis=1) for t in weak], axis=0))[0]
    assert len(rows) >= 4 * len(b["weak"])
    print(f"weak {tag}: redundancy of the weak points' {len(rows)} observations {red[rows].min():.3e} .. "
          f"{red[rows].max():.6f} (exact {r_ref[rows].min():.3e} .. {r_ref[rows].max():.6f}), slack {y['redundancy']:.1e}; "
          f"a/c of the weak ellipsoids up to {(ell[weak, 0] / ell[weak, 2]).max():.3g}")
    assert (red[rows] >= -y["redundancy"]).all() and (red[rows] <= 1 + y["redundancy"]).all()


def _reference(fba, oracle, s, key, lin, lam=0.0):
    """the exact pass of one linearisation and its yardsticks, cached under key"""
    if key not in s:
        ep = ws.exact_pass(oracle, s["od"], lin, lam)
        y = ws.yardsticks(s, lin, ep, fba.capi.eig3_host)
        s[key] = (ep, y)
    s["oracle"] = oracle
    return s[key]


@pytest.mark.parametrize("name", sorted(ws.SCENES))
def test_pass_and_postfit(fba, oracle, work, name):
    from test_gpu_parity import _check_awg
    s = _scene(fba, oracle, work, name)
    ep, y = _reference(fba, oracle, s, "pass1", s["lin"])
    _check_awg(fba, oracle, s["ds"], s["od"], s["x0"])
    ctx = _ctx(fba, s)
    try:
        np.testing.assert_array_equal(ctx.buildxhat(), s["x0"])
        assert np.isfinite(ctx.step())   # an error code of fba_step raises
        x1 = ctx.get_xhat()
        out = ctx.postfit(1.0, reliability=True)
    finally:
        ctx.close()
    _check_pass(fba, name, s, s["lin"], ep, y, x1)
    _check_postfit(fba, name, s, s["lin"], ep, y, out)


@pytest.mark.parametrize("typ", ["fisheye", "pinhole"])
def test_second_pass(fba, oracle, work, typ):
    """from the device's own x1: the weak points have moved by ~1e4 units, the linearisation point is far from the
    first; the exact reference is taken at that x1"""
    from test_gpu_parity import _check_awg
    name = f"chunk-{typ}-B0.3"
    s = _scene(fba, oracle, work, name)
    ctx = _ctx(fba, s)
    try:
        assert np.isfinite(ctx.step())
        x1 = ctx.get_xhat()
        assert np.isfinite(ctx.step())
        x2 = ctx.get_xhat()
        out = ctx.postfit(1.0, reliability=True)
    finally:
        ctx.close()
    assert np.isfinite(x1).all()
    uc = ws.uc_of(oracle, s["od"])
    moved = np.linalg.norm((x1 - s["x0"])[uc:].reshape(-1, 3)[s["b"]["weak"]], axis=1)
    print(f"weak {name} pass 2: the weak points moved by {moved.min():.3g} .. {moved.max():.3g} in pass one")
    assert moved.max() > 1e3
    _check_awg(fba, oracle, s["ds"], s["od"], x1)
    lin = ws.linearise(oracle, s["od"], x1, s["b"]["weights"])
    ep, y = _reference(fba, oracle, s, "pass2", lin)
    _check_pass(fba, name + " pass 2", s, lin, ep, y, x2, first=False)
    _check_postfit(fba, name + " pass 2", s, lin, ep, y, out)


@pytest.mark.parametrize("typ", ["fisheye", "pinhole"])
def test_damped_pass(fba, oracle, work, typ):
    """set_damping(1e-3), the project's own remedy for such points and the WH = true kernels' lambda: V + lambda diag(V),
    then S' + lambda diag(S'), formed in mp"""
    name = f"chunk-{typ}-B0.3"
    s = _scene(fba, oracle, work, name)
    ep, y = _reference(fba, oracle, s, "damped", s["lin"], ws.LAMBDA)
    y = {k: v for k, v in y.items() if k in ws.PASS_METRICS}
    ctx = _ctx(fba, s)
    try:
        ctx.set_damping(ws.LAMBDA)
        assert np.isfinite(ctx.step())
        x1 = ctx.get_xhat()
    finally:
        ctx.close()
    _check_pass(fba, name + " damped", s, s["lin"], ep, y, x1)
