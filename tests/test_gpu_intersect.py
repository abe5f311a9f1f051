"""GPU: forward intersection -- fba_image_rays and fba_intersect (csrc/fba_intersect.hip) against the numpy restatement
(tests/intersect_ref.py), and adjust(..., intersect=True) end to end.

Scenes are synth.generate(12, 40, seed=3, ...) packed without files (intersect_ref.pack_scene), pinhole and
orthographic with max_theta_deg = 60; the restatement of each scene is computed once per module.

Bars, none from a device run:
  rays           device libm against host libm: 1e-12 per component; the centres are xhat's bit for bit
  linear, exact  noise 0, true EOP / IOP: |xyz - X_true| <= 1e-8 object units (the restatement gives 1.3e-11 .. 1.7e-11,
                 three decimal orders are left for the device's libm); measured on the device: see DESIGN.md 6g
  linear, noisy  max(1e-9, 100 x the fp64 / longdouble spread of the restatement) object units (the spread is
                 7e-12 .. 1.4e-11 here, so the bar is 1e-9 .. 1.4e-9); lambda_min / lambda_max to 1e-10
  refined        100 x refine_tol x the mean distance to the centres (both are fixed points of one contraction,
                 each stopped where its step fell below refine_tol x distance); RMS final <= RMS linear
  everything else is bitwise.
"""
import os

import numpy as np
import pytest

import intersect_ref as ir

pytestmark = pytest.mark.gpu

SHIFT = np.array([1500.0, -1500.0, 800.0])
_CACHE = {}


def _theta(typ):
    return 60.0 if typ in ("pinhole", "orthographic") else 80.0


def _scene(fba, typ="fisheye", noise=0.3, opp=3, n_img=12, **kw):
    from fba_amd import synth
    key = (typ, noise, opp, n_img, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = synth.generate(n_img, 40, seed=3, obs_per_point=opp, noise=noise, typ=typ,
                                     max_theta_deg=_theta(typ), **kw)
    return synth, _CACHE[key]


def _ctx(fba, pk, typ, nk, est_iop=True, **kw):
    s = ir.settings_dict(typ, nk)
    if not est_iop:
        for k in ("Estimate_xp", "Estimate_yp", "Estimate_c", "Estimate_radial", "Estimate_decent"):
            s[k] = 0
    return fba.capi.Context(pk, fba.capi.make_settings(s), **kw)


def _restate(pk, typ, nk, key, **kw):
    """(fp64 results, longdouble results) of intersect_ref.intersect_all, cached"""
    key = ("ref", key, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = (ir.intersect_all(ir.Problem(pk, typ, nk), **kw),
                       ir.intersect_all(ir.Problem(pk, typ, nk, dtype=np.longdouble), **kw))
    return _CACHE[key]


# ---- 4. fba_image_rays ----------------------------------------------------------------------------------------------
def _check_rays(fba, synth, sc, typ, nk):
    pk = ir.pack_scene(fba.capi, synth, sc, nk, truth=True)          # K and P not zero
    with _ctx(fba, pk, typ, nk) as ctx:
        ray, st = ctx.image_rays()
        x = ctx.get_xhat()
    assert ray.shape == (pk.n_pts, 6) and (st == 0).all() and (pk.tie < 0).sum() > 0
    eop = x[: 6 * pk.n_img].reshape(-1, 6)
    assert np.array_equal(ray[:, :3], eop[pk.img, :3])                # bit for bit xhat's
    pb = ir.Problem(pk, typ, nk)
    iop, ydir = pk.iop0.reshape(pk.n_cam, 5 + nk), pk.cam_info.reshape(-1, 5)[:, 0]
    d = np.zeros((pk.n_pts, 3))
    for k in range(pk.n_cam):
        rows = np.nonzero(pk.cam == k)[0]
        ct = np.concatenate([iop[k, :3], [ydir[k]], iop[k, 3 + nk:], iop[k, 3:3 + nk]])
        out, hst = fba.capi.unproject_host(typ, pk.xy.reshape(-1, 2)[rows], ct)
        assert (hst == 0).all()
        d[rows] = np.einsum("nji,nj->ni", pb.M[rows], out[:, 2:])
    err = float(np.abs(ray[:, 3:] - d).max())
    print(f"rays {typ} nk {nk} cams {pk.n_cam}: max |d_device - d_host| {err:.2e}")
    assert err <= 1e-12
    assert np.abs(np.linalg.norm(ray[:, 3:], axis=1) - 1).max() <= 1e-15 * 4


@pytest.mark.parametrize("nk", [1, 5, 8])
@pytest.mark.parametrize("typ", ir.TYPES)
def test_image_rays(fba, typ, nk):
    synth, sc = _scene(fba, typ, n_control=5)
    _check_rays(fba, synth, sc, typ, nk)


def test_image_rays_two_cameras(fba):
    synth, sc = _scene(fba, "fisheye", n_control=5, n_cam=2, cam_layout="alternate")
    _check_rays(fba, synth, sc, "fisheye", 5)


# ---- 5. linear intersection -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", ir.TYPES)
def test_linear_exact_at_the_truth(fba, typ):
    synth, sc = _scene(fba, typ, noise=0.0)
    pk = ir.pack_scene(fba.capi, synth, sc, 5, truth=True)
    with _ctx(fba, pk, typ, 5) as ctx:
        xyz, q, st, bad = ctx.intersect(refine_iters=0)
    err = float(np.abs(xyz - sc["X_true"]).max())
    print(f"linear exact {typ}: max |xyz - X_true| {err:.2e} object units; max RMS {q[:, 2].max():.2e} px")
    assert bad == 0 and (st == 0).all() and (q[:, 0] == 3).all()
    assert err <= 1e-8
    assert np.array_equal(q[:, 2], q[:, 3])                          # no refinement: final = linear


LINEAR_CASES = {
    "rays2": dict(opp=2), "rays3": dict(opp=3), "rays9": dict(opp=9),
    "wide": dict(opp=3, n_img=30, n_wide=1, wide_min_obs=17),
    "rig": dict(opp=3, n_cam=2, cam_layout="alternate"),
    **{t: dict(typ=t, opp=3) for t in ir.TYPES[1:]},
}


def _compare(fba, name, refine_iters):
    kw = dict(LINEAR_CASES[name])
    typ = kw.pop("typ", "fisheye")
    synth, sc = _scene(fba, typ, **kw)
    pk = ir.pack_scene(fba.capi, synth, sc, 5)                       # the scene's own C0 / ang0, start IOPs
    r64, rld = _restate(pk, typ, 5, name, refine_iters=refine_iters)
    with _ctx(fba, pk, typ, 5) as ctx:
        out = ctx.intersect(refine_iters=refine_iters)
    return sc, pk, r64, rld, out


@pytest.mark.parametrize("name", sorted(LINEAR_CASES))
def test_linear_against_the_restatement(fba, name):
    sc, pk, r64, rld, (xyz, q, st, bad) = _compare(fba, name, 0)
    if name == "wide":
        assert max(r["rays"] for r in r64) >= 17                    # more than two passes of the 8 lanes
    spread = max(float(np.abs(a["lin"] - b["lin"].astype(np.float64)).max()) for a, b in zip(r64, rld))
    bar = max(1e-9, 100 * spread)
    err = max(float(np.abs(xyz[t] - r["lin"]).max()) for t, r in enumerate(r64))
    e_ratio = max(abs(q[t, 1] - r["ratio"]) for t, r in enumerate(r64))
    e_rms = max(abs(q[t, 2] - r["rms_lin"]) for t, r in enumerate(r64))
    print(f"linear {name}: max |xyz - restatement| {err:.2e} (bar {bar:.2e}, fp64 / longdouble spread {spread:.2e}); "
          f"ratio {e_ratio:.2e}; RMS linear {e_rms:.2e} px; rays {int(q[:, 0].min())} .. {int(q[:, 0].max())}")
    assert bad == 0 and (st == 0).all()
    assert [int(v) for v in q[:, 0]] == [r["rays"] for r in r64]
    assert err <= bar and e_ratio <= 1e-10
    assert e_rms <= 1e-8                                             # positions within 1e-9 units: < 1e-9 px


# ---- 6. refinement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rays2", "rays3", "rays9", "wide", "rig", "orthographic"])
def test_refinement_against_the_restatement(fba, name):
    sc, pk, r64, rld, (xyz, q, st, bad) = _compare(fba, name, 10)
    assert bad == 0 and (st == 0).all()
    worst = 0.0
    for t, r in enumerate(r64):
        assert r["rms_fin"] <= r["rms_lin"]                          # the restatement alone (confirmed on the CPU)
        bar = 100 * 1e-10 * r["dist"]
        e = float(np.abs(xyz[t] - r["fin"]).max())
        worst = max(worst, e / bar)
        assert e <= bar, (t, e, bar)
        assert q[t, 3] <= q[t, 2]
        assert abs(q[t, 3] - r["rms_fin"]) <= 1e-4 and abs(q[t, 2] - r["rms_lin"]) <= 1e-8
    moved = max(float(np.abs(r["fin"] - r["lin"]).max()) for r in r64)
    print(f"refined {name}: worst |xyz - restatement| / bar {worst:.2e}; the refinement moved the points by up to "
          f"{moved:.2e} units in <= {max(r['iters'] for r in r64)} passes; RMS {q[:, 2].max():.3f} -> {q[:, 3].max():.3f} px")


# ---- 7. statuses ----------------------------------------------------------------------------------------------------
def test_statuses(fba):
    typ = "orthographic"
    synth, sc = _scene(fba, typ, opp=3)
    pid, img, xy = sc["pid"], sc["img"], sc["xy"]
    first = {t: np.nonzero(pid == t)[0] for t in (0, 1, 2)}
    keep = np.ones(len(pid), bool)
    keep[first[0][1:]] = False                                       # point 0: one image only -> FEW
    keep[first[1]] = False                                           # point 1: twice in one image, nowhere else -> WEAK
    r1 = first[1][0]
    xy = xy.copy()
    cam0 = synth.camera_params(0)
    xy[first[2][0]] = (cam0[0] + 0.5 + 1.2 * (cam0[2] + 1.0), cam0[1] + 0.5)   # point 2: q = 1.2 > 1 in its first ray
    sc2 = dict(sc, xy=xy)
    pk = ir.pack_scene(fba.capi, synth, sc2, 5, keep=keep, extra=([1, 1], [img[r1], img[r1]], [xy[r1], xy[r1]]))
    pb = ir.Problem(pk, typ, 5)
    r0, r2 = ir.intersect_point(pb, 0), ir.intersect_point(pb, 2)
    with _ctx(fba, pk, typ, 5) as ctx:
        x0 = ctx.get_xhat()
        ray, rst = ctx.image_rays()
        xyz, q, st, bad = ctx.intersect(write_xhat=True)
        x1 = ctx.get_xhat()
    assert rst.sum() == 1 and rst[np.nonzero(pk.tie == 2)[0][0]] == 1
    assert st[0] == 1 and st[1] == 2 and st[2] == 0 and set(st[3:]) <= {0, 3}
    assert bad == int((st != 0).sum()) and bad >= 2
    assert q[0, 0] == 1 and q[1, 0] == 2 and q[1, 1] <= 1e-12 and q[2, 0] == 2
    assert r0 is None and r2["rays"] == 2
    assert np.abs(xyz[2] - r2["fin"]).max() <= 100 * 1e-10 * r2["dist"]
    tie = x0[-3 * pk.n_tie:].reshape(-1, 3)
    assert np.array_equal(xyz[:2], tie[:2])                          # FEW, WEAK: the current value
    assert np.array_equal(x1[-3 * pk.n_tie:].reshape(-1, 3)[:2], tie[:2])   # ... kept bit for bit
    assert np.array_equal(x1[-3 * pk.n_tie:].reshape(-1, 3)[2:], xyz[2:])
    assert np.array_equal(x1[: -3 * pk.n_tie], x0[: -3 * pk.n_tie])


# ---- 8. contract ----------------------------------------------------------------------------------------------------
def _contract_problem(fba):
    synth, sc = _scene(fba, "fisheye", opp=9, n_control=5)
    return ir.pack_scene(fba.capi, synth, sc, 5)


def test_contract_read_only(fba):
    pk = _contract_problem(fba)
    with _ctx(fba, pk, "fisheye", 5, est_iop=False) as ctx, _ctx(fba, pk, "fisheye", 5, est_iop=False) as plain:
        x0 = ctx.get_xhat()
        a = ctx.intersect()
        b = ctx.intersect()
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v)
        ra, rb = ctx.image_rays(), ctx.image_rays()
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        assert np.array_equal(ctx.get_xhat(), x0)
        ctx.accumulate()
        ctx.intersect()                                              # between the two halves: nothing moves either
        d1 = ctx.solve_update()
        d0 = plain.step()
        assert d1 == d0 and np.array_equal(ctx.get_xhat(), plain.get_xhat())
        # not between solve_update_async and solve_finish
        ctx.accumulate()
        ctx.solve_update_async()
        for call in (ctx.intersect, ctx.image_rays):
            with pytest.raises(fba.capi.FBAError) as ei:
                call()
            assert ei.value.code == 1
        ctx.solve_finish()
        plain.step()
        assert np.array_equal(ctx.get_xhat(), plain.get_xhat())


def test_contract_write_xhat(fba):
    pk = _contract_problem(fba)
    with _ctx(fba, pk, "fisheye", 5, est_iop=False) as ctx:
        ctx.step()
        ctx.residuals()
        x0 = ctx.get_xhat()
        xyz, q, st, bad = ctx.intersect(write_xhat=True)
        with pytest.raises(fba.capi.FBAError) as ei:
            ctx.residuals()
        assert ei.value.code == 1
        x1 = ctx.get_xhat()
        nt = pk.n_tie
        assert np.array_equal(x1[: -3 * nt], x0[: -3 * nt])
        ok = (st == 0) | (st == 3)
        t0, t1 = x0[-3 * nt:].reshape(-1, 3), x1[-3 * nt:].reshape(-1, 3)
        assert ok.all() and np.array_equal(t1[ok], xyz[ok]) and np.array_equal(t1[~ok], t0[~ok])
        assert (t1 != t0).any()
        assert np.isfinite(ctx.step())
        ctx.residuals()


def test_contract_weights_loss_priors(fba):
    pk = _contract_problem(fba)
    with _ctx(fba, pk, "fisheye", 5, est_iop=False) as plain:
        want = plain.intersect()
    rng = np.random.default_rng(5)
    pri = (np.array([0, 7]), np.array([100.0, 0.1]), np.array([1.0, 0.01]))
    with _ctx(fba, pk, "fisheye", 5, est_iop=False, priors=pri) as ctx:
        ctx.set_weights(rng.uniform(0.5, 2.0, 2 * pk.n_pts))
        ctx.set_loss("huber")
        ctx.set_damping(1e-3)
        got = ctx.intersect()
    for u, v in zip(want, got):
        assert np.array_equal(u, v)


# ---- 9. two ranks ---------------------------------------------------------------------------------------------------
def test_two_ranks(fba):
    synth, sc = _scene(fba, "fisheye", opp=9, n_control=5)
    pk = ir.pack_scene(fba.capi, synth, sc, 5)
    with _ctx(fba, pk, "fisheye", 5) as single:
        xyz, q, st, bad = single.intersect()
        ray, rst = single.image_rays()
    ranks = [_ctx(fba, pk, "fisheye", 5, rank=r, world=2) for r in range(2)]
    try:
        outs = [c.intersect() for c in ranks]
        rays = [c.image_rays() for c in ranks]
    finally:
        for c in ranks:
            c.close()
    owner, _ = fba.capi.partition(pk, 2)
    for r in range(2):
        assert (outs[r][0][owner != r] == 0).all() and (outs[r][1][owner != r] == 0).all()
        assert (outs[r][0][owner == r] != 0).any()
    assert np.array_equal(outs[0][0] + outs[1][0], xyz)              # bitwise: a point's rays all live on its owner
    assert np.array_equal(outs[0][1] + outs[1][1], q) and np.array_equal(outs[0][2] + outs[1][2], st)
    assert outs[0][3] + outs[1][3] == bad
    assert np.array_equal(rays[0][0] + rays[1][0], ray) and np.array_equal(rays[0][1] + rays[1][1], rst)
    assert ((np.abs(rays[0][0]).sum(1) > 0) ^ (np.abs(rays[1][0]).sum(1) > 0)).all()


# ---- 10. end to end -------------------------------------------------------------------------------------------------
def test_adjust_from_intersected_points(fba, tmp_path):
    """every tie0 displaced by (1500, -1500, 800): adjust(intersect=True) reaches the xhat that adjust reaches from the
    scene's own X0 -- sum |dxhat| <= 2 x Threshold_Value (each run's last correction is below the threshold, and
    Gauss-Newton's remaining error is below its last step).  Control points fix the datum (a free network's datum
    follows the iterates).  Confirmed first on the CPU: the oracle started from the restatement's intersected points
    converges in the same number of passes as from X0."""
    from fba_amd import bundle, report, synth
    sc = synth.generate(12, 40, seed=3, obs_per_point=9, n_control=5)
    moved = dict(sc, X0=np.where(sc["control"][:, None], sc["X0"], sc["X0"] + SHIFT))
    f_own = synth.write_folder(sc, os.path.join(str(tmp_path), "own"))
    f_mov = synth.write_folder(moved, os.path.join(str(tmp_path), "moved"))
    own = bundle.adjust(fba.load_folder(f_own), covariance=False)
    data = fba.load_folder(f_mov)
    res = bundle.adjust(data, covariance=False, intersect=True)
    cap, thr = int(data.settings["Iteration_Cap"]), float(data.settings["threshold"])
    assert res.iterations < cap and res.deltasum[-1] <= thr and own.deltasum[-1] <= thr
    assert res.isect_status.shape == (data.numtie,) and (res.isect_status == 0).all()
    shift = np.abs(res.isect_xyz - np.array([data.CNT[t] for t in data.TIE]) + SHIFT).max()
    diff = float(np.abs(res.xhat - own.xhat).sum())
    print(f"end to end: {res.iterations} passes (own X0: {own.iterations}); intersected points within {shift:.1f} units of "
          f"the undisplaced .cnt values; sum |xhat - xhat_own| {diff:.2e} (bar {2 * thr:.1e})")
    assert diff <= 2 * thr
    assert bundle.main(f_mov, intersect=True) == 0
    name = os.path.splitext(data.settings["Output_Filename"])[0]
    names, rays, xyz, _, _, words = report.read_fwd(os.path.join(f_mov, name + ".fwd"))
    assert len(names) == data.numtie and names == list(data.TIE) and set(words) == {"OK"}
    assert np.allclose(xyz, res.isect_xyz, rtol=0, atol=1e-9)
