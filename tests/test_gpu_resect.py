"""GPU: space resection -- fba_resect (csrc/fba_resect.hip) against fba_resect_host and the numpy restatement
(tests/resect_ref.py), its statuses and contract, and adjust(..., resect="control", intersect=True) end to end.

Scenes are synth scenes packed without files (intersect_ref.pack_scene): 12 images and 40 points, 12 images and 70
points of which 30 are control, 4 images and 200 points; the restatement of each is computed once per module.

Bars, none from a device run (tests/test_resect_host.py's):
  exact    noise 0, true EOP / IOP, the points at X_true: linear |C - C_true| <= 1e-8 units, |M - M_true| <= 1e-11;
           refined |C - C_true| <= 1e-8, RMS <= 1e-8 px
  noisy    linear C against the restatement and against fba_resect_host to max(1e-9 x the mean distance, 100 x the
           spread of the restatement's two ways), M likewise with the distance left out; the ratio to 1e-10; refined C
           to 100 x refine_tol x the distance, |M - M_ref| <= 100 x refine_tol; RMS final <= RMS linear
  everything else is bitwise.
Measured on the device: DESIGN.md 6h, profiles/resect_gpu_errors.log.
"""
import os

import numpy as np
import pytest

import intersect_ref as ir
import resect_ref as rr

pytestmark = pytest.mark.gpu

_CACHE = {}
EOP_FLAGS = ("Estimate_Xc", "Estimate_Yc", "Estimate_Zc", "Estimate_w", "Estimate_p", "Estimate_k")


def _theta(typ):
    return 60.0 if typ in ("pinhole", "orthographic") else 80.0


def _scene(typ="fisheye", noise=0.3, n_img=12, n_pts=40, opp=9, **kw):
    from fba_amd import synth
    key = (typ, noise, n_img, n_pts, opp, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = synth.generate(n_img, n_pts, seed=3, obs_per_point=opp, noise=noise, typ=typ,
                                     max_theta_deg=_theta(typ), **kw)
    return synth, _CACHE[key]


def _ctx(fba, pk, typ, nk=5, est_iop=True, off=(), **kw):
    s = ir.settings_dict(typ, nk)
    if not est_iop:
        for k in ("Estimate_xp", "Estimate_yp", "Estimate_c", "Estimate_radial", "Estimate_decent"):
            s[k] = 0
    for k in off:
        s[k] = 0
    return fba.capi.Context(pk, fba.capi.make_settings(s), **kw)


CASES = {
    **{t: dict(typ=t) for t in ir.TYPES},
    "rig": dict(n_cam=2, cam_layout="alternate"),
    "control": dict(n_pts=70, n_control=30, use="control"),
    "wide": dict(n_img=4, n_pts=200, opp=4),
}


def _case(fba, name):
    kw = dict(CASES[name])
    typ, use = kw.pop("typ", "fisheye"), kw.pop("use", "all")
    synth, sc = _scene(typ, **kw)
    return synth, sc, typ, use, ir.pack_scene(fba.capi, synth, sc, 5)


def _host_inputs(fba, pk, typ, use, nk=5):
    """per image (xyz, rays, c, ydir) from fba_unproject_host, PHO order"""
    iop, ydir = pk.iop0.reshape(pk.n_cam, 5 + nk), pk.cam_info.reshape(-1, 5)[:, 0]
    X = rr.object_points(pk)
    out = []
    for e in range(pk.n_img):
        rows = np.nonzero((pk.img == e) & ((pk.tie < 0) | (use == "all")))[0]
        k = int(pk.cam[rows[0]])
        ct = np.concatenate([iop[k, :3], [ydir[k]], iop[k, 3 + nk:], iop[k, 3:3 + nk]])
        ray, st = fba.capi.unproject_host(typ, pk.xy.reshape(-1, 2)[rows], ct)
        out.append((X[rows], ray, st, ct[2], ct[3]))
    return out


def _restate(pk, typ, use, name):
    """(the restatement by eigh with the refinement, by the SVD of the reversed rows: linear only), cached"""
    key = ("ref", name)
    if key not in _CACHE:
        pb = ir.Problem(pk, typ, 5)
        _CACHE[key] = (rr.resect_all(pk, pb, use), rr.resect_all(pk, pb, use, refine_iters=0, method="svd"))
    return _CACHE[key]


# ---- 1. device against the truth, fba_resect_host and the restatement --------------------------------------------------
@pytest.mark.parametrize("typ", ir.TYPES)
def test_exact_at_the_truth(fba, typ):
    synth, sc = _scene(typ, noise=0.0)
    pk = ir.pack_scene(fba.capi, synth, dict(sc, X0=sc["X_true"]), 5, truth=True)
    with _ctx(fba, pk, typ) as ctx:
        lin, ql, sl, bl = ctx.resect(use="all", refine_iters=0)
        fin, qf, sf, bf = ctx.resect(use="all")
    M_true = ir.rot(sc["ang_true"][:, 0], sc["ang_true"][:, 1], sc["ang_true"][:, 2])
    M_lin = ir.rot(lin[:, 3], lin[:, 4], lin[:, 5])
    eC, eM = np.abs(lin[:, :3] - sc["C_true"]).max(), np.abs(M_lin - M_true).max()
    fC = np.abs(fin[:, :3] - sc["C_true"]).max()
    print(f"exact {typ}: linear |C - C_true| {eC:.2e} (bar 1e-8), |M - M_true| {eM:.2e} (bar 1e-11); refined "
          f"|C - C_true| {fC:.2e} (bar 1e-8), RMS {qf[:, 3].max():.2e} px (bar 1e-8); points {int(ql[:, 0].min())} .. "
          f"{int(ql[:, 0].max())}; ratio >= {ql[:, 1].min():.1e}")
    assert bl == 0 and (sl == 0).all() and np.isin(sf, (0, 3)).all() and np.array_equal(ql[:, 2], ql[:, 3])
    assert np.isin(ql[:, 4], (0.0, 1.0)).all() and (ql[:, 4] == 0.0).all()       # synth's scenes have W < 0
    assert eC <= 1e-8 and eM <= 1e-11
    assert fC <= 1e-8 and qf[:, 3].max() <= 1e-8


@pytest.mark.parametrize("name", sorted(CASES))
def test_noisy_against_host_and_restatement(fba, name):
    synth, sc, typ, use, pk = _case(fba, name)
    ref, alt = _restate(pk, typ, use, name)
    host = _host_inputs(fba, pk, typ, use)
    with _ctx(fba, pk, typ) as ctx:
        lin, ql, sl, bl = ctx.resect(use=use, refine_iters=0)
        fin, qf, sf, bf = ctx.resect(use=use)
    assert bl == 0 and bf == 0 and (sl == 0).all() and (sf == 0).all()
    if name == "wide":
        assert ql[:, 0].min() > 128                                   # the 64 lanes make more than two passes
    if name == "control":
        assert 14 <= ql[:, 0].min() and ql[:, 0].max() <= 30
    worst = np.zeros(8)
    for e, (a, b) in enumerate(zip(ref, alt)):
        assert a["status"] == 0 and a["rms_fin"] <= a["rms_lin"]      # the restatement alone
        assert ql[e, 0] == qf[e, 0] == a["n"]
        sC, sM = np.abs(a["C_lin"] - b["C_lin"]).max(), np.abs(a["M_lin"] - b["M_lin"]).max()
        barC, barM = max(1e-9 * a["dist"], 100 * sC), max(1e-9, 100 * sM)
        X, ray, rst, c, ydir = host[e]
        hl, hql, hsl = fba.capi.resect_host(typ, X, ray, c, ydir, ray_status=rst, refine_iters=0)
        hf, hqf, hsf = fba.capi.resect_host(typ, X, ray, c, ydir, ray_status=rst)
        assert hsl == 0 and hsf == 0 and hql[0] == a["n"]
        M_dev, M_fin = ir.rot(*lin[e, 3:]), ir.rot(*fin[e, 3:])
        eC, eM = np.abs(lin[e, :3] - a["C_lin"]).max(), np.abs(M_dev - a["M_lin"]).max()
        hC, hM = np.abs(lin[e, :3] - hl[:3]).max(), np.abs(M_dev - ir.rot(*hl[3:])).max()
        assert eC <= barC and hC <= barC, (e, eC, hC, barC)
        assert eM <= barM and hM <= barM, (e, eM, hM, barM)
        assert abs(ql[e, 1] - a["ratio"]) <= 1e-10 and abs(ql[e, 1] - hql[1]) <= 1e-10
        assert abs(ql[e, 2] - a["rms_lin"]) <= 1e-6 and ql[e, 3] == ql[e, 2]
        fC, fM = np.abs(fin[e, :3] - a["eop"][:3]).max(), np.abs(M_fin - ir.rot(*a["eop"][3:])).max()
        gC, gM = np.abs(fin[e, :3] - hf[:3]).max(), np.abs(M_fin - ir.rot(*hf[3:])).max()
        assert fC <= 100 * 1e-10 * a["dist"] and gC <= 100 * 1e-10 * a["dist"], (e, fC, gC)
        assert fM <= 100 * 1e-10 and gM <= 100 * 1e-10, (e, fM, gM)
        assert qf[e, 3] <= qf[e, 2] and abs(qf[e, 3] - a["rms_fin"]) <= 1e-6
        assert qf[e, 4] == a["front"] == 0.0
        worst = np.maximum(worst, [eC / barC, eM / barM, max(hC / barC, hM / barM), fC, fM, max(gC, gM), a["iters"],
                                   np.abs(a["eop"][:3] - sc["C_true"][e]).max()])
    print(f"noisy {name}: linear |C - ref| / bar {worst[0]:.2e}, |M - ref| / bar {worst[1]:.2e}, against the host / bar "
          f"{worst[2]:.2e}; refined |C - ref| {worst[3]:.2e}, |M - ref| {worst[4]:.2e}, against the host {worst[5]:.2e}; "
          f"<= {int(worst[6])} passes; points {int(ql[:, 0].min())} .. {int(ql[:, 0].max())}; RMS {qf[:, 2].max():.3f} -> "
          f"{qf[:, 3].max():.3f} px; within {worst[7]:.1f} units of the truth")


# ---- 3. statuses -------------------------------------------------------------------------------------------------------
def test_statuses(fba):
    typ = "orthographic"
    synth, sc = _scene(typ, n_pts=70, n_control=30)
    pid, img = sc["pid"], sc["img"]
    ctl = sc["control"][pid]
    keep = np.ones(len(pid), bool)
    rows0 = np.nonzero(ctl & (img == 0))[0]
    keep[rows0[5:]] = False                                          # image 0: 5 control points -> FEW
    xy = sc["xy"].copy()
    r2 = np.nonzero(ctl & (img == 2))[0][0]
    cam0 = synth.camera_params(0)
    xy[r2] = (cam0[0] + 0.5 + 1.2 * (cam0[2] + 1.0), cam0[1] + 0.5)  # image 2: q = 1.2 > 1 in one control ray
    pk0 = ir.pack_scene(fba.capi, synth, dict(sc, xy=xy), 5, keep=keep)
    xyz = pk0.xyz_fixed.reshape(-1, 3).copy()
    rows1 = np.nonzero((pk0.tie < 0) & (pk0.img == 1))[0]
    xyz[rows1, 2] = 100.0 + 0.01 * xyz[rows1, 0]                     # image 1: its control points in one plane -> WEAK
    pk = fba.capi.PackedProblem(pk0.xy, pk0.img, pk0.cam, pk0.tie, xyz, pk0.eop0, pk0.iop0, pk0.cam_info, pk0.tie0,
                                pk0.n_img, pk0.n_cam, pk0.n_tie)
    n2 = int(((pk.tie < 0) & (pk.img == 2)).sum())
    with _ctx(fba, pk, typ) as ctx:
        x0 = ctx.get_xhat()
        eop, q, st, bad = ctx.resect(write_xhat=True)
        x1 = ctx.get_xhat()
    assert st[0] == 1 and st[1] == 2 and st[2] == 0 and set(st[3:]) <= {0, 3}
    assert bad == int((st != 0).sum()) and bad >= 2
    assert list(q[0]) == [5, 0, 0, 0, 0] and q[1, 0] == len(rows1) and q[1, 1] <= 1e-12 and not q[1, 2:].any()
    assert q[2, 0] == n2 - 1                                          # the DOMAIN ray is left out
    e0, e1 = x0[: 6 * pk.n_img].reshape(-1, 6), x1[: 6 * pk.n_img].reshape(-1, 6)
    assert np.array_equal(eop[:2], e0[:2])                            # FEW, WEAK: the current values
    assert np.array_equal(e1[:2], e0[:2])                             # ... kept bit for bit
    assert np.array_equal(e1[2:], eop[2:]) and (e1[2:] != e0[2:]).any()
    assert np.array_equal(x1[6 * pk.n_img:], x0[6 * pk.n_img:])


# ---- 4. contract -------------------------------------------------------------------------------------------------------
def _contract_problem(fba):
    synth, sc = _scene("fisheye", n_pts=70, n_control=30)
    return ir.pack_scene(fba.capi, synth, sc, 5)


def test_contract_read_only(fba):
    pk = _contract_problem(fba)
    live = fba.capi.live_allocations()
    with _ctx(fba, pk, "fisheye", est_iop=False) as ctx, _ctx(fba, pk, "fisheye", est_iop=False) as plain:
        x0 = ctx.get_xhat()
        for use in ("control", "all"):
            a, b = ctx.resect(use=use), ctx.resect(use=use)
            for u, v in zip(a[:3], b[:3]):
                assert np.array_equal(u, v)
            assert a[3] == b[3] == 0
        assert np.array_equal(ctx.get_xhat(), x0)
        ctx.accumulate()
        ctx.resect()                                                 # between the two halves: nothing moves either
        d1 = ctx.solve_update()
        d0 = plain.step()
        assert d1 == d0 and np.array_equal(ctx.get_xhat(), plain.get_xhat())
        ctx.accumulate()
        ctx.solve_update_async()
        with pytest.raises(fba.capi.FBAError) as ei:                 # not between solve_update_async and solve_finish
            ctx.resect()
        assert ei.value.code == 1
        ctx.solve_finish()
        plain.step()
        assert np.array_equal(ctx.get_xhat(), plain.get_xhat())
    assert fba.capi.live_allocations() == live
    # any flag set without write_xhat; write_xhat with a fixed exterior orientation is the user's: code 5
    with _ctx(fba, pk, "fisheye", est_iop=False, off=("Estimate_k",)) as fixed:
        assert fixed.resect()[3] == 0
        with pytest.raises(fba.capi.FBAError) as ei:
            fixed.resect(write_xhat=True)
        assert ei.value.code == 5
    rank = _ctx(fba, pk, "fisheye", rank=0, world=2)                 # an image's observations are spread over the ranks
    try:
        with pytest.raises(fba.capi.FBAError) as ei:
            rank.resect()
        assert ei.value.code == 5
    finally:
        rank.close()
    assert fba.capi.live_allocations() == live


def test_contract_write_xhat(fba):
    pk = _contract_problem(fba)
    with _ctx(fba, pk, "fisheye", est_iop=False) as ctx:
        ctx.step()
        ctx.residuals()
        x0 = ctx.get_xhat()
        eop, q, st, bad = ctx.resect(write_xhat=True)
        with pytest.raises(fba.capi.FBAError) as ei:
            ctx.residuals()
        assert ei.value.code == 1
        x1 = ctx.get_xhat()
        ni = pk.n_img
        assert np.isin(st, (0, 3)).all()
        assert np.array_equal(x1[: 6 * ni].reshape(-1, 6), eop) and np.array_equal(x1[6 * ni:], x0[6 * ni:])
        assert (x1[: 6 * ni] != x0[: 6 * ni]).any()
        assert np.isfinite(ctx.step())
        ctx.residuals()


def test_contract_weights_loss_priors(fba):
    pk = _contract_problem(fba)
    with _ctx(fba, pk, "fisheye", est_iop=False) as plain:
        want = plain.resect(use="all")
    rng = np.random.default_rng(5)
    pri = (np.array([0, 7]), np.array([100.0, 0.1]), np.array([1.0, 0.01]))
    with _ctx(fba, pk, "fisheye", est_iop=False, priors=pri) as ctx:
        ctx.set_weights(rng.uniform(0.5, 2.0, 2 * pk.n_pts))
        ctx.set_loss("huber")
        ctx.set_damping(1e-3)
        got = ctx.resect(use="all")
    for u, v in zip(want, got):
        assert np.array_equal(u, v)


def test_timing_slot(fba):
    pk = _contract_problem(fba)
    with _ctx(fba, pk, "fisheye") as ctx:
        ctx.set_timing(True)
        ctx.resect()
        ms = ctx.timings()
    assert ms[7] > 0 and not ms[:7].any()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
def test_adjust_from_resected_images(fba, tmp_path):
    """every .ext centre displaced by (800, -600, 500), every angle by (0.3, -0.2, 1.0) rad, every tie X0 by
    (1500, -1500, 800): adjust(resect="control", intersect=True) reaches the xhat that adjust reaches from the scene's
    own start values -- sum |dxhat| <= 2 x Threshold_Value (each run's last correction is below the threshold, and
    Gauss-Newton's remaining error is below its last step).  Confirmed first on the CPU: the oracle started from the
    restatement's resected and intersected values converges to the oracle's own result within the bar."""
    from fba_amd import bundle, report, synth
    sc = synth.generate(12, 70, seed=3, obs_per_point=9, n_control=30)
    moved = dict(sc, C0=sc["C0"] + np.array([800.0, -600.0, 500.0]), ang0=sc["ang0"] + np.array([0.3, -0.2, 1.0]),
                 X0=np.where(sc["control"][:, None], sc["X0"], sc["X0"] + np.array([1500.0, -1500.0, 800.0])))
    f_own = synth.write_folder(sc, os.path.join(str(tmp_path), "own"))
    f_mov = synth.write_folder(moved, os.path.join(str(tmp_path), "moved"))
    own = bundle.adjust(fba.load_folder(f_own), covariance=False)
    data = fba.load_folder(f_mov)
    res = bundle.adjust(data, covariance=False, resect="control", intersect=True)
    cap, thr = int(data.settings["Iteration_Cap"]), float(data.settings["threshold"])
    assert res.iterations < cap and res.deltasum[-1] <= thr and own.deltasum[-1] <= thr
    assert res.resect_status.shape == (data.numImg,) and (res.resect_status == 0).all()
    assert (res.isect_status == 0).all()
    off = np.abs(res.resect_eop[:, :3] - sc["C_true"]).max()
    diff = float(np.abs(res.xhat - own.xhat).sum())
    print(f"end to end: {res.iterations} passes (own start values: {own.iterations}); resected centres within {off:.1f} "
          f"units of the truth at {res.resect_quality[:, 3].max():.2f} px; sum |xhat - xhat_own| {diff:.2e} (bar {2 * thr:.1e})")
    assert diff <= 2 * thr
    assert bundle.main(f_mov, resect="control", intersect=True) == 0
    name = os.path.splitext(data.settings["Output_Filename"])[0]
    names, used, eop, shift, qual, words = report.read_rsc(os.path.join(f_mov, name + ".rsc"))
    assert len(names) == data.numImg and names == [r[0] for r in data.EXT[: data.numImg]] and set(words) == {"OK"}
    assert np.allclose(eop, res.resect_eop, rtol=0, atol=1e-9) and np.array_equal(used, res.resect_quality[:, 0])
    assert np.abs(shift[:, :3] + np.array([800.0, -600.0, 500.0])).max() <= 100.0
