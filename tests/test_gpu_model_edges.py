"""GPU: obs_model -- the one function every linearising kernel inlines -- over the full fish-eye field.

(a)-(c) read tests/golden/model_edges.npz only (numbers of a 50-digit mpmath model differentiated numerically,
tests/golden/make_model_edges.py; tests/test_model_edges_host.py holds the NumPy oracle to a tenth of the bars
below on the same samples and ties that model to the reference's own text).  One image and one camera per sample.

(a) test_build_awg_geometry[type]   fba_build_awg (k_linearize) at nK = 5, all Estimate_* on, at off-axis angles
    1e-9 rad .. 179 deg (W > 0 beyond 90 deg: the reference's atan, not atan2), small and large rotations.
(b) test_build_awg_distortion[nk]   every NK instantiation's camera columns (xp yp c K_j P) and dist_scaling at image
    points at, 1e-6 / 1e-3 px from and far from the principal point, at r = rmax and 1.2 rmax; what is exactly 0 at
    the principal point in the reference is exactly 0.
    Bars of (a) and (b) -- the 1e-12 the project holds inside 1 .. 80 deg (test_gpu_parity.
    test_buildawg_matches_reference_text), made condition-aware; 10 x what the oracle is held to on the CPU:
      position / rotation / tie entries: |d| <= 1e-12 x the largest reference entry of that group in that row;
      projected value w + x: |d| <= 1e-12 c;
      camera columns: |d| <= 1e-12 x max(|entry|, the column's largest entry over the sample set);
      G: 1e-14 of the image block's largest entry; dist_scaling 1e-14 relative.
    Measured on an MI355X (max over each set, in units of what each bar scales; position, rotation, tie, camera,
    f / c; the oracle's figures on the CPU are in tests/test_model_edges_host.py):
      geo_fisheye        5.5e-16 4.7e-16 5.5e-16 4.3e-16 6.7e-16   (position worst at 90.01 deg)
      geo_pinhole        3.4e-15 3.3e-15 3.4e-15 1.4e-15 7.0e-14   (all five worst at 91 deg)
      geo_equisolid      6.8e-16 5.4e-16 6.8e-16 1.2e-15 6.5e-16
      geo_orthographic   4.7e-15 1.6e-15 4.7e-15 3.5e-16 5.9e-16   (position, rotation, tie worst at 90.1 deg)
      geo_stereographic  9.7e-16 7.0e-16 9.7e-16 4.8e-16 7.1e-16
      dist_nk1 .. dist_nk8: camera 2.2e-16 4.0e-16 7.3e-16 6.0e-16 2.2e-16 2.2e-16 1.5e-15 1.5e-15; position / rotation /
      tie <= 4.3e-16, f / c <= 4.6e-16
      G <= 5.5e-19 of the block's largest entry, dist_scaling <= 2.0e-15 relative, in every set
(c) test_cost_forward_only[type]    k_cost's copy of the forward model on the contexts of (a): fba_cost against
    sum p w^2 of the fixture's projected values (p = 1), 1e-12 relative.
      Measured: fisheye 0, pinhole 2.2e-16, equisolid 1.3e-16, orthographic 0, stereographic 0.

Mutation check (scratch builds, never committed): obs_model with atan2(R, -W) for atan(R / W) fails (a), (b) and (c) for
every type but pinhole, (d) for all four types, (e) and (f); with sR = gt tR / R (the "- s" dropped) it fails (a) and
(b) for every type but pinhole, (d) for all four types, (e) and (f).

(d)-(f) run the hot path (k_lin_reduce, the general-point kernels, the reliability rows) in the band the other
scenes never enter: synth.generate(12, 120, typ=T, max_theta_deg=89.5, obs_per_point=4, spacing=4000, n_wide=40,
wide_min_obs=6) at nK = 5 has ~940 observations, of which (fisheye) ~100 lie beyond 80 deg, ~30 beyond 85 deg, the
largest beyond 89 deg.  Seeds: of 17..22 the one at which the dense oracle's two solver variants (explicit
inverse, LU) agree best in deltasum, with no deltasum within 1.25x of Threshold_Value (the rule of
test_gpu_lr_early.py:35-37; SEEDS below, figures beside them).

(d) test_wide_field_every_pass[type]  fisheye, equisolid, orthographic, stereographic: the scene still has >= 40
    observations beyond 80 deg, >= 5 beyond 85 deg and one beyond 88.5 deg; then test_gpu_lr_queue._check_every_pass
    against the dense oracle -- its own bars: xhat per group and per element at max(1e-9, 20 x the oracle's spread
    of that pass), deltasum at 1e-9 of the first, the iteration count, adjust() bit-equal to the stepped loop.
(e) test_near_axis_every_pass         the fisheye scene of (d) with eight tie points put on the optical axis of one of
    their images AT ITS INITIAL VALUES (X = C0 + M(ang0)' (0, 0, -d)) and started 0.01 units from there (generate()'s
    start noise of 10 units is 3e-3 .. 7e-3 rad at this scene's depths of 1500 .. 3000 units, so those points get a
    thousandth of it): their observations in that image are linearised ~1e-5 rad off-axis in the first pass
    (asserted), where sR = (gt tR - s) / R is a difference of nearly equal numbers, and a few 1e-3 rad off-axis
    once the image's angles (started 0.1 deg off) have moved.  Checked as (d).
(f) test_wide_field_general_and_reliability  the fisheye scene of (d) with n_dup = 12 (general points in the band):
    the adjustment against the dense oracle as test_gpu_general.test_adjust_general holds it, redundancy numbers and
    w-statistics with test_gpu_reliability's helper and bars.
"""
import numpy as np
import pytest

from test_model_edges_host import EdgeSet, TYPES, check_awg, edges  # noqa: F401  (edges: the fixture's fixture)

pytestmark = pytest.mark.gpu

GPU_BAR = 1e-12
WIDE_TYPES = ["fisheye", "equisolid", "orthographic", "stereographic"]
WIDE = dict(n_img=12, n_tie=120, max_theta_deg=89.5, obs_per_point=4, spacing=4000.0, n_wide=40, wide_min_obs=6)
# type -> seed.  The oracle's inverse-vs-LU deltasum spread (of the first deltasum) at seeds 17..22, on two hosts
# (it moves with the host's BLAS threading: the explicit inverse of main.m:432 is that sensitive on these
# scenes); the seed taken is the one whose larger figure is smallest:
#   fisheye        5.9e-10  2.8e-10* 2.1e-9 (a deltasum 1.08x the threshold)  3.2e-9  1.6e-9  6.1e-10
#                  4.4e-10  2.2e-10* 8.5e-10                                  1.4e-9  8.0e-10 8.5e-11
#   equisolid      2.9e-9   8.9e-10  3.2e-9  7.7e-10  4.4e-10* 2.5e-9
#                  1.4e-9   1.5e-9   6.2e-10 9.5e-10  8.1e-10* 3.5e-10
#   orthographic   1.9e-9*  6.6e-9   8.7e-9  2.1e-8   1.1e-8 (a deltasum 1.11x the threshold)  3.6e-9
#                  7.2e-10* 4.8e-9   6.7e-8  1.8e-8   3.2e-10                                  9.1e-9
#   stereographic  1.8e-10* 3.5e-9   7.0e-10 3.4e-10  2.6e-10  8.3e-10
#                  1.6e-10* 1.4e-9   1.0e-10 3.5e-10  3.5e-10  7.6e-10
# (orthographic: sin(t) is flat towards 90 deg, the band this scene is made of.)  Measured on an MI355X, deltasum
# error of the worst pass (bar 1e-9) beside the oracle's own spread on that host: fisheye 2.2e-10 / 2.2e-10,
# equisolid 8.1e-10 / 8.1e-10, orthographic 7.6e-10 / 7.2e-10, stereographic 1.6e-10 / 1.6e-10, near axis 6.6e-10 /
# 6.6e-10, general 4.9e-10 / 4.9e-10 -- the device lands on the oracle's LU variant, and every xhat group of every pass
# within max(1e-9, 20 x the spread).
SEEDS = {"fisheye": 18, "equisolid": 21, "orthographic": 17, "stereographic": 17}
NEAR_AXIS_POINTS = 8


# ---- (a) - (c) ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts(fba):
    """one context per sample set, made on first use and shared by (a) and (c)"""
    made = {}

    def get(es):
        if es.name not in made:
            idx = np.arange(es.n)
            packed = fba.capi.PackedProblem(es.xy, idx, idx, idx, es.xyz, es.eop, es.iop, es.cam_info, es.xyz, es.n,
                                            es.n, es.n)
            made[es.name] = fba.capi.Context(packed, fba.capi.make_settings(es.settings))
        return made[es.name]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("typ", TYPES)
def test_build_awg_geometry(edges, contexts, typ):  # noqa: F811
    es = EdgeSet(edges, "geo_" + typ)
    A, w, G, ds = contexts(es).build_awg(es.xhat)
    check_awg(es, np.asarray(A), w, np.asarray(G), np.asarray(ds), GPU_BAR)


@pytest.mark.parametrize("nk", range(1, 9))
def test_build_awg_distortion(edges, contexts, nk):  # noqa: F811
    es = EdgeSet(edges, f"dist_nk{nk}")
    A, w, G, ds = contexts(es).build_awg(es.xhat)
    check_awg(es, np.asarray(A), w, np.asarray(G), np.asarray(ds), GPU_BAR)


@pytest.mark.parametrize("typ", TYPES)
def test_cost_forward_only(edges, contexts, typ):  # noqa: F811
    es = EdgeSet(edges, "geo_" + typ)
    ctx = contexts(es)
    ctx.set_xhat(es.xhat)
    total, image, prior = ctx.cost()
    ref = es.cost()
    print(f"model edges cost {typ}: device {image:.17g} reference {ref:.17g} relative {abs(image - ref) / ref:.1e}")
    assert prior == 0.0 and total == image
    assert abs(image - ref) <= 1e-12 * ref


# ---- (d) - (f) ------------------------------------------------------------------------------------------------
def off_axis_deg(sc, C, ang, X):
    """off-axis angle of every observation of scene `sc` at image positions C, angles ang and points X"""
    from fba_amd import synth
    M = synth._rot(ang[:, 0], ang[:, 1], ang[:, 2])[sc["img"]]
    d = X[sc["pid"]] - C[sc["img"]]
    UVW = np.einsum("nij,nj->ni", M, d)
    return np.degrees(np.arctan2(np.hypot(UVW[:, 0], UVW[:, 1]), -UVW[:, 2]))


def wide_scene(typ, **kw):
    from fba_amd import synth
    return synth.generate(WIDE["n_img"], WIDE["n_tie"], seed=SEEDS[typ], typ=typ,
                          **{k: v for k, v in WIDE.items() if k not in ("n_img", "n_tie")}, **kw)


def near_axis_scene():
    """the fisheye wide scene with NEAR_AXIS_POINTS tie points moved onto the optical axis of the initial pose of
    one of their images, their observations regenerated (synth._project at the true poses, fresh N(0, 0.3) noise);
    returns the scene and the (observation index) of each such point in that image"""
    from fba_amd import synth
    sc = dict(wide_scene("fisheye"))
    sc["X_true"], sc["X0"], sc["xy"] = sc["X_true"].copy(), sc["X0"].copy(), sc["xy"].copy()
    rng = np.random.default_rng(SEEDS["fisheye"])
    xp, yp, c = synth.camera_params(0)
    M0 = synth._rot(sc["ang0"][:, 0], sc["ang0"][:, 1], sc["ang0"][:, 2])
    Mt = synth._rot(sc["ang_true"][:, 0], sc["ang_true"][:, 1], sc["ang_true"][:, 2])
    theta = off_axis_deg(sc, sc["C_true"], sc["ang_true"], sc["X_true"])
    moved = []
    for o in np.argsort(theta):  # the observations nearest their image's axis first: the shortest moves
        j, e = int(sc["pid"][o]), int(sc["img"][o])
        if len(moved) == NEAR_AXIS_POINTS:
            break
        if j in [m[0] for m in moved]:
            continue
        depth = -(Mt[e] @ (sc["X_true"][j] - sc["C_true"][e]))[2]
        Xn = sc["C0"][e] + M0[e].T @ np.array([0.0, 0.0, -depth])
        obs = np.nonzero(sc["pid"] == j)[0]
        UVW = np.einsum("nij,nj->ni", Mt[sc["img"][obs]], Xn - sc["C_true"][sc["img"][obs]])
        x, y = synth._project("fisheye", UVW[:, 0], UVW[:, 1], UVW[:, 2], c, xp, yp, synth.K0, synth.P0)
        seen = (UVW[:, 2] < 0) & (-UVW[:, 2] >= np.cos(np.radians(WIDE["max_theta_deg"])) * np.linalg.norm(UVW, axis=1))
        seen &= (x > 1) & (x < 2047) & (y > 1) & (y < 2047)
        if not seen.all():  # the moved point would leave one of its images: take the next one
            continue
        # generate()'s start noise of 10 units is 3e-3 .. 7e-3 rad at these depths (1500 .. 3000 units); a
        # thousandth of it (10 mm with the scene read in metres) puts the start ~1e-5 rad off-axis
        sc["X0"][j] = Xn + 1e-3 * (sc["X0"][j] - sc["X_true"][j])
        sc["X_true"][j] = Xn
        sc["xy"][obs] = np.stack([x, y], -1) + rng.normal(0, 0.3, (len(obs), 2))
        moved.append((j, int(o)))
    assert len(moved) == NEAR_AXIS_POINTS
    return sc, np.array([o for _, o in moved])


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("model_edges"), "oracle": {}}


def _folder(work, name, sc):
    from fba_amd import synth
    return synth.write_folder(sc, str(work["root"] / name), nk=5)


def _every_pass(fba, oracle, folder, tag):
    from test_gpu_block_shapes import _errors, _solve_lu
    from test_gpu_lr_queue import _check_every_pass
    od = oracle.load_folder(folder)
    ro, lu = oracle.adjust(od), oracle.adjust(od, solver=_solve_lu)
    assert lu.iterations == ro.iterations
    ref = dict(ro=ro, lu=lu, spread=[_errors(lu.xhat_hist[i], ro.xhat_hist[i], ro) for i in range(ro.iterations + 1)],
               spread_dsum=np.abs(np.array(lu.deltasum) - np.array(ro.deltasum)) / ro.deltasum[0])
    _check_every_pass(fba, fba.load_folder(folder), ref, None, tag)


@pytest.mark.parametrize("typ", WIDE_TYPES)
def test_wide_field_every_pass(fba, oracle, work, typ):
    sc = wide_scene(typ)
    th = off_axis_deg(sc, sc["C_true"], sc["ang_true"], sc["X_true"])
    print(f"wide field {typ}: {len(th)} observations, {(th > 80).sum()} beyond 80 deg, {(th > 85).sum()} beyond 85 deg, "
          f"max {th.max():.2f} deg")
    assert (th > 80).sum() >= 40 and (th > 85).sum() >= 5 and th.max() > 88.5
    _every_pass(fba, oracle, _folder(work, typ, sc), f"wide field {typ}")


def test_near_axis_every_pass(fba, oracle, work):
    sc, obs = near_axis_scene()
    start = np.radians(off_axis_deg(sc, sc["C0"], sc["ang0"], sc["X0"]))[obs]
    print("near axis: off-axis angle of the moved points' observations at the initial values (rad):",
          " ".join(f"{a:.1e}" for a in start))
    # 0.01 units per coordinate over a depth of 1500 .. 3000 units
    assert (start > 0).all() and start.max() < 3e-5 and 1e-6 < np.median(start) < 2e-5
    _every_pass(fba, oracle, _folder(work, "near_axis", sc), "near axis")


def test_wide_field_general_and_reliability(fba, oracle, work):
    from conftest import group_rel_err
    from test_gpu_general import _general_count
    from test_gpu_reliability import _check, _reference
    sc = wide_scene("fisheye", n_dup=12)
    th = off_axis_deg(sc, sc["C_true"], sc["ang_true"], sc["X_true"])
    folder = _folder(work, "general", sc)
    od = oracle.load_folder(folder)
    dup_pts = set(sc["pid"][-12:].tolist())  # generate() appends the repeated measurements
    th_gen = th[np.isin(sc["pid"], list(dup_pts))]
    print(f"wide field general: {_general_count(od)} general points, their observations up to {th_gen.max():.2f} deg, "
          f"{(th_gen > 80).sum()} beyond 80 deg")
    assert _general_count(od) == len(dup_pts) >= 10 and (th_gen > 80).sum() >= 1
    ro = oracle.adjust(od)
    res = fba.adjust(fba.load_folder(folder), reliability=True)
    # test_gpu_general.test_adjust_general's comparison, at its bars
    assert res.iterations == ro.iterations
    err = group_rel_err(res.xhat, ro.xhat, ro.names, ro.dist_scaling)
    print("wide field general:", {k: f"{v:.1e}" for k, v in err.items()},
          f"sigma0^2 {abs(res.sigma02 - ro.sigma02) / ro.sigma02:.1e} "
          f"deltasum {np.abs(res.deltasum - np.array(ro.deltasum)).max() / ro.deltasum[0]:.1e} "
          f"v {np.abs(res.v - ro.v).max() / np.abs(ro.v).max():.1e}")
    assert max(err.values()) <= 1e-9, err
    assert res.sigma02 == pytest.approx(ro.sigma02, rel=1e-9)
    np.testing.assert_allclose(res.deltasum, ro.deltasum, rtol=0, atol=1e-9 * ro.deltasum[0])
    assert np.abs(res.v - ro.v).max() <= 1e-10 * np.abs(ro.v).max()
    cdo, corro = oracle.covariance(od, ro)
    np.testing.assert_allclose(res.cx_diag, cdo, rtol=1e-8, atol=0)
    u_img, u_cam = oracle.counts(od.settings)
    for e in range(od.numImg):
        idx = list(range(e * u_img, (e + 1) * u_img)) + list(range(u_img * od.numImg, u_img * od.numImg + u_cam))
        np.testing.assert_allclose(res.corr[e], corro[np.ix_(idx, idx)], rtol=0, atol=5e-9)
    # test_gpu_reliability's comparison, its helper and bars
    _check("wide field general", res, _reference(oracle, od, ro), od, ro)
