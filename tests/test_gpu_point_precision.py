"""fba_postfit_outputs on the GPU: every tie point's full 3 x 3 block of the final Cx (k_cov_pts_blk, k_cov_gen_blk) and
its error ellipsoid (k_ellipsoid) against the dense oracle.

The oracle: the cofactor Cx = oracle.solve_dense(od, A, w, G, P)[1] of the last pass (main.m:428-444); a point's block
is its three consecutive tie indices of the xhat layout (the tie points are xhat's last 3 n_tie entries, TIE order),
times sigma0^2; numpy.linalg.eigh of that block is the oracle's ellipsoid.

Bars, none from a run.  Blocks: |dC_ij| <= bar sqrt(C_ii C_jj), bar = max(1e-8, 20 x the oracle's own spread) --
1e-8 is test_gpu_parity._check_cov's bar on diag(Cx); the spread is the oracle's explicit inverse against the symmetric
solve of the same bordered matrix against the identity (flag_masks.cov_self_spread's pair) on the tie blocks'
correlation form |dC_ij| / sqrt(C_ii C_jj).  The block's diagonal against cx_diag's tie entries: 1e-10 relative (a
reordered fp64 sum).  Eigenvalues: |d lambda| <= 3 bar max_i C_ii (Weyl: the block bar bounds every entry of the
perturbation by bar max C_ii, its 2-norm by 3 times that).  Directions, up to sign, where the vector's relative gap
min_j |lambda_i - lambda_j| / lambda_max exceeds 1e-3: sine of the angle <= 4 bar / gap; the points with a vector this
leaves out are at most 5 % of a scene's tie points (asserted; every scene below was checked with the oracle alone when
it was chosen).  Every run: symmetric blocks, a >= b >= c > 0, orthonormal D, and D' diag(a^2) D reproducing the
GPU's own block at test_ellipsoid_host's bar.

sigma0^2.  cx_tie is linear in the sigma02 the caller hands fba_postfit_outputs, and the reference is the oracle's
cofactor times ITS sigma0^2.  Two exact restatements of the reference do not agree on sigma0^2 to the block bar
everywhere: on cam0's fish-eye variant (inner constraints + control points + a non-pinhole model, conftest.
solver_spread) the oracle's explicit inverse and its LU solve end 3e-8 apart in sigma0^2 (test_gpu_reliability's
vtol there is 6e-7); the device's sigma0^2 there is 3.0e-8 from the oracle's, and with it the blocks were 3.9e-8
from the oracle's, with the oracle's own 9.4e-9.  The scene tests therefore run the adjustment through a context
(_run: adjust()'s calls) and hand fba_postfit_outputs the oracle's sigma0^2, so that the blocks are compared and not
sigma0^2, which the existing suites hold to their own bar; the device's own sigma0^2 is printed beside it.

The measured figures of one run, with the bars beside them: profiles/point_precision_gpu_errors.log (the
"point-precision ..." and "ellipsoid ..." prints of this module).
"""
import os
import shutil
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR = 1e-8   # test_gpu_parity._check_cov's bar on diag(Cx)
GAP = 1e-3
LEFT_OUT = 0.05


# ---- the oracle -------------------------------------------------------------------------------------------------
def oracle_blocks(oracle, od, A, w, G, P, sigma02, n_tie):
    """-> (blocks (n_tie, 3, 3) = sigma02 x the tie blocks of the explicit inverse, the oracle's own spread on their
    correlation form: the explicit inverse against the symmetric solve of the same bordered matrix)"""
    import scipy.linalg as sla
    _, Cx = oracle.solve_dense(od, A, w, G, P)
    u = len(Cx)
    N = A.T @ (P[:, None] * A)
    if od.settings["Inner_Constraints"]:
        d = G.shape[1]
        N = np.block([[N, G], [G.T, np.zeros((d, d))]])
    Cl = sla.solve(N, np.eye(len(N)), assume_a="sym")[:u, :u]
    t0 = u - 3 * n_tie
    idx = t0 + 3 * np.arange(n_tie)[:, None] + np.arange(3)[None, :]
    blk = Cx[idx[:, :, None], idx[:, None, :]]
    bll = Cl[idx[:, :, None], idx[:, None, :]]
    if n_tie == 0:
        return sigma02 * blk, 0.0
    s = np.sqrt(np.einsum("tii->ti", blk))
    return sigma02 * blk, float(np.max(np.abs(bll - blk) / (s[:, :, None] * s[:, None, :])))


def left_out(blocks):
    """per point: True where one of its three axis directions is not compared (relative gap <= GAP)"""
    w = np.linalg.eigvalsh(blocks)[:, ::-1]
    gap = np.minimum.reduce([np.abs(w[:, [0, 0, 1]] - w[:, [1, 2, 2]])[:, k] for k in range(3)]) / w[:, 0]
    return gap <= GAP


def check_scene(tag, res, blocks, own):
    """res.cx_tie / ell_axes / ell_dirs / cx_diag of one adjustment against the oracle's blocks; prints first"""
    from test_ellipsoid_host import check_ellipsoids, pack6
    n_tie = len(blocks)
    assert res.cx_tie.shape == (n_tie, 3, 3) and res.ell_axes.shape == (n_tie, 3) and res.ell_dirs.shape == (n_tie, 3, 3)
    if n_tie == 0:
        print(f"point-precision {tag}: no tie points")
        return
    bar = max(FLOOR, 20 * own)
    C = res.cx_tie
    np.testing.assert_array_equal(C, np.transpose(C, (0, 2, 1)))
    s = np.sqrt(np.einsum("tii->ti", blocks))
    e_blk = float(np.max(np.abs(C - blocks) / (s[:, :, None] * s[:, None, :])))
    dg = np.einsum("tii->ti", C).reshape(-1)
    e_dg = float(np.max(np.abs(dg - res.cx_diag[-3 * n_tie:]) / res.cx_diag[-3 * n_tie:]))
    wo, Vo = np.linalg.eigh(blocks)
    wo, Do = wo[:, ::-1], np.transpose(Vo, (0, 2, 1))[:, ::-1]
    cmax = np.einsum("tii->ti", blocks).max(axis=1)
    e_lam = float(np.max(np.abs(res.ell_axes ** 2 - wo) / cmax[:, None]))
    out = left_out(blocks)
    worst_ang, worst_ratio, compared = 0.0, 0.0, 0
    for t in range(n_tie):
        for i in range(3):
            gap = min(abs(wo[t, i] - wo[t, j]) for j in range(3) if j != i) / wo[t, 0]
            if gap > GAP:
                sn = float(np.linalg.norm(np.cross(res.ell_dirs[t, i], Do[t, i])))
                compared += 1
                worst_ang = max(worst_ang, sn)
                worst_ratio = max(worst_ratio, sn * gap / (4 * bar))
    print(f"point-precision {tag}: n_tie={n_tie} block error {e_blk:.2e} (bar {bar:.1e}, oracle's own spread {own:.1e}) "
          f"diagonal vs cx_diag {e_dg:.2e} (bar 1e-10) eigenvalues {e_lam:.2e} (bar {3 * bar:.1e}) directions worst sine "
          f"{worst_ang:.2e}, worst sine x gap / (4 bar) {worst_ratio:.2e} over {compared} vectors; points left out "
          f"{int(out.sum())} of {n_tie} (cap {LEFT_OUT:.0%}); axes a {res.ell_axes[:, 0].min():.3g}..{res.ell_axes[:, 0].max():.3g} "
          f"c {res.ell_axes[:, 2].min():.3g}..{res.ell_axes[:, 2].max():.3g} a/c up to {(res.ell_axes[:, 0] / res.ell_axes[:, 2]).max():.1f}")
    assert e_blk <= bar
    assert e_dg <= 1e-10
    assert e_lam <= 3 * bar
    assert worst_ratio <= 1.0
    assert out.sum() <= LEFT_OUT * n_tie
    assert (res.ell_axes[:, 2] > 0).all()
    check_ellipsoids(f"{tag} (GPU, its own blocks)", np.array([pack6(c) for c in C]),
                     np.concatenate([res.ell_axes, res.ell_dirs.reshape(-1, 9)], axis=1))


def _run(fba, ds, sigma02, weights=None, priors=None):
    """bundle.adjust(ds, point_precision=True)'s calls on a context, with the given sigma02 for the post-fit outputs"""
    from types import SimpleNamespace
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), priors=priors)
    try:
        if weights is not None:
            ctx.set_weights(weights)
        it, _ = ctx.adjust()
        own = ctx.residuals()[2][3]
        cxd, _, _, _, blk, ell = ctx.postfit(sigma02)
    finally:
        ctx.close()
    print(f"point-precision: the device's sigma0^2 {own:.15g}, the oracle's {sigma02:.15g}, relative difference "
          f"{abs(own - sigma02) / sigma02:.2e}")
    return SimpleNamespace(iterations=it, cx_diag=cxd, cx_tie=fba.capi.tie_blocks(blk), ell_axes=ell[:, :3],
                           ell_dirs=ell[:, 3:].reshape(-1, 3, 3))


def plain_reference(oracle, od, ro):
    return oracle_blocks(oracle, od, ro.A, ro.w, ro.G, oracle.weights(od), ro.sigma02, len(od.TIE))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("point_precision"), "scenes": {}, "cache": {}}


# ---- 1. cam0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["stage3_pinhole", "stage1_pinhole", "stage3_noic_pinhole", "stage3_fisheye"])
def test_cam0_matches_dense_oracle(fba, oracle, cam0_folders, variant):
    """the border on (stage 3) and off (noic), the fish-eye model, tie points next to three fixed control points;
    stage 1 estimates no tie point: empty outputs, and the call still runs"""
    od = oracle.load_folder(cam0_folders[variant])
    ro = oracle.adjust(od)
    ds = fba.load_folder(cam0_folders[variant])
    res = _run(fba, ds, ro.sigma02)
    assert res.iterations == ro.iterations
    assert (len(od.TIE) == 0) == (variant == "stage1_pinhole")
    check_scene(f"cam0 {variant}", res, *plain_reference(oracle, od, ro))


# ---- 2. block-shape rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["u129-leaf12", "u256", "control-leaf12", "b8-leaf8"])
def test_block_shape_rows_match_dense_oracle(fba, oracle, work, row, monkeypatch):
    """cross-block C reads through the rr / cc swap with the mirrored pair's off-diagonal terms (all four), padding
    rows of Z / Wz (u129-leaf12, b8-leaf8), no border (control-leaf12), absent off-pattern blocks (b8-leaf8)"""
    from test_gpu_block_shapes import _oracle, _set_leaf, assert_shape
    _set_leaf(monkeypatch, row)
    s = _oracle(fba, oracle, work, row)
    assert_shape(fba, s["ds"], row)
    if "pp" not in s:
        s["pp"] = plain_reference(oracle, s["od"], s["ro"])
    res = _run(fba, s["ds"], s["ro"].sigma02)
    assert res.iterations == s["ro"].iterations
    check_scene(f"block-shapes {row}", res, *s["pp"])


# ---- 3. general points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dup", "rig2", "rig3_blocks"])
def test_general_points_match_dense_oracle(fba, oracle, tmp_path, name):
    """k_cov_gen_blk: points seen through two / three cameras, points measured twice in one image, next to regular
    points (rig3_blocks)"""
    from test_gpu_general import SCENES, _folder, _general_count
    folder = _folder(tmp_path, name, **SCENES[name])
    od = oracle.load_folder(folder)
    assert _general_count(od) > 0
    ro = oracle.adjust(od)
    res = _run(fba, fba.load_folder(folder), ro.sigma02)
    assert res.iterations == ro.iterations
    check_scene(f"general {name}", res, *plain_reference(oracle, od, ro))


# ---- 4. partial flag sets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["no_Zc_kappa", "eop_kappa_off"])
def test_partial_flag_sets_match_dense_oracle(fba, oracle, work, mask):
    """EOP columns missing (no_Zc_kappa) and no camera unknown at all, cw rows of unit diagonal (eop_kappa_off), on
    flag_masks' control scene"""
    import flag_masks as fm
    folder = fm.synth_folder(work["root"], "control", mask)
    od = oracle.load_folder(folder)
    ro = oracle.adjust(od)
    res = _run(fba, fba.load_folder(folder), ro.sigma02)
    assert res.iterations == ro.iterations
    check_scene(f"mask {mask}", res, *plain_reference(oracle, od, ro))


# ---- 5. priors and per-observation weights ----------------------------------------------------------------------
def test_priors_with_weighted_tie_points(fba, oracle, cam0_folders, work):
    """test_gpu_priors.cam0_mix on cam0 with control points (f = 3): 31 priors, the first five tie points' X Y Z
    among them -- regular points routed to the general path by their priors, V carrying the prior weights"""
    import test_gpu_priors as tp
    folder = cam0_folders["stage3_noic_pinhole"]
    od, base = tp._cam0_base(oracle, work, folder)
    pri = tp.cam0_mix(oracle, od, 3.0, base)
    ro = tp.gn(oracle, od, pri)
    res = _run(fba, fba.load_folder(folder), ro.sigma02, priors=pri)
    assert res.iterations == ro.iterations
    check_scene("priors cam0 stage3_noic_pinhole f=3", res,
                *oracle_blocks(oracle, od, ro.aug.A, ro.aug.w, ro.aug.G, ro.Pa, ro.sigma02, len(od.TIE)))


def test_per_observation_weights(fba, oracle, cam0_folders):
    """test_gpu_weights' weighted cam0 (log-uniform weights over six decades, seed 11): V and T from whitened rows"""
    import test_gpu_weights as tw
    folder = cam0_folders["stage3_pinhole"]
    od = oracle.load_folder(folder)
    wt = tw.random_weights(od.n, 11)
    ref = tw.weighted_oracle(oracle, od, wt)
    ro = ref["ro"]
    res = _run(fba, fba.load_folder(folder), ro.sigma02, weights=wt)
    assert res.iterations == ro.iterations
    check_scene("weights cam0 stage3_pinhole", res,
                *oracle_blocks(oracle, od, ro.A, ro.w, ro.G, ref["Pw"], ro.sigma02, len(od.TIE)))


# ---- 6. contract ------------------------------------------------------------------------------------------------
def test_contract(fba, cam0_folders):
    """cx_diag / corr / redundancy / wstat bit-identical to fba_covariance's / fba_reliability's from identically
    stepped contexts; every NULL combination of the two new outputs; the factor is consumed (a second call, a call
    before any solve and a call after a damped solve give FBA_ERR_ARG); two runs give bitwise-equal cx_tie and
    ellipsoid"""
    import itertools
    from test_gpu_parity import _ctx
    ds = fba.load_folder(cam0_folders["stage3_pinhole"])
    ctxs = []
    try:
        def stepped(damped_last=False):
            c = _ctx(fba, ds)
            ctxs.append(c)
            for _ in range(3):
                c.step()
            if damped_last:
                c.set_damping(1e-3)
                c.step()
            return c
        fresh = _ctx(fba, ds)
        ctxs.append(fresh)
        with pytest.raises(fba.capi.FBAError) as ei:
            fresh.postfit(1.0)
        assert ei.value.code == 1  # FBA_ERR_ARG
        with pytest.raises(fba.capi.FBAError) as ei:
            stepped(damped_last=True).postfit(1.0)
        assert ei.value.code == 1
        a, b, c1, c2 = stepped(), stepped(), stepped(), stepped()
        s02 = a.residuals()[2][3]
        cd0, cr0 = a.covariance(s02)
        cd1, cr1, r1, w1 = b.reliability(s02)
        cd2, cr2, r2, w2, blk, ell = c1.postfit(s02, reliability=True)
        for got, want in ((cd2, cd0), (cr2, cr0), (cd2, cd1), (cr2, cr1), (r2, r1), (w2, w1)):
            np.testing.assert_array_equal(got, want)
        n_tie = ds.pack().n_tie
        assert blk.shape == (n_tie, 6) and ell.shape == (n_tie, 12) and n_tie > 0
        assert np.isfinite(blk).all() and np.isfinite(ell).all() and (ell[:, 2] > 0).all()
        with pytest.raises(fba.capi.FBAError) as ei:
            c1.postfit(s02)
        assert ei.value.code == 1
        cd3, cr3, r3, w3, blk3, ell3 = c2.postfit(s02, reliability=True)
        np.testing.assert_array_equal(blk3, blk)
        np.testing.assert_array_equal(ell3, ell)
        for rel, tie_cov, ellipsoids in itertools.product([False, True], repeat=3):
            c = stepped()
            out = c.postfit(s02, reliability=rel, tie_cov=tie_cov, ellipsoids=ellipsoids)
            for got, want, use in zip(out, (cd0, cr0, r1, w1, blk, ell), (True, True, rel, rel, tie_cov, ellipsoids)):
                assert (got is not None) == use
                if use:
                    np.testing.assert_array_equal(got, want)
            c.close()
    finally:
        for c in ctxs:
            c.close()


# ---- 7. two rank contexts ---------------------------------------------------------------------------------------
def test_two_ranks_sum_to_single_context(fba, cam0_folders):
    """world = 2, replicated solve, cam0 stage 3: zeros outside a rank's own tie points, the ranks' sum is the
    single context's output within the block bar's floor"""
    from test_gpu_parity import _ctx
    from test_gpu_reliability import _step_ranks
    ds = fba.load_folder(cam0_folders["stage3_pinhole"])
    single = _ctx(fba, ds)
    ranks = [_ctx(fba, ds, rank=r, world=2) for r in range(2)]
    try:
        _step_ranks(single, ranks, 3)
        s02 = single.residuals()[2][3]
        blk1, ell1 = single.postfit(s02)[4:]
        outs = [c.postfit(s02)[4:] for c in ranks]
        tie_owner, _ = fba.capi.partition(ds.pack(), 2)
        assert set(tie_owner.tolist()) == {0, 1}
        for k, (blk, ell) in enumerate(outs):
            mine = tie_owner == k
            assert (blk[~mine] == 0).all() and (ell[~mine] == 0).all() and (ell[mine, 2] > 0).all()
        blk_s, ell_s = outs[0][0] + outs[1][0], outs[0][1] + outs[1][1]
        C1, Cs = fba.capi.tie_blocks(blk1), fba.capi.tie_blocks(blk_s)
        s = np.sqrt(np.einsum("tii->ti", C1))
        e_blk = float(np.max(np.abs(Cs - C1) / (s[:, :, None] * s[:, None, :])))
        e_lam = float(np.max(np.abs(ell_s[:, :3] ** 2 - ell1[:, :3] ** 2) / (s ** 2).max(axis=1)[:, None]))
        print(f"point-precision two ranks: sum vs single blocks {e_blk:.2e} (bar {FLOOR:.0e}) eigenvalues {e_lam:.2e} "
              f"(bar {3 * FLOOR:.0e})")
        assert e_blk <= FLOOR and e_lam <= 3 * FLOOR
    finally:
        for c in [single] + ranks:
            c.close()


# ---- 8. config 3: the subtree split, timing ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def config3(tmp_path_factory):
    from fba_amd import synth
    return synth.make_config(3, str(tmp_path_factory.mktemp("pp_c3") / "c3"))


def test_subtree_split(fba, config3):
    """a split context (fba_solve_mode 1): a non-NULL redundancy returns FBA_ERR_UNSUPPORTED and leaves the factor
    in place -- the call without it then succeeds on the same contexts --, and the diagonal of the ranks' summed
    cx_tie is the summed cx_diag's tie entries to 1e-10 relative"""
    from test_gpu_parity import _ctx
    from test_gpu_reliability import _step_ranks
    ds = fba.load_folder(config3)
    ranks = [_ctx(fba, ds, rank=r, world=2, split=True) for r in range(2)]
    try:
        assert all(c.split for c in ranks)
        _step_ranks(None, ranks, 1)
        with pytest.raises(fba.capi.FBAError) as ei:
            ranks[0].postfit(1.0, reliability=True)
        assert ei.value.code == 5  # FBA_ERR_UNSUPPORTED
        assert "subtree split" in fba.capi.last_error()
        outs = [c.postfit(1.0, corr=False) for c in ranks]
        n_tie = ds.pack().n_tie
        cd = outs[0][0] + outs[1][0]
        blk = outs[0][4] + outs[1][4]
        ell = outs[0][5] + outs[1][5]
        dg = blk[:, [0, 3, 5]].reshape(-1)
        e_dg = float(np.max(np.abs(dg - cd[-3 * n_tie:]) / cd[-3 * n_tie:]))
        print(f"point-precision config 3 subtree split: n_tie={n_tie} diagonal of the summed cx_tie vs summed cx_diag "
              f"{e_dg:.2e} (bar 1e-10); semi-axes a {ell[:, 0].min():.3g}..{ell[:, 0].max():.3g} c "
              f"{ell[:, 2].min():.3g}..{ell[:, 2].max():.3g}")
        assert (cd[-3 * n_tie:] > 0).all() and e_dg <= 1e-10
        assert (ell[:, 0] >= ell[:, 1]).all() and (ell[:, 1] >= ell[:, 2]).all() and (ell[:, 2] > 0).all()
    finally:
        for c in ranks:
            c.close()


def test_config3_timing(fba, config3):
    """no bar: fba_covariance against fba_postfit_outputs with both new outputs on identically stepped single-GPU
    contexts (one pass each), a warm call on a throw-away context first, the median of 5 contexts each"""
    from test_gpu_parity import _ctx
    ds = fba.load_folder(config3)

    def timed(call):
        c = _ctx(fba, ds)
        try:
            c.step()
            t0 = time.perf_counter()
            out = call(c)
            return time.perf_counter() - t0, out
        finally:
            c.close()
    cov = lambda c: c.covariance(1.0)   # noqa: E731
    pf = lambda c: c.postfit(1.0)       # noqa: E731
    timed(cov)
    timed(pf)
    t_cov = [timed(cov) for _ in range(5)]
    t_pf = [timed(pf) for _ in range(5)]
    np.testing.assert_array_equal(t_pf[0][1][0], t_cov[0][1][0])
    m_cov, m_pf = float(np.median([t for t, _ in t_cov])), float(np.median([t for t, _ in t_pf]))
    print(f"point-precision config 3 timing (median of 5): fba_covariance {1e3 * m_cov:.2f} ms, fba_postfit_outputs "
          f"with cx_tie and ellipsoid {1e3 * m_pf:.2f} ms, ratio {m_pf / m_cov:.3f}")
    assert m_cov > 0 and m_pf > 0


# ---- 9. end to end ----------------------------------------------------------------------------------------------
def test_end_to_end_ell_table(fba, tmp_path):
    """adjust(ds, point_precision=True) and main(folder, ellipsoids=True) on cam0: the .ell table has n_tie rows
    and its sigma columns are sqrt(cx_diag) of the tie entries"""
    from conftest import CAM0
    from fba_amd import report
    folder = str(tmp_path / "cam0")
    shutil.copytree(CAM0, folder)
    ds = fba.load_folder(folder)
    res = fba.adjust(ds, point_precision=True)
    n_tie = ds.pack().n_tie
    assert res.cx_tie.shape == (n_tie, 3, 3) and n_tie > 0
    want = np.sqrt(res.cx_diag[-3 * n_tie:]).reshape(-1, 3)
    stem = os.path.splitext(ds.settings["Output_Filename"])[0]
    path = os.path.join(folder, stem + ".ell")
    report.write_ell(path, ds, res)
    names, sig, axes, dirs, hor = report.read_ell(path)
    assert names == list(ds.TIE)
    np.testing.assert_allclose(sig, want, rtol=1e-10)
    np.testing.assert_allclose(axes, res.ell_axes, rtol=1e-14)
    os.remove(path)
    assert fba.main(folder, ellipsoids=True) == 0
    names2, sig2, axes2, dirs2, hor2 = report.read_ell(path)
    assert names2 == names and len(names2) == n_tie
    np.testing.assert_allclose(sig2, want, rtol=1e-10)
    np.testing.assert_array_equal(axes2, axes)
    assert (hor2[:, 0] >= hor2[:, 1]).all() and (hor2[:, 2] >= 0).all() and (hor2[:, 2] < 180).all()
    # the horizontal ellipse never exceeds the ellipsoid's largest axis nor falls below its smallest
    assert (hor2[:, 0] <= axes2[:, 0] * (1 + 1e-12)).all() and (hor2[:, 1] >= axes2[:, 2] * (1 - 1e-12)).all()
