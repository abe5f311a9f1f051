"""fba_reliability on the GPU: redundancy numbers r = 1 - p a Cx a' and standardised residuals w = v / (sigma sqrt(r))
of every image measurement (csrc/fba_rel.hip) against the dense oracle.

The oracle quantity, in NumPy from oracle.adjust's last A, w, G: Cx = oracle.solve_dense(...)[1] (main.m:428-444,
before the de-scaling and sigma0^2), r = 1 - P rowsum((A Cx) o A), w = v / sqrt(r / P).

Bars.  r, absolute: max(1e-8, 20 x the oracle's own spread on r for the scene) -- its explicit inverse against a
symmetric solve of the same bordered matrix against the identity, the pair flag_masks.cov_self_spread uses; 1 - r =
p q <= 1 and q is a variance propagated from Cx, which test_gpu_parity._check_cov holds to 1e-8 relative.  w, per
element: |dw_i| <= |w_i| bar_r / (2 r_i) + 10 vtol max|w|, the r bar and test_gpu_block_shapes._every_pass' bar on v
(vtol = max(1e-9, 20 x the LU variant's spread on sigma0^2)) propagated through w = v / (sigma sqrt(r)).  Sum r = n
- u + d (d = 7 with inner constraints) within n bar_r.  The measured errors of one run, with the oracle's own spread
beside them: profiles/reliability_gpu_errors.log (the "reliability ..." prints of this module).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_FLOOR = 1e-8


def _oracle_rel(oracle, od, ro, Cx=None):
    P = oracle.weights(od)
    if Cx is None:
        _, Cx = oracle.solve_dense(od, ro.A, ro.w, ro.G, P)
    r = 1.0 - P * np.einsum("ij,ij->i", ro.A @ Cx, ro.A)
    return r, ro.v / np.sqrt(r / P)


def _own_spread_r(oracle, od, ro, r):
    """the oracle's own spread on r: the symmetric solve against the identity instead of numpy's inv"""
    import scipy.linalg as sla
    P = oracle.weights(od)
    N = ro.A.T @ (P[:, None] * ro.A)
    u = len(N)
    if od.settings["Inner_Constraints"]:
        d = ro.G.shape[1]
        N = np.block([[N, ro.G], [ro.G.T, np.zeros((d, d))]])
    Cl = sla.solve(N, np.eye(len(N)), assume_a="sym")[:u, :u]
    return float(np.abs(_oracle_rel(oracle, od, ro, Cl)[0] - r).max())


def _vtol(oracle, od, ro, lu=None):
    from test_gpu_block_shapes import _solve_lu
    lu = lu or oracle.adjust(od, solver=_solve_lu)
    return max(1e-9, 20 * abs(lu.sigma02 - ro.sigma02) / ro.sigma02)


def _reference(oracle, od, ro, lu=None):
    r, w = _oracle_rel(oracle, od, ro)
    own = _own_spread_r(oracle, od, ro, r)
    return dict(r=r, w=w, own=own, bar_r=max(R_FLOOR, 20 * own), vtol=_vtol(oracle, od, ro, lu),
                d=7 if od.settings["Inner_Constraints"] else 0)


def _check(tag, res, ref, od, ro):
    """all r and w against the oracle, the redundancy sum and 0 < r < 1; prints the measured figures first"""
    r, w, bar_r = ref["r"], ref["w"], ref["bar_r"]
    n, u = ro.A.shape
    assert res.redundancy.shape == res.wstat.shape == (n,)
    e_r = np.abs(res.redundancy - r)
    bar_w = np.abs(w) * bar_r / (2 * r) + 10 * ref["vtol"] * np.abs(w).max()
    e_w = np.abs(res.wstat - w)
    worst_w = int(np.argmax(e_w / bar_w))
    e_sum = res.redundancy.sum() - (n - u + ref["d"])
    print(f"reliability {tag}: n={n} u={u} r error {e_r.max():.2e} (bar {bar_r:.1e}, oracle's own spread {ref['own']:.1e}) "
          f"w error/bar worst {e_w[worst_w]:.2e}/{bar_w[worst_w]:.2e} at r={r[worst_w]:.2e} (max |dw| {e_w.max():.2e}, "
          f"vtol {ref['vtol']:.1e}) sum r - (n-u+d) {e_sum:.2e} (oracle {r.sum() - (n - u + ref['d']):.2e}) "
          f"r min/max {res.redundancy.min():.3e}/{res.redundancy.max():.3f} max|w| {np.abs(res.wstat).max():.2f}")
    assert e_r.max() <= bar_r
    assert (e_w <= bar_w).all(), (worst_w, e_w[worst_w], bar_w[worst_w])
    assert abs(e_sum) <= n * bar_r
    assert (res.redundancy > 0).all() and (res.redundancy < 1).all()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("reliability"), "scenes": {}}


# ---- 1. cam0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["stage3_pinhole", "stage1_pinhole", "stage3_noic_pinhole", "stage3_fisheye"])
def test_cam0_matches_dense_oracle(fba, oracle, cam0_folders, variant):
    """the border on (stage 3) and off (noic), EOPs only (stage 1), tie points with three fixed control points
    (k_rel_pts and k_rel_ctl); redundancies down to 1.6e-3, where the propagated w bar bites"""
    od = oracle.load_folder(cam0_folders[variant])
    ro = oracle.adjust(od)
    ref = _reference(oracle, od, ro)
    res = fba.adjust(fba.load_folder(cam0_folders[variant]), reliability=True)
    assert res.iterations == ro.iterations
    _check(f"cam0 {variant}", res, ref, od, ro)


# ---- 2. block-shape rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["u129-leaf12", "u256", "control-leaf12", "b8-leaf8"])
def test_block_shape_rows_match_dense_oracle(fba, oracle, work, row, monkeypatch):
    """the smallest scenes with cross-block C reads through the rr / cc swap (all four), padding rows of Z / Wz
    within the border's first 21 slots (u129-leaf12, b8-leaf8), a dissected pattern without a border plus control
    observations (control-leaf12) and absent off-pattern blocks (b8-leaf8)"""
    from test_gpu_block_shapes import _oracle, _set_leaf, assert_shape
    _set_leaf(monkeypatch, row)
    s = _oracle(fba, oracle, work, row)
    assert_shape(fba, s["ds"], row)
    if "rel" not in s:
        s["rel"] = _reference(oracle, s["od"], s["ro"], s["lu"])
    res = fba.adjust(s["ds"], reliability=True)
    assert res.iterations == s["ro"].iterations
    _check(f"block-shapes {row}", res, s["rel"], s["od"], s["ro"])


# ---- 3. general points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dup", "rig2", "rig3_blocks"])
def test_general_points_match_dense_oracle(fba, oracle, tmp_path, name):
    """k_rel_gen: points seen through two / three cameras, points measured twice in one image, next to regular
    points (rig3_blocks)"""
    from test_gpu_general import SCENES, _folder, _general_count
    folder = _folder(tmp_path, name, **SCENES[name])
    od = oracle.load_folder(folder)
    assert _general_count(od) > 0
    ro = oracle.adjust(od)
    ref = _reference(oracle, od, ro)
    res = fba.adjust(fba.load_folder(folder), reliability=True)
    assert res.iterations == ro.iterations
    _check(f"general {name}", res, ref, od, ro)


# ---- 4. partial flag sets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["no_Zc_kappa", "eop_kappa_off"])
def test_partial_flag_sets_match_dense_oracle(fba, oracle, work, mask):
    """EOPs not estimated (no_Zc_kappa) and no IOP / distortion unknown at all (eop_kappa_off) on flag_masks' control
    scene: zero Jacobian columns against unit-diagonal rows of the full parameter space contribute nothing"""
    import flag_masks as fm
    folder = fm.synth_folder(work["root"], "control", mask)
    od = oracle.load_folder(folder)
    ro = oracle.adjust(od)
    ref = _reference(oracle, od, ro)
    res = fba.adjust(fba.load_folder(folder), reliability=True)
    assert res.iterations == ro.iterations
    _check(f"mask {mask}", res, ref, od, ro)


# ---- 5. a planted blunder ---------------------------------------------------------------------------------------
def test_planted_blunder_is_found(fba, oracle, tmp_path):
    """+6 px on the x of PHO row 100 of the "u129" scene: the largest |w| sits on that measurement (index 200), in
    the oracle and on the GPU, and write_rel flags that row"""
    from fba_amd import report, synth
    from test_gpu_block_shapes import ROWS
    r = ROWS["u129"]
    sc = dict(synth.generate(r["n_img"], r["n_tie"], seed=r["seed"], obs_per_point=r["opp"], n_control=r["n_control"]))
    order = np.lexsort((sc["pid"], sc["img"]))  # write_folder's PHO order
    sc["xy"] = sc["xy"].copy()
    sc["xy"][order[100], 0] += 6.0
    folder = synth.write_folder(sc, str(tmp_path / "blunder"), nk=r["nk"])
    od = oracle.load_folder(folder)
    ro = oracle.adjust(od)
    _, wo = _oracle_rel(oracle, od, ro)
    assert int(np.argmax(np.abs(wo))) == 200
    second = float(np.abs(np.delete(wo, 200)).max())
    assert second < 0.5 * abs(wo[200]), (wo[200], second)
    ds = fba.load_folder(folder)
    res = fba.adjust(ds, reliability=True)
    print(f"reliability blunder: oracle |w| {abs(wo[200]):.2f} at 200, next {second:.2f}; GPU |w| {abs(res.wstat[200]):.2f}, "
          f"next {np.abs(np.delete(res.wstat, 200)).max():.2f}")
    assert int(np.argmax(np.abs(res.wstat))) == 200
    path = str(tmp_path / "blunder.rel")
    report.write_rel(path, ds, res)
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert len(rows) == ds.n_pts and rows[100][-1] == "*"
    assert rows[100][:2] == [ds.pho_target[100], ds.pho_image[100]]


# ---- 6. config-3 scale ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config3(tmp_path_factory):
    from fba_amd import synth
    return synth.make_config(3, str(tmp_path_factory.mktemp("rel_c3") / "c3"))


def test_config3_redundancy_sum(fba, config3):
    """200 images x 5,000 tie points (no dense oracle): 0 < r < 1 everywhere and sum r = n - u + 7 within n x 1e-8"""
    ds = fba.load_folder(config3)
    res = fba.adjust(ds, reliability=True)
    n, u = 2 * ds.n_pts, len(res.xhat)
    r = res.redundancy
    e_sum = r.sum() - (n - u + 7)
    print(f"reliability config 3: n={n} u={u} sum r - (n-u+7) = {e_sum:.3e} (bar {n * R_FLOOR:.1e}) r min/median/max "
          f"{r.min():.4f}/{np.median(r):.4f}/{r.max():.4f} max|w| {np.abs(res.wstat).max():.2f}")
    assert (r > 0).all() and (r < 1).all()
    assert abs(e_sum) <= n * R_FLOOR


# ---- 7. two rank contexts ---------------------------------------------------------------------------------------
def _step_ranks(single, ranks, passes):
    """test_gpu_parity.test_sharded_ranks_reassemble_single_gpu_result's loop: reduce buffers summed on the host"""
    from test_gpu_parity import _Hip
    hip = _Hip()
    for _ in range(passes):
        if single is not None:
            single.step()
        for c in ranks:
            c.accumulate()
            c.synchronize()
        bufs = [c.reduce_buffer() for c in ranks]
        total = sum(hip.d2h(p, n) for p, n in bufs)
        for p, n in bufs:
            hip.h2d(p, total)
        for c in ranks:
            c.solve_update()


def test_two_ranks_sum_to_single_context(fba, cam0_folders):
    """world = 2, replicated solve, cam0 stage 3: each rank fills its own observations (0 elsewhere), the sum is
    the single context's result within the r bar"""
    from test_gpu_parity import _ctx
    ds = fba.load_folder(cam0_folders["stage3_pinhole"])
    single = _ctx(fba, ds)
    ranks = [_ctx(fba, ds, rank=r, world=2) for r in range(2)]
    try:
        _step_ranks(single, ranks, 3)
        s02 = single.residuals()[2][3]
        _, _, r1, w1 = single.reliability(s02)
        outs = [c.reliability(s02) for c in ranks]
        tie_owner, ctl_owner = fba.capi.partition(ds.pack(), 2)
        pk = ds.pack()
        owner = np.where(pk.tie >= 0, tie_owner[np.maximum(pk.tie, 0)], ctl_owner)
        for k, (_, _, r, w) in enumerate(outs):
            mine = np.repeat(owner == k, 2)
            assert (r[~mine] == 0).all() and (w[~mine] == 0).all() and (r[mine] > 0).all()
        rs, ws = outs[0][2] + outs[1][2], outs[0][3] + outs[1][3]
        print(f"reliability two ranks: sum vs single r {np.abs(rs - r1).max():.2e} w {np.abs(ws - w1).max():.2e}")
        assert np.abs(rs - r1).max() <= R_FLOOR
        # w = v / (sigma sqrt(r)): the r bar propagated, plus the ranks' v at 1e-9 of its scale
        assert (np.abs(ws - w1) <= np.abs(w1) * R_FLOOR / (2 * r1) + 1e-8 * np.abs(w1).max()).all()
    finally:
        for c in [single] + ranks:
            c.close()


def test_subtree_split_is_unsupported(fba, config3):
    """a split context (fba_solve_mode 1) returns FBA_ERR_UNSUPPORTED and leaves the message set"""
    from test_gpu_parity import _ctx
    ds = fba.load_folder(config3)
    ranks = [_ctx(fba, ds, rank=r, world=2, split=True) for r in range(2)]
    try:
        assert all(c.split for c in ranks)
        _step_ranks(None, ranks, 1)
        with pytest.raises(fba.capi.FBAError) as ei:
            ranks[0].reliability(1.0)
        assert ei.value.code == 5  # FBA_ERR_UNSUPPORTED
        assert "subtree split" in fba.capi.last_error()
    finally:
        for c in ranks:
            c.close()


# ---- 8. contract ------------------------------------------------------------------------------------------------
def test_contract(fba, cam0_folders):
    """cx_diag / corr bit-identical to fba_covariance's from an identically stepped context; the factor is consumed
    (a second call, and a call before any solve, give FBA_ERR_ARG); NULL outputs in any combination; two runs give
    bitwise-equal r and w"""
    import itertools
    from test_gpu_parity import _ctx
    ds = fba.load_folder(cam0_folders["stage3_pinhole"])
    lib, h = fba.capi.lib, fba.capi.ptr
    n, ctxs = 2 * ds.n_pts, []
    try:
        def stepped():
            c = _ctx(fba, ds)
            ctxs.append(c)
            for _ in range(3):
                c.step()
            return c
        fresh = _ctx(fba, ds)
        ctxs.append(fresh)
        with pytest.raises(fba.capi.FBAError) as ei:
            fresh.reliability(1.0)
        assert ei.value.code == 1  # FBA_ERR_ARG
        a, b, c2 = stepped(), stepped(), stepped()
        s02 = a.residuals()[2][3]
        cd0, cr0 = a.covariance(s02)
        cd1, cr1, r1, w1 = b.reliability(s02)
        np.testing.assert_array_equal(cd1, cd0)
        np.testing.assert_array_equal(cr1, cr0)
        with pytest.raises(fba.capi.FBAError) as ei:
            b.reliability(s02)
        assert ei.value.code == 1
        _, _, r2, w2 = c2.reliability(s02)
        np.testing.assert_array_equal(r2, r1)
        np.testing.assert_array_equal(w2, w1)
        # every combination of NULL outputs (a context per call: the factor is consumed); the given ones as above
        mu = cr0.shape[1]
        for mask in itertools.product([False, True], repeat=4):
            c = stepped()
            bufs = [np.zeros(len(cd0)), np.zeros((ds.pack().n_img, mu, mu)), np.zeros(n), np.zeros(n)]
            args = [h(x) if use else None for x, use in zip(bufs, mask)]
            fba.capi.check(lib.fba_reliability(c.h, float(s02), *args))
            for x, use, want in zip(bufs, mask, (cd0, cr0, r1, w1)):
                if use:
                    np.testing.assert_array_equal(x, want)
            c.close()
    finally:
        for c in ctxs:
            c.close()
