"""GPU parity under partial Estimate_* flag sets (tests/flag_masks.py).

The device code works in a full parameter space and applies the flags through Jacobian masks
(eop_mask / cam_mask), the unit rows of k_border_rhs and a compression at the C-ABI (full_to_ref_map:
xhat in and out, the dense A's columns, dist_scaling's index columns, BuildRSD's xp / yp, the covariance's
sel[] compaction).  Here every mask of the table goes through BuildAwG, the whole adjustment and the
covariance against the dense oracle, and a partial mask through each of: chunked points, general points
(rig2 / dup), the inner-constraint border (the free network), control points, the sharded replicated solve,
BuildRSD and the reference's own text (tests/golden/ref_cam0_{mix_a_noic,stage2}_pinhole.npz).

Bars: BuildAwG as tests/test_gpu_parity.py (A per column <= 1e-12, w <= 1e-12 of the scale, G and
dist_scaling <= 1e-14; dist_scaling's index columns exactly).  Whole adjustment: flag_masks.bars, i.e.
max(1e-9, 20 x conftest.solver_spread) as test_adjust_cam0; v <= 1e-10 of its scale.  Covariance: 1e-8
relative on diag(Cx) and 5e-9 absolute on the correlations (test_gpu_parity._check_cov).  The measured
errors per mask: profiles/flag_masks_gpu_errors.log.
"""
import ctypes

import numpy as np
import pytest

import flag_masks as fm
from conftest import ELEM_FLOOR, SMALL_SCENE_FLOOR, group_rel_err

pytestmark = pytest.mark.gpu

EOP_HEADS = {"Estimate_Xc": "Xc", "Estimate_Yc": "Yc", "Estimate_Zc": "Zc", "Estimate_w": "w", "Estimate_p": "p",
             "Estimate_k": "k"}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the module's scene folders and, per (scene, mask), the dense oracle's run with its restatement
    spread and the device run -- computed once, shared by the adjustment and covariance tests"""
    return {"root": tmp_path_factory.mktemp("masks"), "cases": {}}


def _folder(work, scene, mask):
    if scene == "cam0":
        return fm.cam0_folder(work["root"], mask)
    return fm.synth_folder(work["root"], scene, mask)


def _case(fba, oracle, work, scene, mask):
    key = (scene, mask)
    if key not in work["cases"]:
        folder = _folder(work, scene, mask)
        ds, od = fba.load_folder(folder), oracle.load_folder(folder)
        ro = oracle.adjust(od)
        floor = ELEM_FLOOR if scene == "cam0" else SMALL_SCENE_FLOOR
        bar, spread = fm.bars(oracle, od, ro, floor=floor)
        work["cases"][key] = dict(ds=ds, od=od, ro=ro, bar=bar, spread=spread, floor=floor, res=fba.adjust(ds))
    return work["cases"][key]


def _ctx(fba, ds, **kw):
    return fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)


def _check_awg(fba, oracle, ds, od, xhat):
    ctx = _ctx(fba, ds)
    try:
        A, w, G, dsc = ctx.build_awg(xhat)
    finally:
        ctx.close()
    Ao, wo, Go, dso = oracle.build_awg(od, xhat)
    assert A.shape == Ao.shape == (od.n, len(xhat))  # the oracle's compact n x u
    colmax = np.maximum(np.abs(Ao).max(axis=0), 1e-300)
    err = np.abs(A - Ao).max(axis=0) / colmax
    assert err.max() <= 1e-12, (err.max(), int(err.argmax()))
    assert ((A != 0) <= (Ao != 0) | (np.abs(A) < 1e-300)).all()
    assert np.abs(w - wo).max() <= 1e-12 * np.abs(ds.xy).max()
    if Go is not None:
        np.testing.assert_allclose(G, Go, rtol=1e-14, atol=1e-14 * np.abs(Go).max())
    else:
        assert G is None
    np.testing.assert_array_equal(dsc[:, :2], dso[:, :2])  # 1-based xhat index of the first K / P unknown, or 0
    np.testing.assert_allclose(dsc, dso, rtol=1e-14)
    return float(err.max())


def _awg_at_start_and_perturbed(fba, oracle, folder):
    ds, od = fba.load_folder(folder), oracle.load_folder(folder)
    ctx = _ctx(fba, ds)
    try:
        x0 = ctx.buildxhat()
    finally:
        ctx.close()
    x0o, names = oracle.buildxhat(od)
    np.testing.assert_array_equal(x0, x0o)  # Buildxhat.m layout under the mask, bit-exact
    assert fba.xhat_names(ds) == names
    e0 = _check_awg(fba, oracle, ds, od, x0)
    rng = np.random.default_rng(1)
    e1 = _check_awg(fba, oracle, ds, od, x0 * (1 + 1e-4 * rng.standard_normal(len(x0))))
    return od, max(e0, e1)


@pytest.mark.parametrize("scene", ["cam0", "control"])
@pytest.mark.parametrize("mask", sorted(fm.MASKS))
def test_buildawg_under_mask(fba, oracle, work, scene, mask):
    """fba_buildxhat and fba_build_awg under every mask, on cam0 (chunked points, 3 control points;
    Inner_Constraints 0 for the EOP and mixed masks, the border's G otherwise) and the 14 x 260 control scene."""
    _, e = _awg_at_start_and_perturbed(fba, oracle, _folder(work, scene, mask))
    print(f"flag-mask awg {scene} {mask}: A per column {e:.2e}")


@pytest.mark.parametrize("scene", ["rig2", "dup"])
@pytest.mark.parametrize("mask", ["c_k_only", "mix_b"])
def test_buildawg_general_points_under_mask(fba, oracle, work, scene, mask):
    """The general-point kernels (fba_general.hip) see the masked J: tests/test_gpu_general.py's rig2 (every
    point through both cameras: two camera blocks to compress) and dup (repeated measurements)."""
    from test_gpu_general import _general_count
    od, e = _awg_at_start_and_perturbed(fba, oracle, _folder(work, scene, mask))
    assert _general_count(od) > 0
    print(f"flag-mask awg {scene} {mask}: A per column {e:.2e}")


ADJUST_CASES = [("control", m) for m in sorted(fm.MASKS)] + [("free", m) for m in sorted(fm.CAM_MASKS)] + \
    [("cam0", m) for m in ("mix_a", "mix_b", "no_omega")] + [("rig2", "mix_a")]


def _estimated_heads(settings):
    heads = {h for k, h in EOP_HEADS.items() if settings[k]}
    heads |= {h for h in ("xp", "yp", "c") if settings["Estimate_" + h]}
    if settings["Estimate_radial"]:
        heads |= {f"k{j + 1}" for j in range(settings["Num_Radial_Distortions"])}
    if settings["Estimate_decent"]:
        heads |= {"p1", "p2"}
    return heads | {"X", "Y", "Z"}


@pytest.mark.parametrize("scene,mask", ADJUST_CASES)
def test_adjust_under_mask(fba, oracle, work, scene, mask):
    """The whole adjustment against the dense oracle: the 14 x 260 control scene under every mask, the
    12 x 240 free network (the inner-constraint border path) under the camera masks, cam0 without inner
    constraints under two mixed masks and an EOP mask, and the 2-camera rig (general points) under mix_a.
    Iteration count, xhat per group and per element, sigma0^2, the deltasum history, RMS at flag_masks.bars
    (1e-9, or 20x the restatement spread where larger: what test_adjust_cam0 allows); v <= 1e-10 of its
    scale.  The result has the oracle's length u and names: every entry an estimated parameter."""
    c = _case(fba, oracle, work, scene, mask)
    ds, od, ro, res, bar, spread = c["ds"], c["od"], c["ro"], c["res"], c["bar"], c["spread"]
    assert res.iterations == ro.iterations
    assert len(res.xhat) == len(ro.xhat) == len(ro.names) and list(res.xhatnames) == ro.names
    heads = _estimated_heads(od.settings)
    assert {nm.split("_", 1)[0] for nm in res.xhatnames} == heads, mask
    err = fm.errors(res.xhat, res.sigma02, res.deltasum[0], ro, floor=c["floor"])
    err_v = float(np.abs(res.v - ro.v).max() / np.abs(ro.v).max())
    assert len(res.deltasum) == len(ro.deltasum)
    err_d = np.abs(np.asarray(res.deltasum) - np.asarray(ro.deltasum)) / ro.deltasum[0]
    not_x = ("sigma02", "deltasum0", "deltasum_hist")
    print(f"flag-mask adjust {scene} {mask}: it {res.iterations} worst xhat "
          f"{max(v for k, v in err.items() if k not in not_x):.2e} sigma02 {err['sigma02']:.2e} "
          f"deltasum0 {err['deltasum0']:.2e} deltasum history {err_d.max():.2e} v {err_v:.2e}; restatement spread: "
          f"xhat {max(v for k, v in spread.items() if k not in not_x):.2e} deltasum0 {spread['deltasum0']:.2e} "
          f"history {spread['deltasum_hist'].max():.2e}")
    for g, e in err.items():
        assert e <= bar[g], (g, e, spread[g])
    assert (err_d <= bar["deltasum_hist"]).all(), (err_d, spread["deltasum_hist"])
    np.testing.assert_allclose(res.rms, ro.rms, rtol=bar["sigma02"])
    assert err_v <= 1e-10


@pytest.mark.parametrize("scene,mask", ADJUST_CASES)
def test_covariance_under_mask(fba, oracle, work, scene, mask):
    """fba_covariance's sel[] compaction and cx_diag scatter: diag(Cx) over all u unknowns (tie variances
    included) and the (u_img + u_cam)^2 correlation block of every image against oracle.covariance, at
    test_gpu_parity._check_cov's bars (1e-8 relative, 5e-9 absolute)."""
    c = _case(fba, oracle, work, scene, mask)
    e_diag, e_corr = None, None
    try:
        e_diag, e_corr = fm.check_cov(c["res"], c["od"], c["ro"], oracle)
    finally:
        own = fm.cov_self_spread(oracle, c["od"], c["ro"])
        print(f"flag-mask covariance {scene} {mask}: diag(Cx) {e_diag} correlations {e_corr}; the oracle's own "
              f"explicit-inverse vs LU spread: diag {own[0]:.2e} correlations {own[1]:.2e}")


@pytest.mark.parametrize("variant", sorted(fm.REF_TEXT_VARIANTS))
def test_adjust_cam0_matches_reference_text_under_mask(fba, work, variant):
    """The HIP path against the reference's own .m text run under a mask, as test_gpu_parity.
    test_adjust_cam0_matches_reference_text holds the pinhole variants: Buildxhat exact, BuildAwG <= 1e-12,
    the iteration count, xhat after every iteration <= 1e-9 per element, deltasum history, sigma0^2, RMS,
    v, RSD, diag(Cx) (1e-9; distortion terms 1e-8) and the correlation blocks (1e-9 absolute)."""
    from conftest import variant_folder
    from test_reference_text import assert_within, check_awg, load_ref, loop_errors
    g = load_ref(variant)
    ds = fba.load_folder(variant_folder(str(work["root"]), variant, fm.REF_TEXT_VARIANTS[variant]))
    ctx = _ctx(fba, ds)
    try:
        x0 = ctx.buildxhat()
        np.testing.assert_array_equal(x0, g["xhat_hist"][0])
        A, w, G, dsc = ctx.build_awg(x0)
        assert A.shape == tuple(g["A0_shape"])
        np.testing.assert_array_equal(dsc[:, :2], g["dist_scaling"][:, :2])
        check_awg(A, w, G, dsc, g, np.abs(ds.xy).max())
        hist, dsum = [x0], []
        for _ in range(int(g["iterations"])):
            dsum.append(ctx.step())
            hist.append(ctx.get_xhat())
        v, rsd, st = ctx.residuals()
    finally:
        ctx.close()
    res = fba.adjust(ds)
    assert res.iterations == int(g["iterations"]) and list(res.xhatnames) == g["names"]
    np.testing.assert_array_equal(res.xhat, hist[-1])
    err = loop_errors(g, hist, dsum, st[3], st[:3], v, rsd, g["dist_scaling"])
    print(f"flag-mask reference text {variant}:", {k: f"{e:.1e}" for k, e in err.items()})
    assert_within(err, "stage3_pinhole", {})
    dist = np.array([nm[0] in "kp" and nm[1:2].isdigit() for nm in g["names"]])
    print(f"flag-mask reference text {variant}: diag(Cx) "
          f"{np.max(np.abs(res.cx_diag - g['cx_diag']) / g['cx_diag']):.1e} correlations "
          f"{np.max(np.abs(res.corr - g['corr_blocks'])):.1e}")
    np.testing.assert_allclose(res.cx_diag[~dist], g["cx_diag"][~dist], rtol=1e-9, atol=0)
    np.testing.assert_allclose(res.cx_diag[dist], g["cx_diag"][dist], rtol=1e-8, atol=0)
    assert res.corr.shape == g["corr_blocks"].shape
    np.testing.assert_allclose(res.corr, g["corr_blocks"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("mask", ["no_xp", "c_only"])
def test_buildrsd_under_mask(fba, oracle, work, mask):
    """fba_build_rsd: xp, yp from xhat where estimated, else the INT values (BuildRSD.m:12-26) -- no_xp: yp
    from xhat (at the index xp would have had), xp from INT; c_only: both from INT."""
    folder = _folder(work, "cam0", mask)
    ds, od = fba.load_folder(folder), oracle.load_folder(folder)
    ro = oracle.adjust(od)
    rows = fba.BuildRSD(ro.v, ds, ro.xhat)
    assert [r[0] for r in rows] == od.target and [r[1] for r in rows] == od.image
    num = np.array([r[4:] for r in rows], dtype=np.float64)
    ref = oracle.build_rsd(od, ro.v, ro.xhat)
    assert np.abs(num - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mask", ["mix_a", "radial_only"])
def test_sharded_ranks_reassemble_single_context_under_mask(fba, work, mask, world):
    """test_gpu_parity.test_sharded_ranks_reassemble_single_gpu_result on the 14 x 260 control scene under a
    mask: `world` rank contexts on one GPU, reduce buffers summed on the host.  The owned-only xhats
    (fba_get_xhat's compression with owned_only) sum to the single context's xhat <= 1e-10 per group and
    the deltasum shares add up."""
    ds = fba.load_folder(_folder(work, "control", mask))
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    single = _ctx(fba, ds)
    ranks = [_ctx(fba, ds, rank=r, world=world) for r in range(world)]
    try:
        d_first = None
        for _ in range(3):
            d1 = single.step()
            d_first = d_first or d1
            for c in ranks:
                c.accumulate()
                c.synchronize()
            bufs = [c.reduce_buffer() for c in ranks]
            total = np.zeros(bufs[0][1])
            for p, n in bufs:
                a = np.empty(n)
                assert hip.hipMemcpy(a.ctypes.data, p, n * 8, 2) == 0
                total += a
            for p, n in bufs:
                assert hip.hipMemcpy(p, total.ctypes.data, n * 8, 1) == 0
            parts = [c.solve_update() for c in ranks]
            assert abs(sum(parts) - d1) <= 1e-7 * d_first
        xs = single.get_xhat()
        owned = [c.get_xhat(owned_only=True) for c in ranks]
        assert all(len(x) == len(xs) for x in owned)
        _, _, _, dsc = single.build_awg(xs)
        err = group_rel_err(sum(owned), xs, fba.xhat_names(ds), dsc)
        assert max(err.values()) <= 1e-10, err
    finally:
        single.close()
        for c in ranks:
            c.close()
