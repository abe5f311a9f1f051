"""CPU: partial Estimate_* flag sets (tests/flag_masks.py) on the restatements and the host side.

* The dense oracle against the reference's OWN .m text run under two masks (tests/golden/
  ref_cam0_mix_a_noic_pinhole.npz, ref_cam0_stage2_pinhole.npz; tests/golden/make_ref_golden.py), held as
  tests/test_reference_text.py holds the pinhole variants.
* oracle/fba_cpu.c (the checker of the full-size GPU tests) against the dense oracle under every mask: the
  same iteration count and names, xhat <= 1e-9 per group and per element (conftest.SMALL_SCENE_FLOOR),
  sigma0^2 <= 1e-9.
* The host side of the HIP path: fba_count_unknowns, fba.xhat_names, and the refusal of inner constraints
  with a fixed EOP before any GPU call.
* The report writers fed with the oracle's mix_a result: the .out lists exactly the estimated rows.
"""
import os

import numpy as np
import pytest

import flag_masks as fm
from conftest import SMALL_SCENE_FLOOR, elem_rel_err, group_rel_err


@pytest.mark.parametrize("variant", sorted(fm.REF_TEXT_VARIANTS))
def test_oracle_matches_reference_text_under_mask(oracle, tmp_path, variant):
    """As test_reference_text.test_oracle_matches_reference_text on its pinhole variants: names and
    Buildxhat exact, BuildAwG (the compact n x u A, dist_scaling's index columns included), the iteration
    count, xhat after every iteration <= 1e-9 per element, deltasum history, sigma0^2, RMS, v, RSD,
    diag(Cx) <= 1e-9 and the (u_img + u_cam)^2 correlation blocks <= 1e-9 absolute."""
    from conftest import variant_folder
    from test_reference_text import assert_within, check_awg, load_ref, loop_errors
    g = load_ref(variant)
    od = oracle.load_folder(variant_folder(str(tmp_path), variant, fm.REF_TEXT_VARIANTS[variant]))
    x0, names = oracle.buildxhat(od)
    assert names == g["names"]
    np.testing.assert_array_equal(x0, g["xhat_hist"][0])
    A, w, G, ds = oracle.build_awg(od, x0)
    assert A.shape == tuple(g["A0_shape"]) == (od.n, len(names))
    np.testing.assert_array_equal(ds[:, :2], g["dist_scaling"][:, :2])
    check_awg(A, w, G, ds, g, max(np.abs(od.x).max(), np.abs(od.y).max()))
    ro = oracle.adjust(od)
    assert ro.iterations == g["iterations"]
    err = loop_errors(g, ro.xhat_hist, ro.deltasum, ro.sigma02, ro.rms, ro.v, ro.rsd, g["dist_scaling"])
    print(f"oracle vs reference text ({variant}):", {k: f"{v:.1e}" for k, v in err.items()})
    assert_within(err, "stage3_pinhole", {})
    cxd, corr = oracle.covariance(od, ro)
    np.testing.assert_allclose(cxd, g["cx_diag"], rtol=1e-9, atol=0)
    u_img, u_cam = oracle.counts(od.settings)
    assert g["corr_blocks"].shape == (od.numImg, u_img + u_cam, u_img + u_cam)
    for e in range(od.numImg):
        idx = fm.cov_index(od, u_img, u_cam, e)
        np.testing.assert_allclose(corr[np.ix_(idx, idx)], g["corr_blocks"][e], rtol=0, atol=1e-9)


def test_masked_fixtures_are_what_main_prints():
    """cam0 under mix_a (Omega, Zc, yp, radial off; no inner constraints): u = 42 x 4 + 4 + 106 x 3 = 490
    and dist_scaling's index columns [0, 171] (no radial unknown; p1 is xhat(171): 168 EOPs + xp + c,
    BuildAwG.m:138, :150).  Under stage2 (radial and decentering off): u = 42 x 6 + 3 + 318 = 573, both 0."""
    from test_reference_text import load_ref
    g = load_ref("mix_a_noic_pinhole")
    assert len(g["names"]) == 490 and g["G0"].size == 0
    np.testing.assert_array_equal(g["dist_scaling"][:, :2], [[0, 171]])
    assert g["names"][:4] == ["Xc_" + g["names"][0][3:], "Yc_" + g["names"][0][3:], "p_" + g["names"][0][3:],
                              "k_" + g["names"][0][3:]]
    assert [n.split("_")[0] for n in g["names"][168:172]] == ["xp", "c", "p1", "p2"]
    g = load_ref("stage2_pinhole")
    assert len(g["names"]) == 573 and g["G0"].shape == (573, 7)
    np.testing.assert_array_equal(g["dist_scaling"][:, :2], [[0, 0]])
    assert [n.split("_")[0] for n in g["names"][252:255]] == ["xp", "yp", "c"]


@pytest.fixture(scope="module")
def fbo():
    import fba_cpu
    fba_cpu.build()
    return fba_cpu


C_ORACLE_CASES = [("control", m, "kkt") for m in sorted(fm.MASKS)] + \
    [("free", m, s) for m in sorted(fm.CAM_MASKS) for s in ("kkt", "chol")]


@pytest.mark.parametrize("scene,mask,solver", C_ORACLE_CASES)
def test_c_oracle_matches_dense_oracle_under_mask(fba, fbo, oracle, tmp_path, scene, mask, solver):
    """oracle/fba_cpu.c against the dense oracle under every mask: the 14 x 260 control scene (no border:
    "kkt" and "chol" are the same Cholesky solve there, so one runs) and the 12 x 240 free network (camera
    masks only; both solvers of the bordered system)."""
    od = oracle.load_folder(fm.synth_folder(tmp_path, scene, mask))
    ro = oracle.adjust(od)
    ca = fbo.CpuAdjustment(od, threads=2, solver=solver)
    try:
        assert ca.names == ro.names and ca.u == len(ro.xhat)
        assert ca.adjust() == ro.iterations
        err = group_rel_err(ca.xhat, ro.xhat, ro.names, ro.dist_scaling)
        assert max(err.values()) <= 1e-9, err
        err = elem_rel_err(ca.xhat, ro.xhat, ro.names, ro.dist_scaling, floor=SMALL_SCENE_FLOOR)
        assert max(err.values()) <= 1e-9, err
        _, s02 = ca.residuals()
        assert abs(s02 - ro.sigma02) <= 1e-9 * ro.sigma02
    finally:
        ca.close()


@pytest.mark.parametrize("mask", sorted(fm.MASKS))
def test_unknown_count_and_names_under_mask(fba, oracle, tmp_path, mask):
    """fba_count_unknowns and fba.xhat_names (the compressed layout at the C-ABI) against Buildxhat.m's,
    on cam0 and on the 2-camera rig."""
    for folder in (fm.cam0_folder(tmp_path, mask), fm.synth_folder(tmp_path, "rig2", mask)):
        ds = fba.load_folder(folder)
        x, names = oracle.buildxhat(oracle.load_folder(folder))
        assert fba.capi.count_unknowns(ds.pack(), fba.capi.make_settings(ds.settings)) == len(x)
        assert fba.xhat_names(ds) == names


@pytest.mark.parametrize("mask", fm.NEEDS_NO_IC)
def test_inner_constraints_with_fixed_eop_refused_before_gpu(fba, mask):
    """Inner constraints need all six EOPs (BuildAwG.m:525): FBA_ERR_UNSUPPORTED from check_settings,
    before any GPU call (this test runs without one)."""
    from conftest import variant_folder
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        ds = fba.load_folder(variant_folder(root, mask, dict(fm.MASKS[mask], Inner_Constraints="1")))
        with pytest.raises(fba.FBAError) as e:
            fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))
        assert e.value.code == 5


@pytest.fixture(scope="module")
def mix_a_outputs(fba, oracle, tmp_path_factory):
    from fba_amd.bundle import Adjustment
    folder = fm.cam0_folder(tmp_path_factory.mktemp("rep"), "mix_a")
    ds = fba.load_folder(folder)
    od = oracle.load_folder(folder)
    ro = oracle.adjust(od)
    cxd, corr = oracle.covariance(od, ro)
    u_img, u_cam = oracle.counts(od.settings)
    blocks = [corr[np.ix_(idx, idx)] for idx in (fm.cov_index(od, u_img, u_cam, e) for e in range(od.numImg))]
    res = Adjustment(xhat=ro.xhat, xhatnames=ro.names, iterations=ro.iterations, deltasum=np.array(ro.deltasum),
                     v=ro.v, rsd=ro.rsd, rms=ro.rms, sigma02=ro.sigma02, seconds=1.25, cx_diag=cxd,
                     corr=np.array(blocks))
    out_dir = str(tmp_path_factory.mktemp("out"))
    path = fba.bundle.write_outputs(ds, res, out_dir)
    return ds, res, path, out_dir


def test_out_report_lists_exactly_the_estimated_rows(mix_a_outputs):
    """main.m:727-818 under mix_a: per image the rows Xc, Yc, Phi, Kappa (no Zc, no Omega), per camera xp,
    c, p1, p2 (no yp, no k1..k5), each with its own xhat entry and sqrt(Cx); Total Unknowns 490; the IOP
    correlation sub-matrix has u_cam = 4 rows."""
    ds, res, path, _ = mix_a_outputs
    lines = open(path).read().splitlines()

    def row(name):
        return next(x for x in lines if x.startswith(name + " .")).split()[-1]
    assert row("Total Unknowns") == "490"
    assert row("Total EOP unknowns") == "168" and row("Total IOP unknowns") == "2"
    assert row("Total distortion unknowns") == "2" and row("Number of Inner Constraints") == "0"
    assert row("Total Degrees of Freedom") == str(ds.n - 490)
    a, b = lines.index("Estimated EOPs"), lines.index("Estimated IOPs and Distortions for each Camera")
    eop_all = ("Xc", "Yc", "Zc", "Omega", "Phi", "Kappa")
    got = [x.split() for x in lines[a + 2:b] if x.split() and x.split()[0] in eop_all and len(x.split()) == 3]
    assert [r[0] for r in got] == ["Xc", "Yc", "Phi", "Kappa"] * ds.numImg
    for q, r in enumerate(got):
        f = 180.0 / np.pi if r[0] in ("Phi", "Kappa") else 1.0
        assert float(r[1]) == pytest.approx(res.xhat[q] * f, abs=1e-5)
        assert float(r[2]) == pytest.approx(np.sqrt(res.cx_diag[q]) * f, abs=1e-5)
    c = lines.index("IOP Correlation sub-matrix")
    iop_all = ("xp", "yp", "c", "k1", "k2", "k3", "k4", "k5", "p1", "p2")
    got = [x.split() for x in lines[b + 2:c] if x.split() and x.split()[0] in iop_all and len(x.split()) == 3]
    assert [r[0] for r in got] == ["xp", "c", "p1", "p2"]
    for j, r in enumerate(got):
        assert float(r[1]) == pytest.approx(res.xhat[168 + j], rel=1e-5, abs=1e-5)
    assert lines[c + 2].split() == ["xp", "c", "p1", "p2"]
    sub = lines[c + 3:c + 7]
    assert [x.split()[0] for x in sub] == ["xp", "c", "p1", "p2"] and [len(x.split()) for x in sub] == [2, 3, 4, 5]
    assert lines[c + 7] == ""
    assert all(float(x.split()[-1]) == 1.0 for x in sub)  # the correlation diagonal


def test_par_has_u_cam_rows_under_mask(mix_a_outputs):
    ds, res, path, out_dir = mix_a_outputs
    name = os.path.splitext(ds.settings["Output_Filename"])[0]
    par = open(os.path.join(out_dir, name + ".par")).read().splitlines()
    assert len(par) == 3 + ds.numCam * (1 + 4)
    assert [r.split("\t")[0] for r in par[3:]] == ["Camera", "xp", "c", "p1", "p2"]
    assert float(par[5].split("\t")[1]) == pytest.approx(res.xhat[169], rel=1e-14)
    assert float(par[5].split("\t")[2]) == pytest.approx(np.sqrt(res.cx_diag[169]), rel=1e-14)
