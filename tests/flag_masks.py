"""Partial Estimate_* flag sets (helper module, no tests).

The device code keeps every unknown in a full parameter space (6 EOPs per image, 5 + nK camera terms per
camera, 3 coordinates per tie point) and applies the .cfg's Estimate_* flags through Jacobian masks, a unit
diagonal in the reduced system and a compression at the C-ABI (csrc/fba_internal.h:3-8).  The reference
implements every flag on its own (BuildAwG.m:56-92, :113-155, :220-445; Buildxhat.m; main.m:460-482,
:727-818).  The masks here are .cfg edits -- keys and value strings as in the .cfg -- so one table serves
conftest.variant_folder (cam0) and synth.write_folder(cfg_overrides=...).
"""
import os

import numpy as np

from conftest import ELEM_FLOOR, elem_rel_err, group_rel_err, solver_spread, variant_folder

_SHORT = {"Xc": "Estimate_Xc", "Yc": "Estimate_Yc", "Zc": "Estimate_Zc", "Omega": "Estimate_Omega",
          "Phi": "Estimate_Phi", "Kappa": "Estimate_Kappa", "xp": "Estimate_xp", "yp": "Estimate_yp",
          "c": "Estimate_c", "radial": "Estimate_Radial_Distortions", "decent": "Estimate_Decentering_Distortions"}


def _off(*short):
    return {_SHORT[s]: "0" for s in short}


# a fixed EOP needs Inner_Constraints 0: check_settings returns FBA_ERR_UNSUPPORTED otherwise (BuildAwG.m:525)
EOP_MASKS = {
    "no_omega": _off("Omega"),
    "no_Zc_kappa": _off("Zc", "Kappa"),
    "pos_only": _off("Omega", "Phi", "Kappa"),
    "ang_only": _off("Xc", "Yc", "Zc"),
}
# valid with or without inner constraints
CAM_MASKS = {
    "no_xp": _off("xp"),
    "no_xp_yp": _off("xp", "yp"),
    "c_only": _off("xp", "yp", "radial", "decent"),
    "radial_only": _off("xp", "yp", "c", "decent"),
    "decent_only": _off("xp", "yp", "c", "radial"),
    "no_radial": _off("radial"),
    "no_decent": _off("decent"),
    "stage2": _off("radial", "decent"),
    "c_k_only": _off("xp", "yp", "decent"),
}
MIXED_MASKS = {
    "mix_a": _off("Omega", "Zc", "yp", "radial"),
    "mix_b": _off("Phi", "Xc", "xp", "c", "decent"),
    "eop_kappa_off": _off("Kappa", "xp", "yp", "c", "radial", "decent"),
}
MASKS = {**EOP_MASKS, **CAM_MASKS, **MIXED_MASKS}
NEEDS_NO_IC = sorted(EOP_MASKS) + sorted(MIXED_MASKS)

# the reference-text fixtures under a mask (tests/golden/ref_cam0_<name>.npz, make_ref_golden.py <ref> <name>)
REF_TEXT_VARIANTS = {
    "mix_a_noic_pinhole": {"Inner_Constraints": "0", **MASKS["mix_a"]},
    "stage2_pinhole": dict(MASKS["stage2"]),
}


def cam0_edits(mask):
    """cam0's .cfg edits for a mask: Inner_Constraints 0 where an EOP is fixed (cam0 has 3 control points)"""
    edits = dict(MASKS[mask])
    if mask in NEEDS_NO_IC:
        edits["Inner_Constraints"] = "0"
    return edits


def cam0_folder(root, mask):
    return variant_folder(str(root), "cam0_" + mask, cam0_edits(mask))


_SCENES = {}


def _scene(key):
    """synth.generate is deterministic; one scene per session, written once per mask"""
    if key not in _SCENES:
        from fba_amd import synth
        if key == "control":   # datum from 12 control points, no inner constraints: every mask is valid
            _SCENES[key] = synth.generate(14, 260, seed=23, typ="fisheye", n_control=12)
        elif key == "free":    # free network, inner constraints on (the border path): camera masks only
            _SCENES[key] = synth.generate(12, 240, seed=17)
        elif key == "rig2":    # tests/test_gpu_general.py SCENES["rig2"]: every point through both cameras
            _SCENES[key] = synth.generate(18, 300, seed=41, n_cam=2)
        elif key == "dup":     # tests/test_gpu_general.py SCENES["dup"]: repeated measurements
            _SCENES[key] = synth.generate(16, 300, seed=41, n_dup=30)
        elif key == "rig2_control":
            _SCENES[key] = synth.generate(18, 300, seed=41, n_cam=2, n_control=12)
        elif key == "dup_control":
            _SCENES[key] = synth.generate(16, 300, seed=41, n_dup=30, n_control=12)
        else:
            raise KeyError(key)
    return _SCENES[key]


def synth_folder(root, scene, mask):
    """scene in control / free / rig2 / dup, written with the mask's flags.  rig2 and dup are free networks
    (inner constraints on), which a fixed EOP rules out (BuildAwG.m:525), and fixed EOPs alone do not hold
    the datum (with Omega and Zc fixed, X / Y shifts and the rotation about Z stay free): under a mask that
    fixes an EOP their first 12 points are control points, as in the control scene, and write_folder then
    switches the inner constraints off."""
    from fba_amd import synth
    if scene == "free" and mask in NEEDS_NO_IC:
        raise ValueError("the free network takes camera masks only")
    if scene in ("rig2", "dup") and mask in NEEDS_NO_IC:
        scene += "_control"
    return synth.write_folder(_scene(scene), os.path.join(str(root), f"{scene}_{mask}"), cfg_overrides=MASKS[mask])


def errors(xhat, sigma02, deltasum0, ro, floor=ELEM_FLOOR):
    """per-group, per-element ("e_<group>"), sigma0^2 and first-deltasum errors, keyed as solver_spread"""
    err = group_rel_err(xhat, ro.xhat, ro.names, ro.dist_scaling)
    err.update({"e_" + g: v for g, v in elem_rel_err(xhat, ro.xhat, ro.names, ro.dist_scaling, floor).items()})
    err["sigma02"] = abs(sigma02 - ro.sigma02) / ro.sigma02
    err["deltasum0"] = abs(deltasum0 - ro.deltasum[0]) / ro.deltasum[0]
    return err


def bars(oracle, od, ro, floor=ELEM_FLOOR):
    """The per-mask bar, as test_gpu_parity.test_adjust_cam0 holds cam0: 1e-9, or 20x the spread of the
    reference restatement against itself under rounding-level changes (conftest.solver_spread) where that
    is larger.  Returns (bar per key, spread per key).

    "deltasum_hist": the same rule for every later deltasum, on the scale of the first (as
    test_gpu_general holds the history): per pass, how far the oracle's explicit bordered inverse
    (main.m:432) and an LU solve of the same system land apart.  With inner constraints the second pass of
    the free network moves by up to 1.5e-9 of the first deltasum between them (radial_only; the C oracle's
    two solvers agree with the LU solve there to 1e-11 and the HIP path lands 1.5e-9 from the explicit inverse
    as well, profiles/flag_masks_gpu_errors.log, so the explicit inverse is the outlier), elsewhere by
    <= 4e-10."""
    spread = solver_spread(oracle, od, ro, floor=floor)
    bar = {k: max(1e-9, 20 * s) for k, s in spread.items()}

    def solve_lu(data, A, w, G, P):
        u = A.T @ (P * w)
        N = A.T @ (P[:, None] * A)
        if G is not None:
            N = np.block([[N, G], [G.T, np.zeros((G.shape[1], G.shape[1]))]])
            u = np.concatenate([u, np.zeros(G.shape[1])])
        return np.linalg.solve(N, -u)[: A.shape[1]]
    lu = oracle.adjust(od, solver=solve_lu)
    assert lu.iterations == ro.iterations
    spread["deltasum_hist"] = np.abs(np.array(lu.deltasum) - np.array(ro.deltasum)) / ro.deltasum[0]
    bar["deltasum_hist"] = np.maximum(1e-9, 20 * spread["deltasum_hist"])
    return bar, spread


def cov_index(od, u_img, u_cam, e):
    """rows of Cx in image e's correlation block: its u_img EOPs, then its camera's u_cam IOPs
    (main.m:845-863)"""
    idx = list(range(e * u_img, (e + 1) * u_img))
    k = int(od.cam_num[np.nonzero(od.ext_index == e)[0][0]])
    return idx + list(range(u_img * od.numImg + k * u_cam, u_img * od.numImg + (k + 1) * u_cam))


def cov_self_spread(oracle, od, ro):
    """The oracle's own spread on the covariance: its explicit inverse (numpy's inv, an LU inverse as
    MATLAB's, main.m:428-444) against a second exact route to the inverse of the same bordered matrix, the
    symmetric-indefinite factorisation solved against the identity (numpy's solve against the identity is
    the very same LU and differs by nothing) -- before the diagonal de-scaling and the sigma0^2 factor,
    which are common to both.  Returns (diag(Cx) relative, correlation absolute)."""
    import scipy.linalg as sla
    P = oracle.weights(od)
    _, Cx = oracle.solve_dense(od, ro.A, ro.w, ro.G, P)
    N = ro.A.T @ (P[:, None] * ro.A)
    if od.settings["Inner_Constraints"]:
        d = ro.G.shape[1]
        N = np.block([[N, ro.G], [ro.G.T, np.zeros((d, d))]])
    Cl = sla.solve(N, np.eye(len(N)), assume_a="sym")[: len(Cx), : len(Cx)]
    s, sl = np.sqrt(np.diag(Cx)), np.sqrt(np.diag(Cl))
    return (float(np.max(np.abs(np.diag(Cl) - np.diag(Cx)) / np.diag(Cx))),
            float(np.max(np.abs(Cl / np.outer(sl, sl) - Cx / np.outer(s, s)))))


def check_cov(res, od, ro, oracle, rtol=1e-8, atol_corr=5e-9):
    """test_gpu_parity._check_cov for u_img <= 6 and u_cam <= 5 + nK: diag(Cx) over the u estimated
    unknowns (tie variances included) and each image's (u_img + u_cam)^2 correlation block of
    fba_covariance against the oracle's dense bordered inverse (main.m:428-482, :602).  Bars as there:
    1e-8 relative on diag(Cx), 5e-9 absolute on the correlations (measured under the masks: <= 6.3e-10 and
    <= 1.2e-10, profiles/flag_masks_gpu_errors.log).  Returns the two measured worst errors."""
    cdo, corro = oracle.covariance(od, ro)
    u_img, u_cam = oracle.counts(od.settings)
    assert res.cx_diag.shape == cdo.shape == (len(ro.xhat),)
    assert res.corr.shape == (od.numImg, u_img + u_cam, u_img + u_cam)
    n_tie_unknowns = len(ro.xhat) - u_img * od.numImg - u_cam * od.numCam
    assert n_tie_unknowns > 0 and (cdo[-n_tie_unknowns:] > 0).all()
    e_diag = float(np.max(np.abs(res.cx_diag - cdo) / np.abs(cdo)))
    e_corr = 0.0
    for e in range(od.numImg):
        idx = cov_index(od, u_img, u_cam, e)
        e_corr = max(e_corr, float(np.max(np.abs(res.corr[e] - corro[np.ix_(idx, idx)]))))
    print(f"covariance: diag(Cx) max relative error {e_diag:.2e}, correlation blocks max absolute error {e_corr:.2e}")
    np.testing.assert_allclose(res.cx_diag, cdo, rtol=rtol, atol=0)
    for e in range(od.numImg):
        idx = cov_index(od, u_img, u_cam, e)
        np.testing.assert_allclose(res.corr[e], corro[np.ix_(idx, idx)], rtol=0, atol=atol_corr)
    return e_diag, e_corr
