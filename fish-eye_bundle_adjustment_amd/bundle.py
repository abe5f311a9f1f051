"""Reference-named host API over libfba.so.

The reference's hot path is a set of MATLAB functions plus an inline loop; these wrappers keep
their names, argument meaning and error behaviour (first output = error flag, 0 ok / 1 fail) so a
caller can switch function by function:

    [error, xhat, xhatnames] = Buildxhat(data, ...)            functions/Buildxhat.m:2
    [error, A, misclosure, G, dist_scaling] = BuildAwG(data, xhat)   functions/BuildAwG.m:14
    RSD = BuildRSD(v, data, xhat)                               functions/BuildRSD.m:1
    main_error = main(folder, plot)                             main.m:10

Every numeric result comes from the HIP path (libfba.so); nothing here computes a Jacobian, a
normal matrix or a solve.
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass

import numpy as np

from . import capi
from .io import Dataset, IngestError, load_folder, xhat_names


def _ctx(data: Dataset, device=0, **kw):
    ctx = getattr(data, "_fba_ctx", None)
    if ctx is None or kw:
        ctx = capi.Context(data.pack(), capi.make_settings(data.settings), device=device, **kw)
        if not kw:
            data._fba_ctx = ctx
    return ctx


def Buildxhat(data: Dataset):
    """Buildxhat.m:2 -> (error, xhat, xhatnames)."""
    try:
        ctx = _ctx(data)
        return 0, ctx.buildxhat(), xhat_names(data)
    except capi.FBAError as e:
        print(f"Error Buildxhat(): {e}")
        return 1, None, None


def BuildAwG(data: Dataset, xhat):
    """BuildAwG.m:14 -> (error, A, misclosure, G, dist_scaling); A dense n x u (debug/parity form).

    G is the scalar 0 when inner constraints are off (BuildAwG.m:38); dist_scaling columns 1-2
    carry the reference's 1-based xhat indices of the first radial / decentering unknown."""
    try:
        ctx = _ctx(data)
        A, w, G, ds = ctx.build_awg(np.asarray(xhat, dtype=np.float64))
        return 0, A, w, (G if G is not None else 0), ds
    except capi.FBAError as e:
        print(f"BuildAwG: {e}")
        return 1, None, None, None, None


def BuildRSD(v, data: Dataset, xhat):
    """BuildRSD.m:1-43: rows [targetID, imageID, x, y, r, vx, vy, vr, vt] -- the radial / tangential
    split of a given v, with xp, yp from xhat where estimated (fba_build_rsd on the device)."""
    rsd = _ctx(data).build_rsd(v, xhat)
    return [[data.pho_target[i], data.pho_image[i], data.xy[i, 0], data.xy[i, 1], *rsd[i]] for i in range(len(rsd))]


@dataclass
class Adjustment:
    xhat: np.ndarray
    xhatnames: list
    iterations: int
    deltasum: np.ndarray
    v: np.ndarray
    rsd: np.ndarray          # (n_pts, 5): r vx vy vr vt
    rms: tuple               # RMSx, RMSy, RMS
    sigma02: float
    seconds: float
    cx_diag: np.ndarray = None   # diag of the final Cx (sigma02-scaled, distortions de-scaled)
    corr: np.ndarray = None      # (numImg, u_img+u_cam, u_img+u_cam) EOP/IOP Correlation sub-blocks
    redundancy: np.ndarray = None  # (2 n_pts) redundancy numbers, PHO order, x y interleaved (reliability=True)
    wstat: np.ndarray = None       # (2 n_pts) standardised residuals w = v / (sigma sqrt(r))
    weights: np.ndarray = None     # (2 n_pts) effective weights, user weight x loss factor (weights= / robust=)
    # prior observations of unknowns (priors=): index into xhat, observed value, std (xhat's units), the residual
    # v = xhat[index] - value, and with a covariance the redundancy number r = 1 - cx_diag[index] / (sigma02 std^2)
    # and the test statistic w = v / (std sqrt(r)), 0 where r < report.R_MIN
    prior_index: np.ndarray = None
    prior_value: np.ndarray = None
    prior_sigma: np.ndarray = None
    prior_v: np.ndarray = None
    prior_r: np.ndarray = None
    prior_w: np.ndarray = None
    # method="lm": one row per trial and polish pass of fba_adjust_lm -- lambda, cost after it, deltasum, accepted
    lm_history: np.ndarray = None
    # point precision (point_precision=True), TIE order: every tie point's full 3 x 3 block of the final Cx, the
    # 1-sigma semi-axes a >= b >= c of its error ellipsoid and the three unit axis vectors as rows
    cx_tie: np.ndarray = None      # (n_tie, 3, 3), full symmetric
    ell_axes: np.ndarray = None    # (n_tie, 3)
    ell_dirs: np.ndarray = None    # (n_tie, 3, 3)
    # forward intersection of the starting values (intersect=True), TIE order: the intersected X Y Z, per point
    # [rays used, lambda_min / lambda_max, RMS px linear, RMS px refined], and FBA_ISECT_* (capi.ISECT_STATUS)
    isect_xyz: np.ndarray = None      # (n_tie, 3)
    isect_quality: np.ndarray = None  # (n_tie, 4)
    isect_status: np.ndarray = None   # (n_tie)
    # space resection of the starting values (resect=...), EXT order: the resected Xc Yc Zc omega phi kappa, per image
    # [points used, lambda_1 / lambda_11, RMS px linear, RMS px refined, share in front], FBA_RESECT_*
    # (capi.RESECT_STATUS)
    resect_eop: np.ndarray = None      # (n_img, 6)
    resect_quality: np.ndarray = None  # (n_img, 5)
    resect_status: np.ndarray = None   # (n_img)
    # variance component estimation (vce=...): per group (then the rows of no group, then the priors: reported only)
    # the cumulative variance factor relative to the starting weights, the a-posteriori standard deviation
    # sqrt(component) x Meas_std in pixels (Meas_std_y for a group of y rows only; nan for the two report entries), the
    # per-round table [R, T, n, sigma2], FBA_VCE_* of the last round (capi.VCE_STATUS), the rounds and the names
    vce_component: np.ndarray = None   # (n_groups + 2)
    vce_sigma: np.ndarray = None       # (n_groups + 2)
    vce_table: np.ndarray = None       # (rounds, n_groups + 2, 4)
    vce_status: np.ndarray = None      # (n_groups + 2)
    vce_rounds: int = None
    vce_names: list = None
    vce_converged: bool = None
    # data snooping (snoop=...), PHO order: per image point 0 active / 1 excluded / 2 re-admitted (capi.SNOOP_STATE),
    # W (or W~ of an excluded point) of the last round, the per-round table [picked, passed by the back-check,
    # excluded after the round, largest active W], and sigma0^2 over the active rows alone:
    # v'Pv / (n - 2 n_excluded + n_prior - u, + 7 with inner constraints)
    snoop_excluded: np.ndarray = None  # (n_pts) uint8
    snoop_stat: np.ndarray = None      # (n_pts)
    snoop_table: np.ndarray = None     # (rounds, 4)
    snoop_rounds: int = None
    snoop_converged: bool = None
    sigma02_active: float = None


def _priors_of(data, priors):
    """adjust()'s priors argument -> (index, value, sigma) or None; True means the folder's .pri table"""
    if priors is None or priors is False:
        return None
    if priors is True:
        if getattr(data, "priors_error", ""):
            raise IngestError(data.priors_error)
        if getattr(data, "priors", None) is None:
            raise IngestError(f"priors requested but there is no .pri file in {data.folder}")
        return data.priors
    return priors


def prior_statistics(sigma02, cx_diag, index, sigma, v):
    """A prior's own redundancy number r = 1 - cx_diag[index] / (sigma02 sigma^2) -- 1 - p (a Cx a') of its unit
    row, from the final Cx's diagonal -- and its test statistic w = v / (sigma sqrt(r)), 0 where r < 1e-10
    (host arithmetic on fba_covariance's output; fba_reliability's convention for an uncheckable observation)"""
    r = 1.0 - np.asarray(cx_diag)[index] / (sigma02 * sigma ** 2)
    ok = r >= 1e-10
    return r, np.where(ok, v / (sigma * np.sqrt(np.where(ok, r, 1.0))), 0.0)


def vce_groups(packed, vce):
    """adjust()'s vce argument -> (group (2 n_pts) int32, names): "xy" one group per axis, "camera" one per camera,
    "camera_xy" one per camera and axis, or (group_array, names) as given (ids in [0, len(names)) or -1)"""
    n = packed.n_pts
    cam = np.asarray(packed.cam, dtype=np.int32)
    g = np.zeros((n, 2), dtype=np.int32)
    if isinstance(vce, str):
        if vce == "xy":
            g[:, 1] = 1
            names = ["x", "y"]
        elif vce == "camera":
            g[:] = cam[:, None]
            names = [f"cam{k}" for k in range(packed.n_cam)]
        elif vce == "camera_xy":
            g[:, 0], g[:, 1] = 2 * cam, 2 * cam + 1
            names = [f"cam{k}.{a}" for k in range(packed.n_cam) for a in "xy"]
        else:
            raise ValueError(f"adjust: unknown vce {vce!r} (\"xy\", \"camera\", \"camera_xy\" or (group, names))")
        return g.reshape(-1), names
    try:
        arr, names = vce
    except (TypeError, ValueError):
        raise ValueError("adjust: vce must be \"xy\", \"camera\", \"camera_xy\" or (group_array, names)") from None
    g = np.ascontiguousarray(arr, dtype=np.int32).reshape(-1)
    if g.size != 2 * n:
        raise ValueError("adjust: the vce group array must have 2*n_pts entries")
    return g, [str(x) for x in names]


def adjust(data: Dataset, weights=None, robust=None, robust_k=None, device=0, verbose=False, covariance=True,
           reliability=False, priors=None, method="gn", lm_options=None, point_precision=False,
           intersect=False, resect=False, vce=None, vce_options=None, snoop=None) -> Adjustment:
    """main.m:386-602 on one GPU: Buildxhat, the Gauss-Newton loop, residuals, sigma0^2 and (with
    covariance=True) the post-fit Cx diagonal and correlation sub-blocks (main.m:428-482, :602).
    reliability=True calls fba_reliability instead of fba_covariance: the same two outputs plus the
    redundancy numbers and standardised residuals of the image measurements.

    No reference counterpart: weights ((2 n_pts), PHO order, x y interleaved) multiply the a-priori weights
    (fba_set_weights); robust ("huber" / "cauchy", robust_k in units of sigma, default capi.LOSS_K) first
    iterates with L2 to the reference's stopping rule -- at the starting values every misclosure is large and a
    loss would down-weight everything -- then sets the loss and continues under the same threshold and the
    remaining Iteration_Cap.  Residuals, sigma0^2, covariance and reliability are those of the final,
    re-weighted state; Adjustment.weights holds the effective weights.

    priors (no reference counterpart): None, True (the folder's .pri table, data.priors) or (index, value, sigma)
    -- prior observations of unknowns, index into xhat, value and standard deviation in xhat's units
    (fba_create_priors).  sigma0^2 then counts them (v'Pv and the degrees of freedom), and Adjustment.prior_*
    carry their residuals, redundancy numbers and test statistics.

    method (no reference counterpart): "gn" is the reference's loop; "lm" replaces the L2 loop by fba_adjust_lm --
    Levenberg-Marquardt trials with step control from the starting values, then undamped passes to the reference's
    stopping rule -- for coarse starting values; lm_options: a capi.LMOptions or a dict of its fields.  iterations
    and deltasum then count every trial and polish pass, Adjustment.lm_history holds the loop's table, and robust=
    continues from there as it does after the Gauss-Newton loop.

    point_precision (no reference counterpart: main.m:460-482 keeps the diagonal of Cx): fba_postfit_outputs in
    place of fba_covariance / fba_reliability -- the same outputs (reliability's too when that is asked for), plus
    every tie point's full 3 x 3 covariance block and 1-sigma error ellipsoid: Adjustment.cx_tie, ell_axes,
    ell_dirs.

    intersect (no reference counterpart: Buildxhat.m:107-134 copies the .cnt coordinates): before the loop, "gn" or
    "lm", every tie point is intersected from its image rays at the starting exterior and interior orientation
    (fba_intersect with write_xhat: linear line intersection, then point-only Gauss-Newton) and replaces its .cnt
    starting value; a point with fewer than two usable rays or too flat an intersection keeps it.
    Adjustment.isect_xyz, isect_quality and isect_status carry the result.

    resect (no reference counterpart: Buildxhat.m:22-63 copies the .ext rows): True or "control" -- before the
    intersection and the loop, "gn" or "lm", every image is resected from its control points and their measured rays
    (fba_resect with write_xhat: a linear ray-based solution, then Gauss-Newton on the image's six unknowns) and
    replaces its .ext starting values; "all" also uses the tie observations at their .cnt coordinates.  An image
    with fewer than six usable points or points too close to a plane keeps its .ext values.  With intersect=True
    the chain resection, intersection, adjustment starts a block from control points and measurements alone.
    Adjustment.resect_eop, resect_quality and resect_status carry the result.

    vce (no reference counterpart: main.m:397-402 fixes the weights): "xy", "camera", "camera_xy" or (group_array,
    names) -- variance component estimation over groups of image measurements (fba_vce; vce_options: a dict of
    capi.Context.vce's max_rounds, tol, min_redundancy, clip).  It runs after resect / intersect; with method="lm"
    after the damped loop, otherwise in place of the plain loop.  sigma0^2, Cx, the reliability numbers and the
    ellipsoids then come from the re-weighted last pass, Adjustment.weights holds the weights and Adjustment.vce_*
    the components.  Priors keep their stated accuracy: the groups are estimated relative to it.  Together with
    robust= it raises ValueError (the loss factor and a variance component would fight over the same residuals).

    snoop (no reference counterpart: main.m never tests a measurement): True, a critical value, or a dict of
    capi.Context.snoop's options -- Baarda data snooping on the device (fba_snoop): the image points whose w-test
    exceeds crit are eliminated round by round (weight 1e-12 x theirs) and re-checked once the adjustment is clean.
    It runs after resect / intersect; with method="lm" after the damped loop, otherwise in place of the plain loop;
    before vce, where the excluded rows join no group (id -1).  The call consumes the last factor, so one further
    step precedes the post-fit outputs.  sigma0^2, Cx and the reliability numbers are those of the cleaned last pass;
    Adjustment.snoop_* carry the states, statistics and rounds, Adjustment.sigma02_active the variance factor over the
    active rows alone (sigma02 still counts every row).  Together with robust= it raises ValueError."""
    if vce is not None and robust:
        raise ValueError("adjust: vce together with robust is not supported")
    if snoop is False:
        snoop = None
    if snoop is not None and robust:
        raise ValueError("adjust: snoop together with robust is not supported")
    if snoop is not None:
        snoop = {} if snoop is True else dict(snoop) if isinstance(snoop, dict) else {"crit": float(snoop)}
    if resect not in (False, None, True, "control", "all"):
        raise ValueError(f"adjust: unknown resect {resect!r} (True, \"control\" or \"all\")")
    if method not in ("gn", "lm"):
        raise ValueError(f"adjust: unknown method {method!r} (\"gn\" or \"lm\")")
    t0 = time.perf_counter()
    pri = _priors_of(data, priors)
    ctx = capi.Context(data.pack(), capi.make_settings(data.settings), device=device, verbose=verbose, priors=pri)
    try:
        if weights is not None:
            ctx.set_weights(weights)
        lmh = None
        ikw = {}
        if resect:
            re, rq, rst, _ = ctx.resect(use="all" if resect == "all" else "control", write_xhat=True)
            ikw = dict(resect_eop=re, resect_quality=rq, resect_status=rst)
        if intersect:
            ix, iq, ist, _ = ctx.intersect(write_xhat=True)
            ikw.update(isect_xyz=ix, isect_quality=iq, isect_status=ist)
        if method == "lm":
            nt, npol, lmh = ctx.adjust_lm(lm_options)
            it, hist = nt + npol, lmh[:, 2].copy()
        elif vce is None and snoop is None:
            it, hist = ctx.adjust()
        else:
            it, hist = 0, np.zeros(0)
        skw = {}
        if snoop is not None:
            sn = ctx.snoop(**snoop)
            it += sn["iterations"]
            skw = dict(snoop_excluded=sn["excluded"], snoop_stat=sn["stat"], snoop_table=sn["table"],
                       snoop_rounds=sn["rounds"], snoop_converged=sn["converged"])
            if vce is None and (covariance or reliability or point_precision):
                ctx.step()  # fba_snoop consumed the factor of its last solve
                it += 1
        vkw = {}
        if vce is not None:
            grp, names = vce_groups(ctx.packed, vce)
            if snoop is not None:
                grp = np.where(np.repeat(skw["snoop_excluded"] == 1, 2), -1, grp).astype(np.int32)
            vr = ctx.vce(grp, len(names), **(vce_options or {}))
            it += vr["iterations"]
            std = np.full(len(names) + 2, np.nan)
            for gi in range(len(names)):
                rows = np.nonzero(grp == gi)[0]
                only_y = rows.size > 0 and bool(np.all(rows % 2 == 1))
                std[gi] = float(ctx.settings.meas_std_y if only_y else ctx.settings.meas_std_x)
            vkw = dict(vce_component=vr["component"], vce_sigma=np.sqrt(vr["component"]) * std, vce_table=vr["table"],
                       vce_status=vr["status"], vce_rounds=vr["rounds"], vce_names=names + ["(no group)", "(priors)"],
                       vce_converged=vr["converged"])
        if robust:
            ctx.set_loss(robust, robust_k)
            cap, thr = max(int(ctx.settings.iteration_cap), 1), float(ctx.settings.threshold)
            more, deltasum = [], 100.0  # main.m:407, :412, :490-493 again, on what the L2 loop left of the cap
            while deltasum > thr and it + len(more) < cap:
                deltasum = ctx.step()
                more.append(deltasum)
            it, hist = it + len(more), np.concatenate([hist, more])
        t1 = time.perf_counter()
        xhat = ctx.get_xhat()
        v, rsd, st = ctx.residuals()
        eff = ctx.get_weights() if (weights is not None or robust or vce is not None or snoop is not None) else None
        if snoop is not None:
            n_ex = int(np.count_nonzero(skw["snoop_excluded"] == 1))
            dof = st[5] - 2 * n_ex + (7 if int(data.settings.get("Inner_Constraints", 0)) else 0)
            skw["sigma02_active"] = float(st[4] / dof) if dof > 0 else float("nan")
        red = wst = None
        ppk = {}
        if point_precision:
            cxd, corr, red, wst, blk, ell = ctx.postfit(st[3], reliability=reliability)
            ppk = dict(cx_tie=capi.tie_blocks(blk), ell_axes=ell[:, :3].copy(), ell_dirs=ell[:, 3:].reshape(-1, 3, 3).copy())
        elif reliability:
            cxd, corr, red, wst = ctx.reliability(st[3])
        else:
            cxd, corr = ctx.covariance(st[3]) if covariance else (None, None)
        pkw = {}
        if ctx.priors is not None:
            pi, pl, ps = ctx.priors
            pv = ctx.get_priors()[0]
            pr, pw = prior_statistics(st[3], cxd, pi, ps, pv) if cxd is not None else (None, None)
            pkw = dict(prior_index=pi, prior_value=pl, prior_sigma=ps, prior_v=pv, prior_r=pr, prior_w=pw)
    finally:
        ctx.close()
    return Adjustment(xhat=xhat, xhatnames=xhat_names(data), iterations=it, deltasum=hist, v=v, rsd=rsd,
                      rms=(st[0], st[1], st[2]), sigma02=st[3], seconds=t1 - t0, cx_diag=cxd, corr=corr,
                      redundancy=red, wstat=wst, weights=eff, lm_history=lmh, **pkw, **ppk, **ikw, **vkw, **skw)


def write_outputs(data: Dataset, res: Adjustment, folder):
    """main.m:631-958: the .out report, the .rsd residual table and the .par camera file
    (fba_amd/report.py)."""
    from . import report
    name = os.path.splitext(data.settings["Output_Filename"])[0]
    out = os.path.join(folder, data.settings["Output_Filename"])
    par = report.write_out(out, data, res, res.seconds)
    report.write_rsd(os.path.join(folder, name + ".rsd"), data, res.rsd)
    report.write_par(os.path.join(folder, name + ".par"), par)
    if res.redundancy is not None:
        report.write_rel(os.path.join(folder, name + ".rel"), data, res)
    if res.weights is not None:
        report.write_wgt(os.path.join(folder, name + ".wgt"), data, res)
    if res.prior_index is not None:
        report.write_prr(os.path.join(folder, name + ".prr"), data, res)
    if res.lm_history is not None:
        report.write_lm(os.path.join(folder, name + ".lm"), res.lm_history)
    if getattr(res, "ell_axes", None) is not None:
        report.write_ell(os.path.join(folder, name + ".ell"), data, res)
    if getattr(res, "isect_status", None) is not None:
        report.write_fwd(os.path.join(folder, name + ".fwd"), data, res)
    if getattr(res, "resect_status", None) is not None:
        report.write_rsc(os.path.join(folder, name + ".rsc"), data, res)
    if getattr(res, "vce_component", None) is not None:
        report.write_vce(os.path.join(folder, name + ".vce"), res)
    if getattr(res, "snoop_excluded", None) is not None:
        report.write_snp(os.path.join(folder, name + ".snp"), data, res)
    return out


def main(folder: str = "", plot: bool = False, device=0, reliability=False, robust=None, robust_k=None,
         priors=False, method="gn", lm_options=None, ellipsoids=False, intersect=False, resect=False, vce=None,
         snoop=None) -> int:
    """main.m:10 contract: returns main_error (0 ok, 1 failure).  Plots (main.m:502-584) are not
    produced; `plot` is accepted for signature compatibility.  reliability=True also writes the .rel
    table (report.write_rel) beside the .out / .par / .rsd files, which stay as without it.  robust / robust_k:
    adjust()'s robust loss; the .wgt table (report.write_wgt) is written too.  priors=True: the folder's .pri
    table as prior observations of unknowns (io.read_pri; without the file main returns 1); the .prr table
    (report.write_prr) is written too.  method="lm" (lm_options: adjust()'s): the damped loop of fba_adjust_lm
    in place of the Gauss-Newton loop; the .lm table (report.write_lm) is written too.  ellipsoids=True:
    adjust()'s point_precision; the .ell table (report.write_ell) is written too.  intersect=True: adjust()'s
    intersect -- the tie points' starting values from their image rays instead of the .cnt file; the .fwd table
    (report.write_fwd) is written too.  resect=True / "control" / "all": adjust()'s resect -- the images' starting
    values by space resection instead of the .ext file; the .rsc table (report.write_rsc) is written too.
    vce="xy" / "camera" / "camera_xy": adjust()'s vce -- variance components of the image measurements' groups; the
    .vce table (report.write_vce) is written too.  snoop=True / a critical value: adjust()'s snoop -- Baarda data
    snooping of the image points; the .snp table (report.write_snp) is written too."""
    project_dir = os.getcwd()
    folder = folder or project_dir
    try:
        data = load_folder(folder, project_dir=None if folder == project_dir else project_dir)
        res = adjust(data, device=device, reliability=reliability, robust=robust, robust_k=robust_k,
                     **({"priors": True} if priors else {}),
                     **({"point_precision": True} if ellipsoids else {}),
                     **({"intersect": True} if intersect else {}),
                     **({"resect": resect} if resect else {}),
                     **({"vce": vce} if vce else {}),
                     **({"snoop": snoop} if snoop else {}),
                     **({"method": method, "lm_options": lm_options} if method != "gn" else {}))
        write_outputs(data, res, folder)
    except (IngestError, capi.FBAError) as e:
        print(f"Error: {e}")
        return 1
    return 0
