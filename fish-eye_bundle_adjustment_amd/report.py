"""Report writers of the reference: the .out summary, the .par camera file and the .rsd residual table.

Restates main.m:631-958 (with functions/printCell.m and main.m's printEOP / printDist / printTIE /
countImagePoints / countTargetImages helpers) so the files a reference user reads come out in the same
layout, from the device results (``bundle.Adjustment``: xhat, the diagonal of the final Cx and the
EOP/IOP correlation sub-blocks from ``fba_covariance``, the residuals of ``fba_residuals``).  Reference
quirks kept on purpose: the "Version:" heading runs into the title line, names
in the EOP/IOP tables are cut to 5 characters (``%-W.5s``), the mean-correlation labels shift by one
after the EOP names (an empty name sits between the EOP and IOP name lists, main.m:847), and
``img_width`` takes the last image ID longer than the longest target ID (main.m:697-703).
Host-side text formatting only; nothing here computes on the device path.
"""
import datetime
import math

import numpy as np

LINE = "*" * 109  # main.m:635
DECIMALS = 5      # main.m:686
PADDING = 4       # main.m:634
VERSION = "fba_amd 1 (MI355X HIP path)"
MDB_DELTA0 = 4.13   # Baarda's non-centrality parameter for alpha0 = 0.1 %, beta0 = 80 % (write_rel's mdb)
W_CRITICAL = 3.29   # two-sided 0.1 % point of the standard normal distribution (write_rel's flag)
R_MIN = 1e-10       # below it an observation cannot be checked (fba_reliability reports w = 0)
WGT_FLAG = 0.5      # write_wgt stars a row with an effective weight below it
ELL_K95 = 2.7955    # sqrt(7.8147), the 0.95 point of chi-square with 3 degrees of freedom: 1-sigma axes -> 95 % region
PRODUCER = "fba_amd, the MI355X-native HIP implementation (not the MATLAB reference)"


def num2str(x, prec=None):
    """MATLAB num2str for a real scalar (or a char array passed through)."""
    if isinstance(x, str):
        return x
    x = float(x)
    if prec is not None:
        return _g(x, prec)
    if math.isfinite(x) and x == int(x) and abs(x) < 1e15:
        return str(int(x))
    if not math.isfinite(x):
        return "NaN" if math.isnan(x) else ("Inf" if x > 0 else "-Inf")
    digits = max(int(math.floor(math.log10(abs(x)))) + 5, 5) if x != 0 else 5
    return _g(x, min(digits, 16))


def _g(x, prec):
    s = f"{x:.{prec}g}"
    return s


def print_cell(fh, rows, prefix="", padding=PADDING):
    """functions/printCell.m: 'name ..... value' rows; '\\line' rows print dashes, '\\n' rows a blank."""
    width = max((len(r[0]) for r in rows), default=0)
    for name, val in rows:
        if name == "\\line":
            fh.write("-" * (width + padding + 6))
        elif name == "\\n":
            pass
        else:
            fh.write(prefix + name + " " + "." * (width + padding - len(name)) + " " + num2str(val))
        fh.write("\n")
    return width + padding + 3


def _settings_rows(s):
    """fieldnames(data.settings) in the order main.m:116-171 assigns them (Meas_std_y removed when it
    was not given, main.m:399)."""
    keys = ["Output_Filename", "Meas_std"]
    if not s.get("no_std_y", 0):
        keys.append("Meas_std_y")
    keys += ["no_std_y", "type", "Check_Points", "Iteration_Cap", "threshold", "Inner_Constraints", "Estimate_Xc",
             "Estimate_Yc", "Estimate_Zc", "Estimate_w", "Estimate_p", "Estimate_k", "Estimate_c", "Estimate_xp",
             "Estimate_yp", "Estimate_radial", "Num_Radial_Distortions", "Estimate_decent", "Estimate_tie",
             "Estimate_AllGCP"]
    return [(k, s.get(k, 0)) for k in keys]


def _line_eop(name, value, std, w):
    """printEOP: '%-W.5s%-W.5f%-W.5f'."""
    return f"{name[:DECIMALS]:<{w}}{value:<{w}.{DECIMALS}f}{std:<{w}.{DECIMALS}f}\n"


def _line_dist(name, value, std, w):
    """printDist: '%-W.5s%-W.5e%-W.5e'."""
    return f"{name[:DECIMALS]:<{w}}{value:<{w}.{DECIMALS}e}{std:<{w}.{DECIMALS}e}\n"


def _corr_rows(fh, names, mat):
    """'%-6.2s' name header, then the lower triangle '%-+6.2f' (main.m:802-815)."""
    for nm in names:
        fh.write(f"{nm[:2]:<6}")
    fh.write("\n")
    for j in range(mat.shape[0]):
        lab = names[j + 1] if j + 1 < len(names) else ""
        fh.write(f"{lab[:2]:<6}")
        for k in range(j + 1):
            fh.write(f"{mat[j, k]:<+6.2f}")
        fh.write("\n")


def write_out(path, data, res, seconds, version=VERSION, date=None):
    """main.m:631-950: the .out report."""
    s = data.settings
    u_img = sum(int(s[k]) for k in ("Estimate_Xc", "Estimate_Yc", "Estimate_Zc", "Estimate_w", "Estimate_p",
                                     "Estimate_k"))
    nK = int(s["Num_Radial_Distortions"])
    u_cam = int(s["Estimate_c"]) + int(s["Estimate_xp"]) + int(s["Estimate_yp"]) + int(s["Estimate_radial"]) * nK + \
        2 * int(s["Estimate_decent"])
    ic = int(s["Inner_Constraints"])
    xhat, cxd = res.xhat, res.cx_diag
    std = np.sqrt(np.maximum(cxd, 0.0)) if cxd is not None else np.full(len(xhat), np.nan)
    date = date or datetime.date.today().strftime("%d-%b-%Y")
    n = data.n
    # prior observations of unknowns (no reference counterpart): counted as observations when they were used
    n_prior = len(res.prior_index) if getattr(res, "prior_index", None) is not None else 0
    prior_rows = [("Number of prior observations", num2str(n_prior))] if n_prior else []
    with open(path, "w") as fh:
        fh.write("Version: " + version)
        # main.m:637's title and author line, with this build named as the producer of the numbers below
        # (the model and the report layout are the reference's; the line count is unchanged)
        fh.write("Fish-eye model Bundle Adjustment\nResults produced by " + PRODUCER + "; model and report format: "
                 "Wynand Tredoux -- University of Calgary -- 2020\n\n")
        fh.write(LINE)
        fh.write(f"\n\nExecution date:\t{date}\nTime Taken:\t\t{num2str(seconds)} seconds\nIterations:\t\t"
                 f"{res.iterations}\nModel Used:\t\t{s['type']}")
        fh.write("\n\nSettings used:\n")
        print_cell(fh, _settings_rows(s), "\t\t")
        fh.write("\n" + LINE + "\n")
        fh.write("\nObservations/Unknowns Summary\n\n")
        rows = [("Number of Photos", num2str(data.numImg)),
                ("Total EOP unknowns", num2str(u_img * data.numImg)),
                ("Number of Cameras", num2str(data.numCam)),
                ("Total IOP unknowns", num2str((int(s["Estimate_c"]) + int(s["Estimate_xp"]) + int(s["Estimate_yp"]))
                                               * data.numCam)),
                ("Total distortion unknowns", num2str((int(s["Estimate_radial"]) * nK + int(s["Estimate_decent"]) * 2)
                                                      * data.numCam)),
                ("Number of tie/control points", num2str(data.numGCP)),
                ("Number of tie/control points to be estimated", num2str(data.numtie)),
                ("Number of control/tie point unknowns", num2str(data.numtie * 3)),
                ("\\line", ""),
                ("Total Unknowns", num2str(len(xhat))),
                ("\\n", ""),
                ("Number of image points", num2str(n // 2)),
                ("Total number of observations", num2str(n)),
                ("Number of Inner Constraints", num2str(7 * ic))] + prior_rows + [
                ("\\line", ""),
                ("Total Number of Observations", num2str(n + 7 * ic + n_prior)),
                ("\\n", ""),
                ("Total Degrees of Freedom", num2str(n + 7 * ic + n_prior - len(xhat))),
                ("\\n", ""),
                ("A-Posteriori", num2str(res.sigma02, 10)),
                ("RMSx", num2str(res.rms[0], 10)),
                ("RMSy", num2str(res.rms[1], 10)),
                ("RMS", num2str(res.rms[2], 10)),
                ("\\n", "")]
        print_cell(fh, rows, "")
        fh.write(LINE + "\n\n")

        # column width (main.m:687-706)
        tw = max((len(t) for t in sorted(set(data.pho_target))), default=0)
        iw = 0
        for t in sorted(set(data.pho_image)):
            if len(t) > tw:
                iw = len(t)
        w = max(tw, iw, 12) + 2

        # Estimated EOPs (main.m:709-770)
        fh.write("Estimated EOPs\nEOP Name\tValue\tStandard Deviation\n")
        img_count = {}
        for im in data.pho_image:
            img_count[im] = img_count.get(im, 0) + 1
        eop_names = [nm for nm, k in zip(("Xc", "Yc", "Zc", "Omega", "Phi", "Kappa"),
                                          ("Estimate_Xc", "Estimate_Yc", "Estimate_Zc", "Estimate_w", "Estimate_p",
                                           "Estimate_k")) if s[k]]
        q = 0
        eop_idx = []
        for i in range(data.numImg):
            r = data.EXT[i]
            fh.write("\n")
            print_cell(fh, [("Image", r[0]), ("Camera", r[1]), ("Number of image points", num2str(img_count.get(r[0], 0))),
                            ("\\line", "")], "")
            idx = []
            for nm in eop_names:
                f = 180.0 / math.pi if nm in ("Omega", "Phi", "Kappa") else 1.0
                fh.write(_line_eop(nm, xhat[q] * f, std[q] * f, w))
                idx.append(q)
                q += 1
            eop_idx.append(idx)

        # IOPs and distortions per camera (main.m:773-840)
        fh.write("\n" + LINE + "\n\nEstimated IOPs and Distortions for each Camera\nIOP Name\tValue\tStandard Deviation\n\n")
        par = [["Created with Fish-eye model Bundle Adjustment version:", version, None], ["Execution date", date, None],
               [None, None, None]]
        iop_names = ([nm for nm, k in (("xp", "Estimate_xp"), ("yp", "Estimate_yp"), ("c", "Estimate_c")) if s[k]]
                     + ([f"k{j + 1}" for j in range(nK)] if s["Estimate_radial"] else [])
                     + (["p1", "p2"] if s["Estimate_decent"] else []))
        cam_iop = {}
        for i in range(data.numCam):
            cid, ydir, xmin, ymin, xmax, ymax = data.INT[i][:6]
            par.append(["Camera", cid, None])
            print_cell(fh, [("Camera", cid), ("y axis dir", num2str(ydir)), ("x min", num2str(xmin)),
                            ("y min", num2str(ymin)), ("x max", num2str(xmax)), ("y max", num2str(ymax)),
                            ("\\line", "")], "")
            start = q
            for nm in iop_names:
                line = _line_eop if nm in ("xp", "yp", "c") else _line_dist
                fh.write(line(nm, xhat[q], std[q], w))
                par.append([nm, xhat[q], std[q]])
                q += 1
            cam_iop[cid] = (start, q)
            fh.write("\nIOP Correlation sub-matrix\n-------------------------------\n")
            sub = _iop_corr(res, data, cid, u_img, u_cam)
            _corr_rows(fh, [""] + iop_names, sub)
            fh.write("\n")

        # ground coordinates (main.m:843-866)
        if s["Estimate_tie"]:
            fh.write("\n" + LINE + "\n\nEstimated Ground Coordinates of targets\n"
                     "TargetID\tnumImages\tX\tY\tZ\tstdX\tstdY\tstdZ\n\n")
            tgt_count = {}
            for t in data.pho_target:
                tgt_count[t] = tgt_count.get(t, 0) + 1
            var = []
            for t in data.TIE:
                X = xhat[q:q + 3]
                sd = std[q:q + 3]
                var.append(sd ** 2)
                fh.write(f"{t:<{w}}{tgt_count.get(t, 0):<{w}d}" + "".join(f"{v:<{w}.{DECIMALS}f}" for v in X)
                         + "".join(f"{v:<{w}.{DECIMALS}f}" for v in sd) + "\n")
                q += 3
            avg = np.sqrt(np.mean(np.array(var), axis=0)) if var else np.full(3, np.nan)
            fh.write("\n\t\tMeanStd X\tMeanStd Y\tMeanStd Z\n")
            fh.write("\t\t" + "".join(f"{v:<{w}.{DECIMALS}f}" for v in avg) + "\n")

        # corrected image measurements (main.m:586-590, :869-873)
        fh.write("\n" + LINE + "\n\nCorrected Image Measurements\nPointID\tImageID\tCorrected x\tCorrected y\n\n")
        for i in range(data.n_pts):
            xc = data.xy[i, 0] + res.rsd[i, 1]
            yc = data.xy[i, 1] + res.rsd[i, 2]
            fh.write(f"{data.pho_target[i]:<{w}}{data.pho_image[i]:<{w}}{xc:<{w}.{DECIMALS}f}{yc:<{w}.{DECIMALS}f}\n")

        # mean absolute EOP/IOP correlations per camera (main.m:879-917)
        fh.write("\n" + LINE + "\n\nAbsolute (positive) mean correlation coefficients between EOPs and IOPs\n\n")
        order = sorted(range(data.numImg), key=lambda e: data.EXT[e][1])  # sortrows(EOP_IOP_Corr, 2): stable
        g = 0
        while g < len(order):
            cid = data.EXT[order[g]][1]
            members = []
            while g < len(order) and data.EXT[order[g]][1] == cid:
                members.append(order[g])
                g += 1
            has_iop = cid in cam_iop and cam_iop[cid][1] > cam_iop[cid][0]
            names = [""] + eop_names + ([""] + iop_names if cid in cam_iop else [])
            fh.write(f"Camera {cid}\n")
            m = u_img + (u_cam if has_iop else 0)
            acc = np.zeros((m, m))
            for e in members:
                acc += np.abs(np.tril(_img_corr(res, e, m)))
            _corr_rows(fh, names, acc / len(members))
            fh.write("\n")

        # check points (main.m:604-628, :920-931)
        if s.get("Check_Points") and data.CZE:
            names_x = {nm: j for j, nm in enumerate(res.xhatnames)}
            diffs = []
            for r in data.CZE:
                j = names_x.get("X_" + r[0])
                if j is None:
                    print(f"Warning: Check point not found in xhat -> {r[0]}")
                    continue
                diffs.append((r[0], *(xhat[j:j + 3] - np.array([float(v) for v in r[1:4]]))))
            fh.write("\n" + LINE + "\n\nCheck point differences\n")
            fh.write(f"{'TargetID':<{w}}{'diff X':<{w}}{'diff Y':<{w}}{'diff Z':<{w}}\n\n")
            for d in diffs:
                fh.write(f"{d[0]:<{w}}" + "".join(f"{v:<{w}.{DECIMALS}f}" for v in d[1:]) + "\n")
            if diffs:
                a = np.array([d[1:] for d in diffs], dtype=float)
                fh.write(f"\n{'Mean':<{w}}" + "".join(f"{v:<{w}.{DECIMALS}f}" for v in a.mean(0)) + "\n")
                fh.write(f"{'RMS':<{w}}" + "".join(f"{v:<{w}.{DECIMALS}f}" for v in np.sqrt((a ** 2).mean(0))) + "\n")
    return par


def _img_corr(res, e, m):
    if res.corr is None:
        return np.full((m, m), np.nan)
    return res.corr[e][:m, :m]


def _iop_corr(res, data, cid, u_img, u_cam):
    """The camera's IOP block of Correlation: the trailing u_cam x u_cam part of any of its images'
    EOP/IOP sub-blocks (they are the same entries of Correlation)."""
    if res.corr is None or u_cam == 0:
        return np.zeros((u_cam, u_cam))
    for e in range(data.numImg):
        if data.EXT[e][1] == cid:
            return res.corr[e][u_img:u_img + u_cam, u_img:u_img + u_cam]
    return np.zeros((u_cam, u_cam))


def _cell(v):
    if v is None:
        return ""
    if isinstance(v, str):
        return v
    return f"{float(v):.15g}"


def write_par(path, par):
    """writecell(PAR, name.par, tab-delimited) (main.m:956)."""
    with open(path, "w") as fh:
        for r in par:
            fh.write("\t".join(_cell(v) for v in r) + "\n")


def write_rsd(path, data, rsd):
    """writecell(RSD, name.rsd, tab-delimited) (main.m:955, BuildRSD.m:29-40): targetID, imageID, x, y,
    r, vx, vy, vr, vt per image point."""
    with open(path, "w") as fh:
        for i in range(data.n_pts):
            r = rsd[i]
            fh.write("\t".join([data.pho_target[i], data.pho_image[i], _cell(data.xy[i, 0]), _cell(data.xy[i, 1])]
                               + [_cell(v) for v in r]) + "\n")


def write_rel(path, data, res):
    """The reliability table <Output_Filename stem>.rel (no reference counterpart), tab-delimited in
    write_rsd's style: targetID, imageID, r_x, r_y, w_x, w_y, mdb_x, mdb_y, flag per image point.  r and w
    are fba_reliability's (res.redundancy, res.wstat); mdb = MDB_DELTA0 sigma / sqrt(r) is the smallest
    gross error the w-test detects (inf where r < R_MIN); flag is * where max(|w_x|, |w_y|) > W_CRITICAL."""
    if res.redundancy is None or res.wstat is None:
        raise ValueError("write_rel: the adjustment carries no reliability (adjust(..., reliability=True))")
    r = np.asarray(res.redundancy, dtype=np.float64).reshape(-1, 2)
    w = np.asarray(res.wstat, dtype=np.float64).reshape(-1, 2)
    sigma = (float(data.settings["Meas_std"]), float(data.settings["Meas_std_y"]))
    with open(path, "w") as fh:
        for i in range(data.n_pts):
            mdb = [MDB_DELTA0 * sigma[m] / math.sqrt(r[i, m]) if r[i, m] >= R_MIN else math.inf for m in range(2)]
            flag = "*" if max(abs(w[i, 0]), abs(w[i, 1])) > W_CRITICAL else ""
            fh.write("\t".join([data.pho_target[i], data.pho_image[i]]
                               + [_cell(v) for v in (r[i, 0], r[i, 1], w[i, 0], w[i, 1], mdb[0], mdb[1])] + [flag]) + "\n")


def write_wgt(path, data, res):
    """The weight table <Output_Filename stem>.wgt (no reference counterpart), written when per-observation
    weights or a robust loss are in force; tab-delimited in write_rsd's style: PHO row (1-based, the line of
    the .pho file), targetID, imageID, effective weight x, y (fba_get_weights: user weight x loss factor at the
    last linearisation), flag per image point; flag is * where either weight is below WGT_FLAG."""
    if res.weights is None:
        raise ValueError("write_wgt: the adjustment carries no weights (adjust(..., weights= / robust=))")
    w = np.asarray(res.weights, dtype=np.float64).reshape(-1, 2)
    if len(w) != data.n_pts:
        raise ValueError("write_wgt: weights must have 2*n_pts entries")
    with open(path, "w") as fh:
        for i in range(data.n_pts):
            flag = "*" if min(w[i, 0], w[i, 1]) < WGT_FLAG else ""
            fh.write("\t".join([str(i + 1), data.pho_target[i], data.pho_image[i], _cell(w[i, 0]), _cell(w[i, 1]), flag])
                     + "\n")


def write_prr(path, data, res):
    """The prior-observation table <Output_Filename stem>.prr (no reference counterpart), written when priors
    were used; tab-delimited in write_rsd's style: unknown name, prior value, std, adjusted value, v = adjusted -
    prior, redundancy number r, test statistic w, flag per prior, in the order they were given.  Angles (w_, p_,
    k_ unknowns) in degrees like the .pri table; r and w empty when the adjustment carries no covariance; flag is
    * where |w| > W_CRITICAL."""
    if getattr(res, "prior_index", None) is None:
        raise ValueError("write_prr: the adjustment carries no priors (adjust(..., priors=))")
    with open(path, "w") as fh:
        for j, i in enumerate(res.prior_index):
            name = res.xhatnames[i]
            f = 180.0 / math.pi if name.split("_", 1)[0] in ("w", "p", "k") else 1.0
            r = None if res.prior_r is None else res.prior_r[j]
            w = None if res.prior_w is None else res.prior_w[j]
            flag = "*" if w is not None and abs(w) > W_CRITICAL else ""
            fh.write("\t".join([name] + [_cell(v) for v in (res.prior_value[j] * f, res.prior_sigma[j] * f, res.xhat[i] * f,
                                                           res.prior_v[j] * f, r, w)] + [flag]) + "\n")


def write_lm(path, history):
    """The damped loop's table <Output_Filename stem>.lm (no reference counterpart), written with method="lm";
    tab-delimited in write_rsd's style, one row per trial and polish pass of fba_adjust_lm: number (1-based),
    lambda (0 for an undamped polish pass), the cost after it, deltasum, accepted (1 / 0)."""
    h = np.asarray(history, dtype=np.float64).reshape(-1, 4)
    with open(path, "w") as fh:
        for i, (lam, cost, dsum, acc) in enumerate(h):
            fh.write("\t".join([str(i + 1), _cell(lam), _cell(cost), _cell(dsum), str(int(acc))]) + "\n")


def horizontal_ellipse(sxx, sxy, syy):
    """The 1-sigma error ellipse of a 2 x 2 covariance [[sxx, sxy], [sxy, syy]] in closed form: (semi-major,
    semi-minor, azimuth of the major axis in degrees in [0, 180), counted from +Y towards +X; 0 for a circle)."""
    m, d = 0.5 * (sxx + syy), 0.5 * (sxx - syy)
    r = math.hypot(d, sxy)
    az = 0.0 if r == 0.0 else math.degrees(0.5 * math.atan2(2.0 * sxy, syy - sxx)) % 180.0
    return math.sqrt(max(m + r, 0.0)), math.sqrt(max(m - r, 0.0)), (0.0 if az >= 180.0 else az)


def write_ell(path, data, res):
    """The point-precision table <Output_Filename stem>.ell (no reference counterpart: main.m:460-482 keeps the
    diagonal of Cx), tab-delimited in write_rsd's style, one row per tie point in TIE order: targetID; sigma X, Y,
    Z (the square roots of the block's diagonal); the 1-sigma semi-axes a >= b >= c of the error ellipsoid; the
    nine direction cosines of its axes (axis a's X Y Z, then b's, then c's); the horizontal error ellipse of the
    block's XY part (horizontal_ellipse): semi-major, semi-minor, azimuth of the major axis in degrees in
    [0, 180).  Every length is 1 sigma: multiply the three semi-axes by ELL_K95 = 2.7955 = sqrt(chi2_3(0.95)) for
    the region that holds the point with 95 % probability."""
    if getattr(res, "cx_tie", None) is None or getattr(res, "ell_axes", None) is None or getattr(res, "ell_dirs", None) is None:
        raise ValueError("write_ell: the adjustment carries no point precision (adjust(..., point_precision=True))")
    blk = np.asarray(res.cx_tie, dtype=np.float64).reshape(-1, 3, 3)
    ax = np.asarray(res.ell_axes, dtype=np.float64).reshape(-1, 3)
    dr = np.asarray(res.ell_dirs, dtype=np.float64).reshape(-1, 9)
    if not (len(blk) == len(ax) == len(dr) == len(data.TIE)):
        raise ValueError("write_ell: one block and one ellipsoid per tie point expected")
    with open(path, "w") as fh:
        for t, name in enumerate(data.TIE):
            b = blk[t]
            sig = [math.sqrt(max(b[k, k], 0.0)) for k in range(3)]
            fh.write("\t".join([name] + [_cell(v) for v in (*sig, *ax[t], *dr[t], *horizontal_ellipse(b[0, 0], b[0, 1], b[1, 1]))])
                     + "\n")


def read_ell(path):
    """write_ell's table back: (targetIDs, sigma (n, 3), axes (n, 3), directions (n, 3, 3), horizontal (n, 3):
    semi-major, semi-minor, azimuth)"""
    names, vals = [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if len(c) != 19:
                raise ValueError(f"read_ell: {path}: expected 19 tab-separated columns, got {len(c)}")
            names.append(c[0])
            vals.append([float(x) for x in c[1:]])
    v = np.array(vals, dtype=np.float64).reshape(-1, 18)
    return names, v[:, 0:3], v[:, 3:6], v[:, 6:15].reshape(-1, 3, 3), v[:, 15:18]


FWD_STATUS = ("OK", "FEW", "WEAK", "REFINE")  # FBA_ISECT_*


def write_fwd(path, data, res):
    """The forward-intersection table <Output_Filename stem>.fwd (no reference counterpart: the reference takes the
    object points' starting values from the .cnt file; .int is the interior-orientation file, hence .fwd),
    tab-delimited in write_ell's style, one row per tie point in TIE order: targetID; rays used; the intersected
    X Y Z; its shift from the .cnt value; lambda_min / lambda_max of the intersection's normal matrix ((1 - |cos a|)
    / 2 for two rays meeting at the angle a); the RMS reprojection residual in pixels of the linear and of the
    refined solution; and, where the status is not OK, * and the status word -- FEW (fewer than 2 usable rays) and
    WEAK (ratio below the bound): the point kept its .cnt value; REFINE: the linear solution was kept."""
    if getattr(res, "isect_xyz", None) is None or getattr(res, "isect_quality", None) is None or \
            getattr(res, "isect_status", None) is None:
        raise ValueError("write_fwd: the adjustment carries no intersection (adjust(..., intersect=True))")
    xyz = np.asarray(res.isect_xyz, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(res.isect_quality, dtype=np.float64).reshape(-1, 4)
    st = np.asarray(res.isect_status).reshape(-1)
    if not (len(xyz) == len(q) == len(st) == len(data.TIE)):
        raise ValueError("write_fwd: one intersection per tie point expected")
    with open(path, "w") as fh:
        for t, name in enumerate(data.TIE):
            x0 = np.asarray(data.CNT[name], dtype=np.float64)
            flag = [] if st[t] == 0 else ["*", FWD_STATUS[int(st[t])]]
            fh.write("\t".join([name, str(int(q[t, 0]))] + [_cell(v) for v in (*xyz[t], *(xyz[t] - x0), *q[t, 1:])] + flag)
                     + "\n")


def read_fwd(path):
    """write_fwd's table back: (targetIDs, rays (n), xyz (n, 3), shift (n, 3), quality (n, 3): ratio, RMS linear,
    RMS final; status words (n), "OK" where the row carries no flag)"""
    names, rays, vals, words = [], [], [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if len(c) not in (11, 13) or (len(c) == 13 and c[11] != "*"):
                raise ValueError(f"read_fwd: {path}: expected 11 tab-separated columns, or 13 with the flag, got {len(c)}")
            names.append(c[0])
            rays.append(int(c[1]))
            vals.append([float(x) for x in c[2:11]])
            words.append(c[12] if len(c) == 13 else "OK")
    v = np.array(vals, dtype=np.float64).reshape(-1, 9)
    return names, np.array(rays, dtype=np.int64), v[:, 0:3], v[:, 3:6], v[:, 6:9], words


RSC_STATUS = ("OK", "FEW", "WEAK", "REFINE")  # FBA_RESECT_*


def write_rsc(path, data, res):
    """The space-resection table <Output_Filename stem>.rsc (no reference counterpart: the reference takes the
    exterior orientation's starting values from the .ext file), tab-delimited in write_fwd's style, one row per image
    in EXT order: imageID; points used; the resected Xc Yc Zc omega phi kappa (radians); its shift from the .ext
    values; lambda_1 / lambda_11 of the linear solution's Gram matrix (about (relief / extent)^2; 0 for coplanar
    points); the RMS reprojection residual in pixels of the linear and of the refined solution; and, where the status
    is not OK, * and the status word -- FEW (fewer than 6 usable points) and WEAK (ratio below the bound): the image
    kept its .ext values; REFINE: the linear solution was kept."""
    if getattr(res, "resect_eop", None) is None or getattr(res, "resect_quality", None) is None or \
            getattr(res, "resect_status", None) is None:
        raise ValueError("write_rsc: the adjustment carries no resection (adjust(..., resect=True))")
    eop = np.asarray(res.resect_eop, dtype=np.float64).reshape(-1, 6)
    q = np.asarray(res.resect_quality, dtype=np.float64).reshape(-1, 5)
    st = np.asarray(res.resect_status).reshape(-1)
    if not (len(eop) == len(q) == len(st)) or len(eop) > len(data.EXT):
        raise ValueError("write_rsc: one resection per image expected")
    with open(path, "w") as fh:
        for i in range(len(eop)):
            row = data.EXT[i]
            x0 = np.asarray(row[2:8], dtype=np.float64)
            flag = [] if st[i] == 0 else ["*", RSC_STATUS[int(st[i])]]
            fh.write("\t".join([str(row[0]), str(int(q[i, 0]))] + [_cell(v) for v in (*eop[i], *(eop[i] - x0), *q[i, 1:4])]
                               + flag) + "\n")


def read_rsc(path):
    """write_rsc's table back: (imageIDs, points used (n), eop (n, 6), shift (n, 6), quality (n, 3): ratio, RMS
    linear, RMS final; status words (n), "OK" where the row carries no flag)"""
    names, used, vals, words = [], [], [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if len(c) not in (17, 19) or (len(c) == 19 and c[17] != "*"):
                raise ValueError(f"read_rsc: {path}: expected 17 tab-separated columns, or 19 with the flag, got {len(c)}")
            names.append(c[0])
            used.append(int(c[1]))
            vals.append([float(x) for x in c[2:17]])
            words.append(c[18] if len(c) == 19 else "OK")
    v = np.array(vals, dtype=np.float64).reshape(-1, 15)
    return names, np.array(used, dtype=np.int64), v[:, 0:6], v[:, 6:12], v[:, 12:15], words


VCE_STATUS = ("OK", "EMPTY", "WEAK", "CLIPPED")  # FBA_VCE_*


def write_vce(path, res):
    """The variance-component table <Output_Filename stem>.vce (no reference counterpart: main.m:397-402 fixes the
    weights), tab-delimited in write_rsd's style, two parts.  Per group, then the rows of no group and the priors
    (reported only): `G`, name, rows, sum of the redundancy numbers, the component (cumulative variance factor relative
    to the starting weights), the a-posteriori sigma in pixels (empty for the two report entries), the status word.
    Per round and group, the history: `R`, round (1-based), name, R, T, n, sigma2.  The G rows' rows and sum r are
    the last round's."""
    if getattr(res, "vce_component", None) is None or getattr(res, "vce_table", None) is None:
        raise ValueError("write_vce: the adjustment carries no variance components (adjust(..., vce=...))")
    comp = np.asarray(res.vce_component, dtype=np.float64).reshape(-1)
    sig = np.asarray(res.vce_sigma, dtype=np.float64).reshape(-1)
    st = np.asarray(res.vce_status).reshape(-1)
    tab = np.asarray(res.vce_table, dtype=np.float64).reshape(-1, len(comp), 4)
    names = list(res.vce_names)
    if not (len(comp) == len(sig) == len(st) == len(names)) or len(tab) < 1:
        raise ValueError("write_vce: one name, component, sigma and status per group and at least one round expected")
    with open(path, "w") as fh:
        for g, name in enumerate(names):
            fh.write("\t".join(["G", name, str(int(tab[-1, g, 2])), _cell(tab[-1, g, 0]), _cell(comp[g]),
                                "" if math.isnan(sig[g]) else _cell(sig[g]), VCE_STATUS[int(st[g])]]) + "\n")
        for k in range(len(tab)):
            for g, name in enumerate(names):
                fh.write("\t".join(["R", str(k + 1), name] + [_cell(x) for x in tab[k, g]]) + "\n")


def read_vce(path):
    """write_vce's table back: (names, rows (g), sum r (g), component (g), sigma (g) -- NaN for an empty cell --,
    status words (g), table (rounds, g, 4))"""
    names, head, words, hist = [], [], [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if c[0] == "G" and len(c) == 7:
                names.append(c[1])
                head.append([float(c[2]), float(c[3]), float(c[4]), float(c[5]) if c[5] else math.nan])
                words.append(c[6])
            elif c[0] == "R" and len(c) == 7:
                hist.append([float(x) for x in c[3:7]])
            else:
                raise ValueError(f"read_vce: {path}: expected 7 tab-separated columns starting with G or R")
    h = np.array(head, dtype=np.float64).reshape(-1, 4)
    if not names or len(hist) % len(names):
        raise ValueError(f"read_vce: {path}: the history does not hold whole rounds")
    return (names, h[:, 0].astype(np.int64), h[:, 1], h[:, 2], h[:, 3], words,
            np.array(hist, dtype=np.float64).reshape(-1, len(names), 4))


def read_prr(path):
    """write_prr's table back: (names, values (n, 6): prior, std, adjusted, v, r, w -- NaN for an empty cell --,
    flagged (n) bool)"""
    names, vals, flag = [], [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if len(c) != 8:
                raise ValueError(f"read_prr: {path}: expected 8 tab-separated columns, got {len(c)}")
            names.append(c[0])
            vals.append([float(x) if x else math.nan for x in c[1:7]])
            flag.append(c[7] == "*")
    return names, np.array(vals, dtype=np.float64).reshape(-1, 6), np.array(flag, dtype=bool)


def read_wgt(path):
    """write_wgt's table back: (rows, targetIDs, imageIDs, weights (n_pts, 2), flagged (n_pts) bool)."""
    rows, tgt, img, w, flag = [], [], [], [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if len(c) != 6:
                raise ValueError(f"read_wgt: {path}: expected 6 tab-separated columns, got {len(c)}")
            rows.append(int(c[0]))
            tgt.append(c[1])
            img.append(c[2])
            w.append((float(c[3]), float(c[4])))
            flag.append(c[5] == "*")
    return rows, tgt, img, np.array(w, dtype=np.float64).reshape(-1, 2), np.array(flag, dtype=bool)


SNOOP_STATE = ("ACTIVE", "EXCLUDED", "READMITTED")


def write_snp(path, data, res):
    """The data-snooping table <Output_Filename stem>.snp (no reference counterpart: main.m never tests a
    measurement), tab-delimited in write_rsd's style, two parts.  Per image point the snooping excluded or re-admitted:
    `E`, PHO row (1-based), image name, point name, the state word, W~ (an excluded point's statistic of the predicted
    residual; W for a re-admitted one) of the last round, vx, vy in pixels.  Per round: `R`, round (1-based), points
    picked, points the back-check passed, points excluded after the round, the largest W of an active point."""
    if getattr(res, "snoop_excluded", None) is None or getattr(res, "snoop_table", None) is None:
        raise ValueError("write_snp: the adjustment carries no data snooping (adjust(..., snoop=...))")
    ex = np.asarray(res.snoop_excluded).reshape(-1)
    stat = np.asarray(res.snoop_stat, dtype=np.float64).reshape(-1)
    v = np.asarray(res.v, dtype=np.float64).reshape(-1, 2)
    tab = np.asarray(res.snoop_table, dtype=np.float64).reshape(-1, 4)
    if not (len(ex) == len(stat) == len(v) == len(data.pho_image)):
        raise ValueError("write_snp: one state, statistic and residual pair per PHO row expected")
    with open(path, "w") as fh:
        for i in np.nonzero(ex)[0]:
            fh.write("\t".join(["E", str(i + 1), str(data.pho_image[i]), str(data.pho_target[i]), SNOOP_STATE[int(ex[i])],
                                _cell(stat[i]), _cell(v[i, 0]), _cell(v[i, 1])]) + "\n")
        for k, row in enumerate(tab):
            fh.write("\t".join(["R", str(k + 1), str(int(row[0])), str(int(row[1])), str(int(row[2])), _cell(row[3])]) + "\n")


def read_snp(path):
    """write_snp's table back: (rows (m) 0-based PHO rows, images (m), points (m), state words (m), stat (m), v (m, 2),
    table (rounds, 4))"""
    rows, imgs, pts, words, num, hist = [], [], [], [], [], []
    with open(path) as fh:
        for ln in fh:
            c = ln.rstrip("\n").split("\t")
            if c[0] == "E" and len(c) == 8:
                rows.append(int(c[1]) - 1)
                imgs.append(c[2])
                pts.append(c[3])
                words.append(c[4])
                num.append([float(x) for x in c[5:8]])
            elif c[0] == "R" and len(c) == 6:
                hist.append([float(x) for x in c[2:6]])
            else:
                raise ValueError(f"read_snp: {path}: expected 8 tab-separated columns starting with E or 6 starting with R")
    a = np.array(num, dtype=np.float64).reshape(-1, 3)
    return (np.array(rows, dtype=np.int64), imgs, pts, words, a[:, 0], a[:, 1:], np.array(hist, dtype=np.float64).reshape(-1, 4))
