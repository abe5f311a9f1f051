"""numpy restatements for the forward-intersection tests (tests/test_intersect_host.py, tests/test_gpu_intersect.py):
the inverse projection model, the linear line intersection and the point-only Gauss-Newton refinement with the
analytic tie Jacobian, each in any float dtype (float64, longdouble), and the packed problems of synth scenes.

Written from include/fba.h's description of fba_unproject_host / fba_image_rays / fba_intersect and BuildAwG.m's
model, not from the device code: the sums here are numpy's, in PHO order."""
import numpy as np

TYPES = ("fisheye", "pinhole", "equisolid", "orthographic", "stereographic")
F64_MAX = np.finfo(np.float64).max
SENSOR = (0.0, 0.0, 2048.0, 2048.0)


def rot(w, p, k):
    """BuildAwG.m:163-165: (U, V, W) = M (X - Xc)"""
    cw, sw, cp, sp, ck, sk = np.cos(w), np.sin(w), np.cos(p), np.sin(p), np.cos(k), np.sin(k)
    return np.stack([np.stack([ck * cp, cw * sk + ck * sp * sw, sk * sw - ck * cw * sp], -1),
                     np.stack([-cp * sk, ck * cw - sk * sp * sw, ck * sw + cw * sk * sp], -1),
                     np.stack([sp, -cp * sw, cp * cw], -1)], -2)


def g_of(typ, t):
    return {"fisheye": lambda: t, "pinhole": lambda: np.tan(t), "equisolid": lambda: 2 * np.sin(t / 2),
            "orthographic": lambda: np.sin(t), "stereographic": lambda: 2 * np.tan(t / 2)}[typ]()


def distortion(xb, yb, K, P1, P2):
    r2 = xb * xb + yb * yb
    dr = sum(K[j] * r2 ** (j + 1) for j in range(len(K)))
    return (dr * xb + P1 * (yb * yb + 3 * xb * xb) + 2 * P2 * xb * yb,
            dr * yb + P2 * (xb * xb + 3 * yb * yb) + 2 * P1 * xb * yb)


def forward(typ, UVW, camtab, dtype=np.longdouble, iters=80):
    """pixels of camera-frame points, either sign of W, the distortion at the OBSERVED coordinates (fixed point)"""
    ct = np.asarray(camtab, dtype=dtype)
    xp, yp, c, ydir, P1, P2, K = ct[0], ct[1], ct[2], ct[3], ct[4], ct[5], ct[6:]
    U, V, W = (np.asarray(UVW, dtype=dtype)[:, i] for i in range(3))
    R = np.sqrt(U * U + V * V)
    s = (1 / W) if typ == "pinhole" else g_of(typ, np.arctan(R / W)) / R
    px, py = -c * s * U, -c * ydir * s * V
    xb, yb = px.copy(), py.copy()
    for _ in range(iters):
        dx, dy = distortion(xb, yb, K, P1, P2)
        xb, yb = px + dx, py + dy
    return np.stack([xb + xp, yb + yp], -1)


def unproject(typ, xy, camtab, dtype=np.float64):
    """(xu yu | d) (n, 5) and status (n): include/fba.h's closed-form ray"""
    ct = np.asarray(camtab, dtype=dtype)
    xp, yp, c, ydir, P1, P2, K = ct[0], ct[1], ct[2], ct[3], ct[4], ct[5], ct[6:]
    xy = np.asarray(xy, dtype=dtype).reshape(-1, 2)
    xb, yb = xy[:, 0] - xp, xy[:, 1] - yp
    dx, dy = distortion(xb, yb, K, P1, P2)
    xu, yu = xb - dx, yb - dy
    rho = np.sqrt(xu * xu + yu * yu)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = rho / c
        bad = ~(np.abs(q) <= F64_MAX)
        if typ == "orthographic":
            bad |= ~(np.abs(q) <= 1)
        if typ == "equisolid":
            bad |= ~(np.abs(q) <= 2)
        qs = np.where(bad, 0, q)
        t = {"fisheye": lambda: qs, "pinhole": lambda: np.arctan(qs), "equisolid": lambda: 2 * np.arcsin(qs / 2),
             "orthographic": lambda: np.arcsin(qs), "stereographic": lambda: 2 * np.arctan(qs / 2)}[typ]()
        safe = np.where(rho > 0, rho, 1)
        d = np.stack([-np.sin(t) * xu / safe, -ydir * np.sin(t) * yu / safe, np.cos(t)], -1)
    d[rho == 0] = (0, 0, 1)
    d[bad] = 0
    return np.concatenate([np.stack([xu, yu], -1), d], -1), bad.astype(np.int32)


def sym3_solve(S, r):
    """x = S^-1 r by the adjugate, any dtype (longdouble has no LAPACK)"""
    c00 = S[1, 1] * S[2, 2] - S[1, 2] * S[1, 2]
    c01 = S[0, 2] * S[1, 2] - S[0, 1] * S[2, 2]
    c02 = S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]
    det = S[0, 0] * c00 + S[0, 1] * c01 + S[0, 2] * c02
    inv = np.array([[c00, c01, c02],
                    [c01, S[0, 0] * S[2, 2] - S[0, 2] * S[0, 2], S[0, 1] * S[0, 2] - S[0, 0] * S[1, 2]],
                    [c02, S[0, 1] * S[0, 2] - S[0, 0] * S[1, 2], S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]]], dtype=S.dtype) / det
    return inv @ r


def project_tie(typ, M, e, c, ydir):
    """the forward model's part that depends on the point, (px, py) = -c s (U, ydir V), and its 2 x 3 derivative to
    X Y Z (BuildAwG.m:216-503's tie columns by the chain rule); M (n, 3, 3), e = X - C (n, 3), c, ydir (n)"""
    UVW = np.einsum("nij,nj->ni", M, e)
    U, V, W = UVW[:, 0], UVW[:, 1], UVW[:, 2]
    R = np.sqrt(U * U + V * V)
    if typ == "pinhole":
        s, sR, sW = 1 / W, 0 * W, -1 / (W * W)
    else:
        t = np.arctan(R / W)
        q2 = R * R + W * W
        tR, tW = W / q2, -R / q2
        g = g_of(typ, t)
        gt = {"fisheye": lambda: 1 + 0 * t, "equisolid": lambda: np.cos(t / 2), "orthographic": lambda: np.cos(t),
              "stereographic": lambda: 1 / np.cos(t / 2) ** 2}[typ]()
        s = g / R
        sR, sW = (gt * tR - s) / R, gt * tW / R
    dU, dV, dW = M[:, 0, :], M[:, 1, :], M[:, 2, :]          # (n, 3): d / dX_q
    dR = (U[:, None] * dU + V[:, None] * dV) / R[:, None]
    ds = sR[:, None] * dR + sW[:, None] * dW
    jx = -c[:, None] * (dU * s[:, None] + U[:, None] * ds)
    jy = -(c * ydir)[:, None] * (dV * s[:, None] + V[:, None] * ds)
    return -c * s * U, -c * ydir * s * V, jx, jy


class Problem:
    """what the restatement needs of a packed problem at given EOPs / IOPs: per PHO row the ray and the tables"""

    def __init__(self, packed, typ, nk, eop=None, iop=None, dtype=np.float64):
        self.typ, self.dtype = typ, dtype
        n_img, n_cam = packed.n_img, packed.n_cam
        eop = np.asarray(packed.eop0 if eop is None else eop, dtype=dtype).reshape(n_img, 6)
        iop = np.asarray(packed.iop0 if iop is None else iop, dtype=dtype).reshape(n_cam, 5 + nk)
        ydir = np.asarray(packed.cam_info, dtype=dtype).reshape(n_cam, 5)[:, 0]
        self.xy = np.asarray(packed.xy, dtype=dtype).reshape(-1, 2)
        self.img, self.cam, self.tie = packed.img, packed.cam, packed.tie
        self.M = rot(eop[:, 3], eop[:, 4], eop[:, 5])[self.img]
        self.C = eop[self.img, :3]
        self.c, self.ydir = iop[self.cam, 2], ydir[self.cam]
        self.uv = np.zeros((len(self.img), 5), dtype=dtype)
        self.rst = np.zeros(len(self.img), dtype=np.int32)
        for k in range(n_cam):
            rows = np.nonzero(self.cam == k)[0]
            ct = np.concatenate([iop[k, :3], [ydir[k]], iop[k, 3 + nk:5 + nk], iop[k, 3:3 + nk]])
            self.uv[rows], self.rst[rows] = unproject(typ, self.xy[rows], ct, dtype)
        self.d = np.einsum("nji,nj->ni", self.M, self.uv[:, 2:])     # M' d
        self.n_tie = packed.n_tie

    def rows_of(self, t):
        return np.nonzero(self.tie == t)[0]


def rms_at(pb, rows, X):
    px, py, _, _ = project_tie(pb.typ, pb.M[rows], X[None, :] - pb.C[rows], pb.c[rows], pb.ydir[rows])
    w = np.stack([px - pb.uv[rows, 0], py - pb.uv[rows, 1]], -1)
    return np.sqrt((w * w).sum() / len(rows))


def intersect_point(pb, t, refine_iters=10, refine_tol=1e-10, sx=0.3, sy=0.3):
    """(rays, ratio (float64 eigvalsh), X linear, X final, rms linear, rms final, iterations) of tie point t, or
    None with fewer than 2 usable rays"""
    rows = pb.rows_of(t)
    rows = rows[pb.rst[rows] == 0]
    if len(rows) < 2:
        return None
    dt = pb.dtype
    C, d = pb.C[rows], pb.d[rows]
    Pm = np.eye(3, dtype=dt)[None] - d[:, :, None] * d[:, None, :]
    A = Pm.sum(0)
    b = np.einsum("nij,nj->i", Pm, C - C[0])
    lam = np.linalg.eigvalsh(A.astype(np.float64))
    XL = C[0] + sym3_solve(A, b)
    X = XL.copy()
    pw = np.array([1 / dt(sx) ** 2, 1 / dt(sy) ** 2], dtype=dt)
    it = 0
    for it in range(1, refine_iters + 1):
        e = X[None, :] - C
        px, py, jx, jy = project_tie(pb.typ, pb.M[rows], e, pb.c[rows], pb.ydir[rows])
        w0, w1 = px - pb.uv[rows, 0], py - pb.uv[rows, 1]
        V = pw[0] * jx.T @ jx + pw[1] * jy.T @ jy
        g = pw[0] * jx.T @ w0 + pw[1] * jy.T @ w1
        step = sym3_solve(V, g)
        tol = dt(refine_tol) * np.sqrt((e * e).sum(1)).mean()
        X = X - step
        if np.abs(step).max() <= tol:
            break
    return dict(rays=len(rows), ratio=lam[0] / lam[2], lin=XL, fin=X, rms_lin=rms_at(pb, rows, XL),
                rms_fin=rms_at(pb, rows, X), iters=it if refine_iters else 0, dist=np.sqrt(((XL - C) ** 2).sum(1)).mean())


def intersect_all(pb, **kw):
    return [intersect_point(pb, t, **kw) for t in range(pb.n_tie)]


# ---- synth scenes as packed problems (no files) ---------------------------------------------------------------------
def settings_dict(typ, nk, cap=20):
    s = {k: 1 for k in ("Estimate_Xc", "Estimate_Yc", "Estimate_Zc", "Estimate_w", "Estimate_p", "Estimate_k",
                        "Estimate_xp", "Estimate_yp", "Estimate_c", "Estimate_radial", "Estimate_decent")}
    s.update({"Num_Radial_Distortions": nk, "type": typ, "Inner_Constraints": 0, "Iteration_Cap": cap,
              "threshold": 1e-6, "Meas_std": 0.3, "Meas_std_y": 0.3})
    return s


def true_iop(synth, n_cam, nk):
    K = (list(synth.K0) + [0.0] * 8)[:nk]
    return np.array([[*synth.camera_params(k), *K, *synth.P0] for k in range(n_cam)])


def start_iop(synth, n_cam, nk):
    """write_folder's .int values"""
    return np.array([[synth.camera_params(k)[0] + 0.5, synth.camera_params(k)[1] + 0.5, synth.camera_params(k)[2] + 1.0,
                      *([0.0] * nk), 0.0, 0.0] for k in range(n_cam)])


def pack_scene(capi, synth, sc, nk, truth=False, keep=None, extra=None):
    """the scene as a capi.PackedProblem in scene order; truth: the true EOPs / IOPs (else C0 / ang0 and the start
    IOPs); keep: a row mask; extra: (pid, img, xy) rows appended.  tie0 = X0 of the non-control points."""
    pid, img, xy = sc["pid"], sc["img"], sc["xy"]
    if keep is not None:
        pid, img, xy = pid[keep], img[keep], xy[keep]
    if extra is not None:
        pid = np.concatenate([pid, np.atleast_1d(extra[0])])
        img = np.concatenate([img, np.atleast_1d(extra[1])])
        xy = np.concatenate([xy, np.reshape(extra[2], (-1, 2))])
    n_img, n_cam = len(sc["C0"]), int(sc["cam"].max()) + 1
    control = sc["control"]
    tie_of = np.where(control, -1, np.cumsum(~control) - 1)
    eop = np.concatenate([sc["C_true"], sc["ang_true"]], 1) if truth else np.concatenate([sc["C0"], sc["ang0"]], 1)
    iop = true_iop(synth, n_cam, nk) if truth else start_iop(synth, n_cam, nk)
    cam_info = np.array([[synth.YDIR, *SENSOR]] * n_cam)
    return capi.PackedProblem(xy, img, sc["cam"][img], tie_of[pid], sc["X0"][pid], eop, iop, cam_info,
                              sc["X0"][~control], n_img, n_cam, int((~control).sum()))
