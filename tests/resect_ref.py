"""numpy restatement of the space resection for tests/test_resect_host.py and tests/test_gpu_resect.py.

Written from include/fba.h's description of fba_resect / fba_resect_host and BuildAwG.m's model, not from the device
code.  The linear solution is computed two ways -- eigh of the 12 x 12 Gram matrix, and the SVD of the stacked 3n x 12
matrix with the rows in reversed order -- whose spread is the yardstick of the linear tests; the refinement uses an
analytic Jacobian (the rotation as a product of three elementary rotations, its derivatives by the product rule)."""
import numpy as np

import intersect_ref as ir

GIMBAL = 1e-14


def r1(w):
    c, s = np.cos(w), np.sin(w)
    return np.array([[1, 0, 0], [0, c, s], [0, -s, c]]), np.array([[0, 0, 0], [0, -s, c], [0, -c, -s]])


def r2(p):
    c, s = np.cos(p), np.sin(p)
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]]), np.array([[-s, 0, -c], [0, 0, 0], [c, 0, -s]])


def r3(k):
    c, s = np.cos(k), np.sin(k)
    return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]]), np.array([[-s, c, 0], [-c, -s, 0], [0, 0, 0]])


def rot_and_derivatives(w, p, k):
    """M = R3(kappa) R2(phi) R1(omega) (= intersect_ref.rot) and dM / d(omega, phi, kappa)"""
    (A, dA), (B, dB), (Cc, dC) = r1(w), r2(p), r3(k)
    return Cc @ B @ A, Cc @ B @ dA, Cc @ dB @ A, dC @ B @ A


def angles_of(M):
    ph = np.arcsin(np.clip(M[2, 0], -1.0, 1.0))
    if M[2, 1] ** 2 + M[2, 2] ** 2 <= GIMBAL:
        return np.array([0.0, ph, np.arctan2(M[0, 1], M[1, 1])])
    return np.array([np.arctan2(-M[2, 1], M[2, 2]), ph, np.arctan2(-M[1, 0], M[0, 0])])


def cross_matrix(d):
    return np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])


def linear(xyz, d, method="eigh"):
    """(C, M, ratio, lambda) of the ray-based DLT; ratio from eigvalsh of the Gram matrix in both methods"""
    xyz, d = np.asarray(xyz, dtype=np.float64), np.asarray(d, dtype=np.float64)
    m = xyz.mean(0)
    s = np.sqrt(((xyz - m) ** 2).sum(1)).mean()
    Xt = np.concatenate([(xyz - m) / s, np.ones((len(xyz), 1))], 1)
    G = sum(np.kron(np.eye(3) - np.outer(di, di), np.outer(x, x)) for di, x in zip(d, Xt))
    lam = np.linalg.eigvalsh(G)
    if method == "eigh":
        p = np.linalg.eigh(G)[1][:, 0]
    else:
        rows = [cross_matrix(di) @ np.kron(np.eye(3), x[None, :]) for di, x in zip(d[::-1], Xt[::-1])]
        p = np.linalg.svd(np.concatenate(rows))[2][-1]
    P = p.reshape(3, 4)
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    U, sv, Vt = np.linalg.svd(P[:, :3])
    M = U @ Vt
    t = P[:, 3] / sv.mean()
    return m - s * M.T @ t, M, lam[1] / lam[-1], sv.mean()


def evaluate(typ, eop, xyz, uv, c, ydir, sx, sy):
    """residuals (n, 2), the normal matrix N (6, 6) and the gradient g (6) at eop"""
    M, dw, dp, dk = rot_and_derivatives(*eop[3:])
    e = xyz - eop[:3]
    n = len(xyz)
    Mn = np.broadcast_to(M, (n, 3, 3))
    px, py, jx, jy = ir.project_tie(typ, Mn, e, np.full(n, c), np.full(n, ydir))
    w = np.stack([px - uv[:, 0], py - uv[:, 1]], -1)
    jux, juy = jx @ M.T, jy @ M.T                       # derivatives to (U, V, W): jx = jux M, M orthonormal
    J = np.zeros((n, 2, 6))
    J[:, 0, :3], J[:, 1, :3] = -jx, -jy
    for a, dM in enumerate((dw, dp, dk)):
        duvw = e @ dM.T
        J[:, 0, 3 + a] = (jux * duvw).sum(1)
        J[:, 1, 3 + a] = (juy * duvw).sum(1)
    pw = np.array([1 / sx ** 2, 1 / sy ** 2])
    N = np.einsum("nra,r,nrb->ab", J, pw, J)
    g = np.einsum("nra,r,nr->a", J, pw, w)
    return w, N, g


def rms_of(w):
    return np.sqrt((w * w).sum() / len(w))


def resect_image(typ, xyz, uv, c, ydir, refine_iters=10, refine_tol=1e-10, min_ratio=1e-6, sx=0.3, sy=0.3,
                 method="eigh"):
    """the header's procedure for one image: dict(n, status, ratio, C_lin, M_lin, eop_lin, eop, rms_lin, rms_fin, iters,
    dist, front); uv (n, 5): xu yu d of the usable points only"""
    xyz, uv = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(uv, dtype=np.float64).reshape(-1, 5)
    out = dict(n=len(xyz), status=1, ratio=0.0, rms_lin=0.0, rms_fin=0.0, iters=0)
    if len(xyz) < 6:
        return out
    C, M, ratio, _ = linear(xyz, uv[:, 2:], method)
    out.update(status=2, ratio=ratio)
    if not ratio >= min_ratio:
        return out
    lin = np.concatenate([C, angles_of(M)])
    w, N, g = evaluate(typ, lin, xyz, uv, c, ydir, sx, sy)
    x, it = lin.copy(), 0
    rms_lin = rms_fin = rms_of(w)
    status = 0
    for it in range(1, refine_iters + 1):
        try:
            step = np.linalg.solve(N, g)
            np.linalg.cholesky(N)
        except np.linalg.LinAlgError:
            status = 3
            break
        tol = refine_tol * np.sqrt(((xyz - x[:3]) ** 2).sum(1)).mean()
        x = x - step
        w, N, g = evaluate(typ, x, xyz, uv, c, ydir, sx, sy)
        rms_fin = rms_of(w)
        if not np.isfinite(rms_fin):
            status = 3
            break
        if np.abs(step[:3]).max() <= tol and np.abs(step[3:]).max() <= refine_tol:
            break
    if status == 3 or not rms_fin <= rms_lin + 1e-9:
        status, x, rms_fin = 3, lin.copy(), rms_lin
    Mx = ir.rot(*x[3:])
    front = float(((uv[:, 2:] * ((xyz - x[:3]) @ Mx.T)).sum(1) > 0).mean())
    out.update(status=status, C_lin=C, M_lin=M, eop_lin=lin, eop=x, rms_lin=rms_lin, rms_fin=rms_fin,
               iters=it if refine_iters else 0, dist=np.sqrt(((xyz - C) ** 2).sum(1)).mean(), front=front)
    return out


# ---- packed problems ------------------------------------------------------------------------------------------------
def object_points(pk, tie_xyz=None):
    """per PHO row the object point: xyz_fixed for control rows, tie_xyz (default tie0) for tie rows"""
    X = pk.xyz_fixed.reshape(-1, 3).copy()
    t = (pk.tie0 if tie_xyz is None else np.asarray(tie_xyz)).reshape(-1, 3)
    rows = pk.tie >= 0
    X[rows] = t[pk.tie[rows]]
    return X


def image_rows(pk, pb, e, use="control"):
    """the usable PHO rows of image e, ascending"""
    rows = np.nonzero((pk.img == e) & (pb.rst == 0) & ((pk.tie < 0) | (use == "all")))[0]
    return rows


def resect_all(pk, pb, use="control", **kw):
    """resect_image for every image of a packed problem at its start values (pb: intersect_ref.Problem of pk)"""
    X = object_points(pk)
    out = []
    for e in range(pk.n_img):
        rows = image_rows(pk, pb, e, use)
        out.append(resect_image(pb.typ, X[rows], pb.uv[rows], pb.c[rows[0]] if len(rows) else 1.0,
                                pb.ydir[rows[0]] if len(rows) else 1.0, **kw))
    return out
