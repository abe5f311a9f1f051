"""Generate tests/golden/model_edges.npz: the projection model and its Jacobian over the full fish-eye
field, from a plain 50-digit mpmath model differentiated numerically.

    python tests/golden/make_model_edges.py

What is modelled is the reference's forward model as include/fba.h:40-46 states it (BuildAwG.m:163-207):

    (U, V, W) = M(omega, phi, kappa) (X - Xc),  R = sqrt(U^2 + V^2),  t = atan(R / W)   [atan, NOT atan2]
    fisheye        -c U/R t              pinhole   -c U/W          equisolid  -2c U/R sin(t/2)
    orthographic   -c U/R sin(t)         stereographic  -2c U/R tan(t/2)
    fx = proj_x + xp + dr xbar + decx,   fy = y_dir proj_y + yp + dr ybar + decy

with the distortion evaluated at the OBSERVED coordinates (xbar = x - xp, r^2 = xbar^2 + ybar^2,
dr = sum K_j r^(2j), decx = P1 (ybar^2 + 3 xbar^2) + 2 P2 xbar ybar, decy likewise), rmax = half the sensor's
diagonal, the K_j columns divided by rmax^(2j) and the P columns by rmax^2 (the reference's scaled unknowns),
and the inner-constraint block G of one image (a stated 6 x 7 matrix, no derivative).  A point with W > 0
(more than 90 degrees off-axis) has a defined value under atan; that value is what is pinned.

EVERY derivative is mp.diff (central differences at raised precision) of `forward`: this file holds no
hand-derived partial and shares no chain rule with oracle/fba_oracle.py, oracle/fba_cpu.c or the kernels.
It reads nothing but its own constants and needs mpmath; only tests/test_model_edges_host.py imports it (to
tie the model to tests/golden/jac_golden.json and to regenerate every tenth sample bit for bit).  The .npz
holds float64 arrays only: per sample set the inputs (`*_in`, columns below) and the expected values, plus
`inputs_sha256` (32 bytes) over all inputs.

Sample sets (one image and one camera per sample, as the reference-text test of the Jacobian):
  geo_<type>   nK = 5; off-axis angles GEO_ANGLES (orthographic: 89.9 / 90.1 deg in place of 89.99 / 90.01;
               pinhole without 89.9, 89.99, 90.01), four poses each: two azimuths x (|omega|, |phi|, |kappa| <=
               0.2 | |omega|, |kappa| <= pi, |phi| <= 1.5), range 500-8000, c 300-1500, y_dir alternating;
               R runs from ~1e-6 up (R = 0 is no sample: the reference divides by it)
  dist_nk<k>   k = 1..8, type DIST_TYPES[k - 1], one 45 degree geometry and nine observed image points: the
               principal point itself, (1e-6, 0) and (0, -1e-3) px from it, three inside the sensor, two at
               r = rmax, one at r = 1.2 rmax; K_j within +-10 px / rmax^(2j+1), P within +-1e-6
"""
import hashlib
import math
import os

import mpmath as mp
import numpy as np

DPS = 50
TYPES = ("fisheye", "pinhole", "equisolid", "orthographic", "stereographic")
# input columns
EOP, XYZ, XP, YP, CC, YDIR, BOUNDS, OBS, PP, KK = slice(0, 6), slice(6, 9), 9, 10, 11, 12, slice(13, 17), \
    slice(17, 19), slice(19, 21), 21
GEO_NK = 5
_DEG = math.pi / 180
GEO_ANGLES = [1e-9, 1e-7, 1e-5, 1e-3] + [a * _DEG for a in (1, 45, 75, 85, 89, 89.9, 89.99, 90.01, 91, 100, 135, 179)]
DIST_TYPES = [TYPES[(k - 1) % 5] for k in range(1, 9)]
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model_edges.npz")


def geo_angles(typ):
    if typ == "orthographic":
        swap = {89.99 * _DEG: 89.9 * _DEG, 90.01 * _DEG: 90.1 * _DEG}
        return [swap.get(a, a) for a in GEO_ANGLES if a != 89.9 * _DEG]
    if typ == "pinhole":
        return [a for a in GEO_ANGLES if a not in (89.9 * _DEG, 89.99 * _DEG, 90.01 * _DEG)]
    return list(GEO_ANGLES)


# ---- the model ----------------------------------------------------------------------------------------------
def rot(w, p, k, lib=mp):
    cw, sw, cp, sp, ck, sk = lib.cos(w), lib.sin(w), lib.cos(p), lib.sin(p), lib.cos(k), lib.sin(k)
    return [[ck * cp, cw * sk + ck * sp * sw, sk * sw - ck * cw * sp],
            [-cp * sk, ck * cw - sk * sp * sw, ck * sw + cw * sk * sp],
            [sp, -cp * sw, cp * cw]]


def uvw(eop, xyz):
    M = rot(eop[3], eop[4], eop[5])
    d = [xyz[j] - eop[j] for j in range(3)]
    return [M[i][0] * d[0] + M[i][1] * d[1] + M[i][2] * d[2] for i in range(3)]


def forward(typ, v, x, y, ydir, nk):
    """(fx, fy) at the unknowns v = [Xc Yc Zc omega phi kappa | xp yp c K_1..K_nk P1 P2 | X Y Z]"""
    eop, cam, xyz = v[:6], v[6:11 + nk], v[11 + nk:]
    xp, yp, c, K, P = cam[0], cam[1], cam[2], cam[3:3 + nk], cam[3 + nk:]
    U, V, W = uvw(eop, xyz)
    R = mp.sqrt(U ** 2 + V ** 2)
    if typ == "fisheye":
        px, py = -c * U / R * mp.atan(R / W), -c * V / R * mp.atan(R / W)
    elif typ == "pinhole":
        px, py = -c * U / W, -c * V / W
    elif typ == "equisolid":
        px, py = -2 * c * U / R * mp.sin(mp.atan(R / W) / 2), -2 * c * V / R * mp.sin(mp.atan(R / W) / 2)
    elif typ == "orthographic":
        px, py = -c * U / R * mp.sin(mp.atan(R / W)), -c * V / R * mp.sin(mp.atan(R / W))
    elif typ == "stereographic":
        px, py = -2 * c * U / R * mp.tan(mp.atan(R / W) / 2), -2 * c * V / R * mp.tan(mp.atan(R / W) / 2)
    else:
        raise ValueError(typ)
    xbar, ybar = x - xp, y - yp
    r = mp.sqrt(xbar ** 2 + ybar ** 2)
    dr = sum((K[j - 1] * r ** (2 * j) for j in range(1, nk + 1)), mp.mpf(0))
    decx = P[0] * (ybar ** 2 + 3 * xbar ** 2) + 2 * P[1] * xbar * ybar
    decy = P[1] * (xbar ** 2 + 3 * ybar ** 2) + 2 * P[0] * xbar * ybar
    return px + xp + dr * xbar + decx, ydir * py + yp + dr * ybar + decy


def gblock(Xc, Yc, Zc, w, p):
    """the inner-constraint rows of one image (translations, rotations about X Y Z, scale)"""
    return [[1, 0, 0, 0, -Zc, Yc, Xc],
            [0, 1, 0, Zc, 0, -Xc, Yc],
            [0, 0, 1, -Yc, Xc, 0, Zc],
            [0, 0, 0, -1, -mp.sin(w) * mp.tan(p), mp.cos(w) * mp.tan(p), 0],
            [0, 0, 0, 0, -mp.cos(w), -mp.sin(w), 0],
            [0, 0, 0, 0, mp.sin(w) / mp.cos(p), -mp.cos(w) / mp.cos(p), 0]]


def unknowns(row, nk):
    """the sample's unknowns in forward()'s order, as exact mpf of the float64 inputs"""
    f = [mp.mpf(float(a)) for a in row]
    return f[EOP] + [f[XP], f[YP], f[CC]] + f[KK:KK + nk] + f[PP] + f[XYZ]


def evaluate(typ, row, nk):
    """every expected value of one sample, rounded to float64 once at the end:
    f (2), J (2, 14 + nk) in forward()'s column order with the K_j columns divided by rmax^(2j) and the P columns
    by rmax^2, G (6, 7), scale (nk) = rmax^(2j), theta = the off-axis angle atan2(R, -W) of the inputs"""
    mp.mp.dps = DPS
    v = unknowns(row, nk)
    x, y, ydir = (mp.mpf(float(a)) for a in (row[OBS][0], row[OBS][1], row[YDIR]))
    xmin, ymin, xmax, ymax = (mp.mpf(float(a)) for a in row[BOUNDS])
    rmax = mp.sqrt(((xmax - xmin) / 2) ** 2 + ((ymax - ymin) / 2) ** 2)
    scale = [rmax ** (2 * j) for j in range(1, nk + 1)]
    col_scale = [mp.mpf(1)] * 9 + scale + [scale[0], scale[0]] + [mp.mpf(1)] * 3
    f = forward(typ, v, x, y, ydir, nk)
    J = np.empty((2, len(v)))
    for q in range(len(v)):
        for i in range(2):
            J[i, q] = float(mp.diff(lambda t: forward(typ, v[:q] + [t] + v[q + 1:], x, y, ydir, nk)[i], v[q])
                            / col_scale[q])
    U, V, W = uvw(v[:6], v[11 + nk:])
    return dict(f=np.array([float(f[0]), float(f[1])]), J=J,
                G=np.array([[float(e) for e in r] for r in gblock(*v[:5])]),
                scale=np.array([float(s) for s in scale]),
                theta=np.array(float(mp.atan2(mp.sqrt(U ** 2 + V ** 2), -W))))


# ---- the samples (float64 inputs; plain numpy) ---------------------------------------------------------------
def _camera(rng, nk):
    """sensor bounds, principal point, c, K, P as tests/golden/make_jac_golden.dist_samples draws them"""
    xmin, ymin = rng.uniform(-10, 10, 2)
    xmax, ymax = xmin + rng.uniform(1500, 2500), ymin + rng.uniform(1500, 2500)
    rmax = math.hypot((xmax - xmin) / 2, (ymax - ymin) / 2)
    xp, yp = 0.5 * (xmin + xmax) + rng.uniform(-20, 20), 0.5 * (ymin + ymax) + rng.uniform(-20, 20)
    K = [rng.uniform(-10, 10) / rmax ** (2 * j + 1) for j in range(1, nk + 1)]
    P = list(rng.uniform(-1e-6, 1e-6, 2))
    return dict(bounds=[xmin, ymin, xmax, ymax], rmax=rmax, xp=xp, yp=yp, c=rng.uniform(300, 1500), K=K, P=P)


def _pose(rng, theta, az, large):
    C = rng.uniform(-5000, 5000, 3)
    if large:
        w, p, k = rng.uniform(-math.pi, math.pi), rng.uniform(-1.5, 1.5), rng.uniform(-math.pi, math.pi)
    else:
        w, p, k = rng.uniform(-0.2, 0.2, 3)
    dist = rng.uniform(500, 8000)
    d_cam = dist * np.array([math.sin(theta) * math.cos(az), math.sin(theta) * math.sin(az), -math.cos(theta)])
    X = C + np.array(rot(w, p, k, lib=math)).T @ d_cam
    return list(C) + [w, p, k], list(X)


def _row(eop, xyz, cam, ydir, x, y):
    return eop + xyz + [cam["xp"], cam["yp"], cam["c"], ydir] + cam["bounds"] + [x, y] + cam["P"] + cam["K"]


def geometry_inputs(typ):
    rng = np.random.default_rng(20260000 + TYPES.index(typ))
    rows, nominal = [], []
    for theta in geo_angles(typ):
        az = rng.uniform(-math.pi, math.pi, 2)
        for q in range(4):
            cam = _camera(rng, GEO_NK)
            eop, xyz = _pose(rng, theta, az[q % 2], large=q >= 2)
            b = cam["bounds"]
            rows.append(_row(eop, xyz, cam, 1.0 if len(rows) % 2 else -1.0, rng.uniform(b[0], b[2]),
                             rng.uniform(b[1], b[3])))
            nominal.append(theta)
    return np.array(rows), np.array(nominal)


def distortion_inputs(nk):
    rng = np.random.default_rng(20261000 + nk)
    cam = _camera(rng, nk)
    eop, xyz = _pose(rng, 45 * _DEG, rng.uniform(-math.pi, math.pi), large=False)
    b, xp, yp, rmax = cam["bounds"], cam["xp"], cam["yp"], cam["rmax"]
    obs = [(xp, yp), (xp + 1e-6, yp), (xp, yp - 1e-3)]
    obs += [(rng.uniform(b[0], b[2]), rng.uniform(b[1], b[3])) for _ in range(3)]
    for rr in (1.0, 1.0, 1.2):
        a = rng.uniform(-math.pi, math.pi)
        obs.append((xp + rr * rmax * math.cos(a), yp + rr * rmax * math.sin(a)))
    return np.array([_row(eop, xyz, cam, 1.0 if i % 2 else -1.0, x, y) for i, (x, y) in enumerate(obs)])


def sample_sets():
    """{name: (type, nK, inputs)} in the fixture's order"""
    out = {}
    for typ in TYPES:
        out["geo_" + typ] = (typ, GEO_NK, geometry_inputs(typ)[0])
    for nk in range(1, 9):
        out[f"dist_nk{nk}"] = (DIST_TYPES[nk - 1], nk, distortion_inputs(nk))
    return out


def inputs_sha256(inputs):
    """inputs: {name: array}; the digest over name and bytes in sorted order, as 32 numbers"""
    h = hashlib.sha256()
    for name in sorted(inputs):
        h.update(name.encode() + np.ascontiguousarray(inputs[name], dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).astype(np.float64)


def main():
    out, inputs = {}, {}
    for name, (typ, nk, rows) in sample_sets().items():
        vals = [evaluate(typ, r, nk) for r in rows]
        inputs[name + "_in"] = rows
        for key in ("f", "J", "G", "scale", "theta"):
            out[f"{name}_{key}"] = np.stack([v[key] for v in vals])
        th = np.degrees(out[name + "_theta"])
        print(f"{name}: {len(rows)} samples ({typ}, nK = {nk}), off-axis {th.min():.3g} .. {th.max():.6g} deg")
    out.update(inputs)
    out["inputs_sha256"] = inputs_sha256(inputs)
    np.savez_compressed(DST, **out)
    print("wrote", DST, os.path.getsize(DST), "bytes")


if __name__ == "__main__":
    main()
