"""CPU: the projection model and its Jacobian over the FULL fish-eye field against a reference that shares no
chain rule with the code under test.

tests/golden/model_edges.npz holds numbers from a plain 50-digit mpmath model (tests/golden/make_model_edges.py:
the five projections as include/fba.h:40-46 states them, atan not atan2, distortion at the observed coordinates,
rmax and the rmax^(2j) scaling, G), every derivative by mp.diff of that forward model.  Its samples are where
tests/golden/jac_golden.json (0.02 rad .. 80 deg, W < 0, omega phi kappa within +-45 deg, nK = 5, no image point at the
principal point or at r >= rmax) does not go: off-axis 1e-9 rad .. 179 deg with large rotations (geo_<type>), and for
every nK = 1..8 image points at, next to and far from the principal point up to 1.2 rmax (dist_nk<k>).

1. test_oracle_within_bars[set]: oracle.point_model and oracle.build_awg on every sample, at a TENTH of the bars
   tests/test_gpu_model_edges.py holds the device to -- the condition that makes those bars meaningful:
     * position / rotation / tie entries: |d| <= 1e-13 x the largest reference entry of that group in that row
       (a row's entries share U, V, W, whose rounding is absolute on the scale of the row, not of the entry);
     * projected value w + x: |d| <= 1e-13 c;
     * camera columns (xp yp c K_j P): |d| <= 1e-13 x max(|entry|, the column's largest entry over the sample set)
       -- a relative bar per entry with that floor, which is the larger of the two: the c column is -U s, U a
       dot product whose error is absolute on the scale of |X - Xc|, so an entry near the axis cannot be held to
       a fraction of itself;
     * G: 1e-14 of the image block's largest entry; dist_scaling: 1e-14 relative (rmax^(2j), j <= 8: 2j ulps of
       rmax and one of the power, <= 1.9e-15); entries outside a sample's own blocks and the K / P columns of the
       principal-point sample (exactly 0 in the reference): exactly 0.
   Measured (max over each set's samples, in units of what each bar scales; position, rotation, tie, camera, f / c):
     geo_fisheye        6.4e-16 5.1e-16 6.4e-16 4.0e-16 7.0e-16
     geo_pinhole        1.8e-15 1.8e-15 1.8e-15 7.6e-16 4.1e-14   (all five worst at 89 deg)
     geo_equisolid      7.1e-16 6.1e-16 7.1e-16 6.9e-16 6.7e-16
     geo_orthographic   3.1e-15 1.1e-15 3.1e-15 5.5e-16 5.9e-16   (position, rotation, tie worst at 90.1 deg)
     geo_stereographic  8.1e-16 7.0e-16 8.1e-16 4.3e-16 7.4e-16
     dist_nk1..8        <= 4.2e-16 position / rotation / tie, <= 1.3e-15 camera, <= 4.6e-16 f / c
     G <= 4.2e-19 of the block's largest entry, dist_scaling <= 1.8e-15 relative
   so every listed sample stays within 1e-13 and none had to be replaced.
2. test_mpmath_model_matches_reference_text[type]: the same mpmath model on jac_golden.json's 24 "distortion"
   points against every number stored there (from the reference's own expression text): 1e-14 relative.  This
   ties the new reference to the reference's text where the domains overlap.
3. test_fixture_integrity: the stored hash of the inputs, the inputs as the generator draws them, the sample lists
   (angles per type, image points per nK), and every tenth sample regenerated bit for bit.
(2 and 3's regeneration need mpmath; the fixture and test 1 do not.)
"""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

TYPES = ("fisheye", "pinhole", "equisolid", "orthographic", "stereographic")
SETS = ["geo_" + t for t in TYPES] + [f"dist_nk{k}" for k in range(1, 9)]
CPU_BAR = 1e-13  # the device bar of tests/test_gpu_model_edges.py is 10 x this
# input columns of a sample (tests/golden/make_model_edges.py)
EOP, XYZ, XP, YP, CC, YDIR, BOUNDS, OBS, PP, KK = slice(0, 6), slice(6, 9), 9, 10, 11, 12, slice(13, 17), \
    slice(17, 19), slice(19, 21), 21


class EdgeSet:
    """one sample set of the fixture laid out as a problem with one image and one camera per sample"""

    def __init__(self, g, name):
        self.name, rows = name, g[name + "_in"]
        self.nk = rows.shape[1] - KK
        self.n, self.cw = len(rows), 5 + self.nk
        self.typ = name[4:] if name.startswith("geo_") else TYPES[(self.nk - 1) % 5]
        self.eop, self.xyz, self.xy = rows[:, EOP], rows[:, XYZ], rows[:, OBS]
        self.c = rows[:, CC]
        self.iop = np.column_stack([rows[:, XP], rows[:, YP], rows[:, CC], rows[:, KK:], rows[:, PP]])
        self.cam_info = np.column_stack([rows[:, YDIR], rows[:, BOUNDS]])
        self.xhat = np.concatenate([self.eop.reshape(-1), self.iop.reshape(-1), self.xyz.reshape(-1)])
        self.f, self.J, self.G, self.scale = (g[f"{name}_{k}"] for k in ("f", "J", "G", "scale"))
        self.theta = g[name + "_theta"]
        self.settings = {"type": self.typ, "Num_Radial_Distortions": self.nk, "Inner_Constraints": 1, "Iteration_Cap": 1,
                         "threshold": 1e-6, "Meas_std": 1.0, "Meas_std_y": 1.0}
        for k in ("Xc", "Yc", "Zc", "w", "p", "k", "c", "xp", "yp", "radial", "decent"):
            self.settings["Estimate_" + k] = 1

    def blocks(self, i):
        """column slices of sample i in the reference layout: EOP, camera, tie"""
        n, cw = self.n, self.cw
        return slice(6 * i, 6 * i + 6), slice(6 * n + cw * i, 6 * n + cw * (i + 1)), \
            slice(6 * n + cw * n + 3 * i, 6 * n + cw * n + 3 * i + 3)

    def oracle_data(self):
        from fba_oracle import Data
        idx = np.arange(self.n)
        return Data(settings=self.settings, x=self.xy[:, 0].copy(), y=self.xy[:, 1].copy(),
                    target=[f"T{i}" for i in idx], image=[f"I{i}" for i in idx], ext_index=idx, cam_num=idx,
                    tie_index=idx, eop_fixed=self.eop, iop_fixed=self.iop, bounds=self.cam_info, xyz_fixed=self.xyz,
                    numImg=self.n, numCam=self.n, n=2 * self.n, numGCP=self.n, numtie=self.n)

    def cost(self):
        """sum p w^2 of the fixture's projected values (p = 1), added exactly"""
        import math
        return math.fsum(((self.f - self.xy) ** 2).reshape(-1))


@pytest.fixture(scope="session")
def edges():
    g = np.load(os.path.join(GOLDEN, "model_edges.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def check_awg(es, A, w, G, ds, bar):
    """A, w, G, dist_scaling of one sample set against the fixture at `bar` (the module docstring's rules);
    returns the measured maxima (in units of the quantity each bar scales), printed before anything is asserted"""
    n, nk, cw = es.n, es.nk, es.cw
    u = 6 * n + cw * n + 3 * n
    assert A.shape == (2 * n, u) and w.shape == (2 * n,) and G.shape == (u, 7) and ds.shape == (n, 2 + nk)
    Aref, scale_of = np.zeros((2 * n, u)), np.zeros((2 * n, u))
    cam_colmax = np.abs(es.J[:, :, 6:6 + cw]).max(axis=(0, 1))
    groups = {"position": [], "rotation": [], "tie": [], "camera": []}
    for i in range(n):
        rows = slice(2 * i, 2 * i + 2)
        be, bc, bt = es.blocks(i)
        J = es.J[i]
        Aref[rows, be], Aref[rows, bc], Aref[rows, bt] = J[:, :6], J[:, 6:6 + cw], J[:, 6 + cw:]
        scale_of[rows, be.start:be.start + 3] = np.abs(J[:, 0:3]).max(axis=1, keepdims=True)
        scale_of[rows, be.start + 3:be.stop] = np.abs(J[:, 3:6]).max(axis=1, keepdims=True)
        scale_of[rows, bt] = np.abs(J[:, 6 + cw:]).max(axis=1, keepdims=True)
        scale_of[rows, bc] = np.maximum(np.abs(J[:, 6:6 + cw]), cam_colmax)
        groups["position"].append((rows, slice(be.start, be.start + 3)))
        groups["rotation"].append((rows, slice(be.start + 3, be.stop)))
        groups["tie"].append((rows, bt))
        groups["camera"].append((rows, bc))
    inside = scale_of > 0
    assert np.isfinite(A).all() and np.isfinite(w).all()
    rel = np.zeros_like(A)
    rel[inside] = np.abs(A - Aref)[inside] / scale_of[inside]
    got = {k: max(float(rel[r, c].max()) for r, c in v) for k, v in groups.items()}
    e_f = np.abs(w.reshape(n, 2) + es.xy - es.f) / es.c[:, None]
    got["f/c"] = float(e_f.max())
    Gref = np.zeros((u, 7))
    e_g = 0.0
    for i in range(n):
        Gref[6 * i:6 * i + 6] = es.G[i]
        e_g = max(e_g, float(np.abs(G[6 * i:6 * i + 6] - es.G[i]).max() / np.abs(es.G[i]).max()))
    got["G"] = e_g
    got["dist_scaling"] = float(np.abs(ds[:, 2:] / es.scale - 1.0).max())
    worst = {k: int(np.argmax([rel[r, c].max() for r, c in v])) for k, v in groups.items()}
    print(f"model edges {es.name} ({es.typ}, nK = {nk}, {n} samples) bar {bar:.0e}: "
          + " ".join(f"{k}={v:.1e}" for k, v in got.items())
          + " | worst sample (off-axis deg): "
          + " ".join(f"{k}@{np.degrees(es.theta[i]):.6g}" for k, i in worst.items())
          + f" f/c@{np.degrees(es.theta[int(e_f.max(axis=1).argmax())]):.6g}")
    for k in ("position", "rotation", "tie", "camera", "f/c"):
        assert got[k] <= bar, (es.name, k, got[k], bar)
    assert got["G"] <= 1e-14 and got["dist_scaling"] <= 1e-14, (es.name, got)
    # nothing outside a sample's own blocks, in A and in G
    assert (A[~inside] == 0).all() and (G[Gref == 0] == 0).all()
    if es.name.startswith("dist_"):  # sample 0 is the principal point itself: what is exactly 0 there stays 0
        got0, ref0 = A[0:2, es.blocks(0)[1]], es.J[0][:, 6:6 + cw]
        assert (ref0[:, 3:] == 0).all(), "the K and P columns vanish at the principal point"
        assert (got0[ref0 == 0] == 0).all(), got0
    return got


@pytest.mark.parametrize("name", SETS)
def test_oracle_within_bars(oracle, edges, name):
    es = EdgeSet(edges, name)
    A, w, G, ds = oracle.build_awg(es.oracle_data(), es.xhat)
    check_awg(es, A, w, G, ds, CPU_BAR)
    # point_model called directly (what build_awg scatters): the same rules on its own outputs
    t, nk, cw = TYPES.index(es.typ), es.nk, es.cw
    m = oracle.point_model(t, es.eop, es.xyz, es.iop[:, 0], es.iop[:, 1], es.c, es.iop[:, 3:3 + nk], es.iop[:, 3 + nk:],
                           es.cam_info[:, 0], es.xy[:, 0], es.xy[:, 1])
    assert (np.abs(m["f"] - es.f) <= CPU_BAR * es.c[:, None]).all()
    for got, ref in ((m["J_eop"][:, :, :3], es.J[:, :, :3]), (m["J_eop"][:, :, 3:], es.J[:, :, 3:6]),
                     (m["J_xyz"], es.J[:, :, 6 + cw:])):
        assert (np.abs(got - ref) <= CPU_BAR * np.abs(ref).max(axis=2, keepdims=True)).all()
    for key, q in (("J_xp", 6), ("J_yp", 7), ("J_c", 8)):
        ref = es.J[:, :, q]
        assert (np.abs(m[key] - ref) <= CPU_BAR * np.maximum(np.abs(ref), np.abs(ref).max())).all(), key


def test_sample_lists(edges):
    """the fixture has the samples it was written for (no mpmath needed)"""
    deg = np.pi / 180
    base = [1e-9, 1e-7, 1e-5, 1e-3] + [a * deg for a in (1, 45, 75, 85, 89, 89.9, 89.99, 90.01, 91, 100, 135, 179)]
    want = {t: list(base) for t in TYPES}
    want["orthographic"] = [a for a in base if a not in (89.99 * deg, 90.01 * deg)] + [90.1 * deg]
    want["pinhole"] = [a for a in base if a not in (89.9 * deg, 89.99 * deg, 90.01 * deg)]
    r_min = np.inf
    for t in TYPES:
        es = EdgeSet(edges, "geo_" + t)
        assert es.nk == 5 and es.n == 4 * len(want[t])
        th = es.theta.reshape(-1, 4)
        # the inputs are float64, so the angle they realise differs from the nominal one by the rounding of
        # X - Xc (<= 1e-12 m over a range >= 500 m) -- and by no more
        np.testing.assert_allclose(th, np.sort(want[t])[:, None] * np.ones(4), rtol=1e-9, atol=1e-13)
        large = np.abs(es.eop[:, 3:]).max(axis=1).reshape(-1, 4) > 0.2
        assert (~large[:, :2]).all() and large[:, 2:].all()
        assert (es.cam_info[:, 0].reshape(-1, 2) == [-1.0, 1.0]).all()
        rng_ = np.linalg.norm(es.xyz - es.eop[:, :3], axis=1)
        assert (rng_ > 499).all() and (rng_ < 8001).all() and (es.c >= 300).all() and (es.c <= 1500).all()
        r_min = min(r_min, float((rng_ * np.sin(es.theta)).min()))
        assert np.isfinite(es.f).all() and np.isfinite(es.J).all()
    assert 1e-7 < r_min < 1e-5  # R from about 1e-6 m up; R = 0 is no sample
    for nk in range(1, 9):
        es = EdgeSet(edges, f"dist_nk{nk}")
        assert es.nk == nk and es.n == 9 and np.allclose(es.theta, 45 * deg, rtol=1e-12)
        xb, yb = (es.xy - es.iop[:, :2]).T
        b = es.cam_info[0, 1:]
        rmax = np.hypot((b[2] - b[0]) / 2, (b[3] - b[1]) / 2)
        assert (xb[0], yb[0]) == (0.0, 0.0)
        assert abs(xb[1] - 1e-6) < 1e-12 and yb[1] == 0.0 and xb[2] == 0.0 and abs(yb[2] + 1e-3) < 1e-12
        inside = (es.xy[3:6] > b[:2]).all() and (es.xy[3:6] < b[2:]).all()
        assert inside
        np.testing.assert_allclose(np.hypot(xb, yb)[6:], np.array([1.0, 1.0, 1.2]) * rmax, rtol=1e-12)
        K = es.iop[0, 3:3 + nk]
        assert (np.abs(K) * rmax ** (2 * np.arange(1, nk + 1) + 1) <= 10).all() and (np.abs(es.iop[0, 3 + nk:]) <= 1e-6).all()


def _generator():
    pytest.importorskip("mpmath")
    sys.path.insert(0, GOLDEN)
    import make_model_edges
    return make_model_edges


def test_fixture_integrity(edges):
    """the stored input hash; the inputs as the generator draws them; every tenth sample regenerated bit for bit"""
    import hashlib
    h = hashlib.sha256()
    for name in sorted(s + "_in" for s in SETS):
        h.update(name.encode() + np.ascontiguousarray(edges[name], dtype=np.float64).tobytes())
    assert bytes(edges["inputs_sha256"].astype(np.uint8)) == h.digest()
    assert all(v.dtype == np.float64 for v in edges.values())
    assert os.path.getsize(os.path.join(GOLDEN, "model_edges.npz")) < 400 * 1024
    gen = _generator()
    sets = gen.sample_sets()
    assert list(sets) == SETS
    count = 0
    for name, (typ, nk, drawn) in sets.items():
        rows = edges[name + "_in"]
        # the generator still draws these samples (X = C + M'd goes through the host's sin / cos: not bit for bit)
        np.testing.assert_allclose(drawn, rows, rtol=1e-9, atol=1e-9, err_msg=name)
        assert typ == EdgeSet(edges, name).typ
        for i in range(len(rows)):
            if count % 10 == 0:  # from the STORED inputs: mpmath's arithmetic is the same everywhere
                vals = gen.evaluate(typ, rows[i], nk)
                for key, v in vals.items():
                    assert v.tobytes() == edges[f"{name}_{key}"][i].tobytes(), (name, i, key)
            count += 1


@pytest.mark.parametrize("t", range(5))
def test_mpmath_model_matches_reference_text(t):
    """make_model_edges.evaluate on jac_golden.json's 24 "distortion" points (nK = 5) against every value stored
    there -- fx fy, the twelve EOP and six tie partials, d/dc, the xp / yp columns, rmax, the rmax^(2j) scaling, the
    scaled K / P columns and G, all from the reference's own expression text at 40 digits: 1e-14 relative"""
    from test_oracle import EOP_NAMES, TIE_NAMES
    gen = _generator()
    with open(os.path.join(GOLDEN, "jac_golden.json")) as fh:
        g = json.load(fh)["distortion"]
    typ, nk = TYPES[t], g["nk"]
    assert len(g["points"]) == 24 and nk == 5
    worst = 0.0

    def close(a, b, what):
        nonlocal worst
        assert abs(a - b) <= 1e-14 * abs(b), (typ, what, a, b)
        worst = max(worst, abs(a - b) / abs(b)) if b else worst
    for i, (p, v) in enumerate(zip(g["points"], g["values"][typ])):
        row = np.array([p["Xc"], p["Yc"], p["Zc"], p["w"], p["p"], p["k"], p["X"], p["Y"], p["Z"], p["xp"], p["yp"],
                        p["c"], p["y_dir"], p["xmin"], p["ymin"], p["xmax"], p["ymax"], p["x"], p["y"], *p["P"], *p["K"]])
        m = gen.evaluate(typ, row, nk)
        J, cam, tie = m["J"], 6, 11 + nk
        close(m["f"][0], v["fx"], (i, "fx"))
        close(m["f"][1], v["fy"], (i, "fy"))
        for nm, (r, col) in EOP_NAMES.items():
            close(J[r, col], v[nm], (i, nm))
        for nm, (r, col) in TIE_NAMES.items():
            close(J[r, tie + col], v[nm], (i, nm))
        for q, par in enumerate(("A_xp", "A_yp")):
            close(J[0, cam + q], v[par][0], (i, par, "x"))
            close(J[1, cam + q], v[par][1], (i, par, "y"))
        close(J[0, cam + 2], v["Ax_c"], (i, "Ax_c"))
        close(J[1, cam + 2], v["Ay_c"], (i, "Ay_c"))
        close(m["scale"][0] ** 0.5, v["rmax"], (i, "rmax"))
        for j in range(nk):
            close(J[0, cam + 3 + j], v["Ax_K"][j], (i, "Ax_K", j))
            close(J[1, cam + 3 + j], v["Ay_K"][j], (i, "Ay_K", j))
            close(m["scale"][j], v["scale"][j], (i, "scale", j))
        for j in range(2):
            close(J[0, cam + 3 + nk + j], v["Ax_P"][j], (i, "Ax_P", j))
            close(J[1, cam + 3 + nk + j], v["Ay_P"][j], (i, "Ay_P", j))
        for a in range(6):
            for b in range(7):
                close(m["G"][a, b], v["G"][a][b], (i, "G", a, b))
    print(f"mpmath model vs the reference text, {typ}: worst relative difference {worst:.1e}")
