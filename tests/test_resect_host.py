"""Host side of the space resection (no GPU): fba_resect_host -- csrc/fba_resect.h's per-image routines, the arithmetic
k_resect runs on the device -- against the numpy restatement (tests/resect_ref.py), its edge cases, report.write_rsc's
table, the image-list builder and a stand-alone sanitizer program (tests/resect_check.cpp).

Scenes are synth.generate(12, 40, seed=3, obs_per_point=9) with max_theta_deg as in test_gpu_intersect.py; an image's
points are the scene's points it sees.

Bars, none from a run of the code under test:
  exact   noise 0, true EOP / IOP: linear |C - C_true| <= 1e-8 units, |M - M_true| <= 1e-11 (the restatement gives
          2.1e-11 .. 6.6e-11 and <= 2.2e-14; the margin is left for libm and the order of the sums); refined
          |C - C_true| <= 1e-8, RMS <= 1e-8 px (the restatement: <= 1.5e-12, <= 2.5e-13)
  noisy   noise 0.3, start IOPs, points at X0: linear C against the restatement to max(1e-9 x the mean distance, 100 x
          the spread of the restatement's two ways), M likewise with the distance left out; the ratio to 1e-10; refined
          C to 100 x refine_tol x the distance, |M - M_ref| <= 100 x refine_tol; RMS final <= RMS linear for the
          restatement alone
  phi = +-pi/2   the rotation rebuilt from the angles against the truth to 1e-6: M's entries carry ~1e-14 of rounding,
          so cos phi (the norm of (M21, M22)) is known to ~1e-7 only, which is where the header switches to omega = 0
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import intersect_ref as ir
import resect_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fish-eye_bundle_adjustment_amd", "csrc")
_CACHE = {}


def _theta(typ):
    return 60.0 if typ in ("pinhole", "orthographic") else 80.0


def _scene(typ, noise):
    from fba_amd import synth
    key = (typ, noise)
    if key not in _CACHE:
        _CACHE[key] = synth.generate(12, 40, seed=3, obs_per_point=9, noise=noise, typ=typ, max_theta_deg=_theta(typ))
    return synth, _CACHE[key]


def _image_inputs(fba, synth, sc, typ, nk, truth, e):
    """(xyz, uv, c, ydir) of image e: its points (X_true with the true IOPs, X0 with the start IOPs) and rays"""
    iop = (ir.true_iop if truth else ir.start_iop)(synth, 1, nk)[0]
    ct = np.concatenate([iop[:3], [synth.YDIR], iop[3 + nk:], iop[3:3 + nk]])
    rows = np.nonzero(sc["img"] == e)[0]
    X = (sc["X_true"] if truth else sc["X0"])[sc["pid"][rows]]
    xy = sc["xy"][rows]
    if truth:
        # exact pixels of exactly this camera: synth's K0 has two terms, so with nk = 1 the scene's own pixels are not
        # those of the nk-term camera; the restatement's forward model (longdouble, rounded to fp64) gives them
        M = ir.rot(*sc["ang_true"][e])
        xy = ir.forward(typ, (X - sc["C_true"][e]) @ M.T, ct).astype(np.float64)
        if nk >= 2:
            assert np.abs(xy - sc["xy"][rows]).max() <= 1e-9
    uv, st = fba.capi.unproject_host(typ, xy, ct)
    assert (st == 0).all()
    return X, uv, ct[2], ct[3]


# ---- 1. exact data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 5, 8])
@pytest.mark.parametrize("typ", ir.TYPES)
def test_exact_at_the_truth(fba, typ, nk):
    synth, sc = _scene(typ, 0.0)
    M_true = ir.rot(sc["ang_true"][:, 0], sc["ang_true"][:, 1], sc["ang_true"][:, 2])
    worst = np.zeros(4)
    for e in range(12):
        X, uv, c, ydir = _image_inputs(fba, synth, sc, typ, nk, True, e)
        assert len(X) >= 6
        lin, ql, sl = fba.capi.resect_host(typ, X, uv, c, ydir, refine_iters=0)
        fin, qf, sf = fba.capi.resect_host(typ, X, uv, c, ydir)
        assert sl == 0 and sf in (0, 3) and ql[0] == len(X) and ql[2] == ql[3] and ql[4] in (0.0, 1.0)
        worst = np.maximum(worst, [np.abs(lin[:3] - sc["C_true"][e]).max(), np.abs(ir.rot(*lin[3:]) - M_true[e]).max(),
                                   np.abs(fin[:3] - sc["C_true"][e]).max(), qf[3]])
    print(f"exact {typ} nk {nk}: linear |C - C_true| {worst[0]:.2e}, |M - M_true| {worst[1]:.2e}; refined |C - C_true| "
          f"{worst[2]:.2e}, RMS {worst[3]:.2e} px")
    assert worst[0] <= 1e-8 and worst[1] <= 1e-11
    assert worst[2] <= 1e-8 and worst[3] <= 1e-8


# ---- 2. noisy data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", ir.TYPES)
def test_noisy_against_the_restatement(fba, typ):
    synth, sc = _scene(typ, 0.3)
    worst = np.zeros(5)
    for e in range(12):
        X, uv, c, ydir = _image_inputs(fba, synth, sc, typ, 5, False, e)
        a = rr.resect_image(typ, X, uv, c, ydir, method="eigh")
        b = rr.resect_image(typ, X, uv, c, ydir, refine_iters=0, method="svd")
        assert a["status"] == 0 and a["rms_fin"] <= a["rms_lin"]        # the restatement alone
        sC, sM = np.abs(a["C_lin"] - b["C_lin"]).max(), np.abs(a["M_lin"] - b["M_lin"]).max()
        lin, ql, sl = fba.capi.resect_host(typ, X, uv, c, ydir, refine_iters=0)
        fin, qf, sf = fba.capi.resect_host(typ, X, uv, c, ydir)
        assert sl == 0 and sf == 0 and ql[0] == qf[0] == len(X)
        eC, eM = np.abs(lin[:3] - a["C_lin"]).max(), np.abs(ir.rot(*lin[3:]) - a["M_lin"]).max()
        assert eC <= max(1e-9 * a["dist"], 100 * sC), (e, eC, sC)
        assert eM <= max(1e-9, 100 * sM), (e, eM, sM)
        assert abs(ql[1] - a["ratio"]) <= 1e-10 and abs(qf[1] - a["ratio"]) <= 1e-10
        assert abs(ql[2] - a["rms_lin"]) <= 1e-6 and ql[3] == ql[2]
        fC, fM = np.abs(fin[:3] - a["eop"][:3]).max(), np.abs(ir.rot(*fin[3:]) - ir.rot(*a["eop"][3:])).max()
        assert fC <= 100 * 1e-10 * a["dist"], (e, fC)
        assert fM <= 100 * 1e-10, (e, fM)
        assert qf[3] <= qf[2] and abs(qf[3] - a["rms_fin"]) <= 1e-6
        worst = np.maximum(worst, [eC, eM, fC, fM, a["iters"]])
    print(f"noisy {typ}: linear |C - ref| {worst[0]:.2e}, |M - ref| {worst[1]:.2e}; refined |C - ref| {worst[2]:.2e}, "
          f"|M - ref| {worst[3]:.2e} in <= {int(worst[4])} passes; last image RMS {a['rms_lin']:.3f} -> {a['rms_fin']:.3f} px")


# ---- 3. edge cases ---------------------------------------------------------------------------------------------------
def _one_image(fba, typ="fisheye", noise=0.0):
    synth, sc = _scene(typ, noise)
    return (sc, *_image_inputs(fba, synth, sc, typ, 5, noise == 0.0, 0))


def test_few_and_exactly_six(fba):
    sc, X, uv, c, ydir = _one_image(fba)
    eop, q, st = fba.capi.resect_host("fisheye", X[:5], uv[:5], c, ydir)
    assert st == 1 and list(q) == [5, 0, 0, 0, 0] and not eop.any()
    eop, q, st = fba.capi.resect_host("fisheye", X[:0], uv[:0], c, ydir)
    assert st == 1 and list(q) == [0, 0, 0, 0, 0]
    eop, q, st = fba.capi.resect_host("fisheye", X[:6], uv[:6], c, ydir, refine_iters=0)
    assert st == 0 and q[0] == 6 and np.isfinite(eop).all()


def test_coplanar_points_are_weak(fba):
    from fba_amd import synth
    sc, X, uv, c, ydir = _one_image(fba)
    Xp = X.copy()
    Xp[:, 2] = 100.0 + 0.01 * Xp[:, 0]                                   # a tilted plane
    M = ir.rot(*sc["ang_true"][0])
    ct = np.concatenate([ir.true_iop(synth, 1, 5)[0, :3], [synth.YDIR], [0.0, 0.0], [0.0] * 5])
    xy = ir.forward("fisheye", (Xp - sc["C_true"][0]) @ M.T, ct).astype(np.float64)
    uvp, st = fba.capi.unproject_host("fisheye", xy, ct)
    eop, q, status = fba.capi.resect_host("fisheye", Xp, uvp, ct[2], ct[3])
    assert (st == 0).all() and status == 2 and q[0] == len(Xp) and q[1] <= 1e-12 and q[2] == q[3] == 0 and not eop.any()


def test_reversed_directions_give_the_same_pose(fba):
    sc, X, uv, c, ydir = _one_image(fba)
    a, qa, sa = fba.capi.resect_host("fisheye", X, uv, c, ydir)
    rev = uv.copy()
    rev[:, 2:] *= -1.0
    b, qb, sb = fba.capi.resect_host("fisheye", X, rev, c, ydir)
    assert sa in (0, 3) and sb == sa
    assert np.abs(a[:3] - b[:3]).max() <= 1e-8 and np.abs(ir.rot(*a[3:]) - ir.rot(*b[3:])).max() <= 1e-11
    assert {qa[4], qb[4]} == {0.0, 1.0}
    assert qa[4] == 0.0                                                   # synth's scenes have W < 0


def test_domain_ray_is_left_out(fba):
    sc, X, uv, c, ydir = _one_image(fba)
    st = np.zeros(len(X), dtype=np.int32)
    st[3] = 1
    bad = uv.copy()
    bad[3, 2:] = 0.0
    a, qa, sa = fba.capi.resect_host("fisheye", X, bad, c, ydir, ray_status=st)
    keep = np.arange(len(X)) != 3
    b, qb, sb = fba.capi.resect_host("fisheye", X[keep], uv[keep], c, ydir)
    assert qa[0] == len(X) - 1 and sa == sb and np.array_equal(a, b) and np.array_equal(qa, qb)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_phi_at_a_right_angle(fba, sign):
    from fba_amd import synth
    rng = np.random.default_rng(11)
    ang = np.array([0.3, sign * np.pi / 2, -0.7])
    M, Ct = ir.rot(*ang), np.array([100.0, -200.0, 50.0])
    uvw = np.stack([rng.uniform(-800, 800, 30), rng.uniform(-800, 800, 30), -rng.uniform(900, 2500, 30)], -1)
    X = uvw @ M + Ct                                                     # (U V W) = M (X - C)
    ct = np.concatenate([ir.true_iop(synth, 1, 5)[0, :3], [synth.YDIR], [0.0, 0.0], [0.0] * 5])
    xy = ir.forward("fisheye", uvw, ct).astype(np.float64)
    uv, st = fba.capi.unproject_host("fisheye", xy, ct)
    eop, q, status = fba.capi.resect_host("fisheye", X, uv, ct[2], ct[3])
    err = np.abs(ir.rot(*eop[3:]) - M).max()
    print(f"phi = {sign:+.0f} pi/2: status {status}, |rot(angles) - M| {err:.2e}, |C - C_true| {np.abs(eop[:3] - Ct).max():.2e}")
    assert (st == 0).all() and status in (0, 3) and q[0] == 30
    assert err <= 1e-6 and np.abs(eop[:3] - Ct).max() <= 1e-3 and np.isfinite(q).all()


def test_exports_and_arguments(fba):
    lib = C.CDLL(fba.capi.LIB_PATH)
    for name in ("fba_resect", "fba_resect_host"):
        assert hasattr(lib, name) and name in fba.capi.EXPORTS
    assert fba.capi.lib.fba_abi_version() == 2 and hasattr(fba.capi.Context, "resect")
    assert fba.capi.lib.fba_resect(None, None, None, None, None, None) == 1
    op = fba.capi.ResectOptions()
    assert (op.use, op.refine_iters, op.write_xhat, op.min_ratio, op.refine_tol) == (0, 10, 0, 1e-6, 1e-10)
    assert fba.capi.ResectOptions("all").use == 1
    with pytest.raises(ValueError):
        fba.capi.ResectOptions("ties")
    z = np.zeros(40)
    p = fba.capi.ptr
    assert fba.capi.lib.fba_resect_host(9, 0, None, None, None, 1.0, 1.0, 0.3, 0.3, None, None, None, None) == 2
    assert fba.capi.lib.fba_resect_host(0, -1, None, None, None, 1.0, 1.0, 0.3, 0.3, None, None, None, None) == 1
    assert fba.capi.lib.fba_resect_host(0, 2, p(z), p(z), None, 1.0, 1.0, 0.0, 0.3, None, None, None, None) == 1
    bad = fba.capi.ResectOptions()
    bad.use = 2
    assert fba.capi.lib.fba_resect_host(0, 0, None, None, None, 1.0, 1.0, 0.3, 0.3, C.byref(bad), None, None, None) == 1
    assert fba.capi.lib.fba_resect_host(0, 0, None, None, None, 1.0, 1.0, 0.3, 0.3, None, None, None, None) == 0


# ---- the .rsc table --------------------------------------------------------------------------------------------------
class _Data:
    images = ["img_a", "img_b", "img_c", "img_d"]
    EXT = [["img_a", "cam", 1.0, 2.0, 3.0, 0.0625, 0.5, 0.25], ["img_b", "cam", 10.0, 20.0, 30.0, 0.0, 0.0, 0.0],
           ["img_c", "cam", -5.0, 0.0, 5.0, -0.125, 0.0, 3.0], ["img_d", "cam", 7.0, 8.0, 9.0, 0.5, 0.25, -2.0]]


class _Res:
    resect_eop = np.array([[1.5, 2.0, 2.0, 0.125, 0.25, 0.5], [10.0, 20.0, 30.0, 0.0, 0.0, 0.0],
                           [-5.0, 0.0, 5.0, -0.125, 0.0, 3.0], [7.25, 8.0, 9.0, 0.5, 0.5, -2.0]])
    resect_quality = np.array([[30, 0.25, 1.5, 0.5, 0.0], [4, 0.0, 0.0, 0.0, 0.0], [12, 1e-9, 0.0, 0.0, 0.0],
                               [8, 0.125, 2.0, 2.0, 1.0]])
    resect_status = np.array([0, 1, 2, 3], dtype=np.int32)


def test_write_rsc(fba, tmp_path):
    """column layout (write_fwd's style: tab-delimited, no header, EXT order), the * flag and the status words"""
    from fba_amd import report
    path = os.path.join(str(tmp_path), "x.rsc")
    report.write_rsc(path, _Data, _Res)
    cells = [r.split("\t") for r in open(path).read().splitlines()]
    assert [c[0] for c in cells] == _Data.images and [c[1] for c in cells] == ["30", "4", "12", "8"]
    for c, x, row, q in zip(cells, _Res.resect_eop, _Data.EXT, _Res.resect_quality):
        assert [float(v) for v in c[2:8]] == list(x)
        assert [float(v) for v in c[8:14]] == list(x - np.array(row[2:8]))
        assert [float(v) for v in c[14:17]] == list(q[1:4])
    assert len(cells[0]) == 17
    assert [c[17:] for c in cells[1:]] == [["*", "FEW"], ["*", "WEAK"], ["*", "REFINE"]]
    names, used, eop, shift, qual, words = report.read_rsc(path)
    assert names == _Data.images and list(used) == [30, 4, 12, 8] and words == ["OK", "FEW", "WEAK", "REFINE"]
    assert np.array_equal(eop, _Res.resect_eop) and np.array_equal(qual, _Res.resect_quality[:, 1:4])
    assert np.array_equal(shift, _Res.resect_eop - np.array([r[2:8] for r in _Data.EXT]))
    with pytest.raises(ValueError):
        report.write_rsc(path, _Data, object())


# ---- 4. the stand-alone sanitizer program ----------------------------------------------------------------------------
def test_sanitizer_program(tmp_path):
    """tests/resect_check.cpp: the header routines over the edge cases and the image-list builder (an image without
    observations, an empty problem), compiled with the host compiler under AddressSanitizer and UBSan, run directly"""
    exe = os.path.join(str(tmp_path), "resect_check")
    # host code only: each sanitizer option applies to the host compilation (-Xarch_host), none to a device pass
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "resect_check.cpp"),
                    os.path.join(CSRC, "fba_api_host.cpp"), os.path.join(CSRC, "fba_plan.cpp"), os.path.join(CSRC, "fba_order.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and all(ln.startswith("ok ") for ln in lines), r.stdout + r.stderr
    assert len(lines) >= 8
