"""CPU: the host side of the point-precision outputs -- the device's symmetric 3 x 3 eigen routine run on the host
(fba_eig3_host, csrc/fba_eig3.h) against numpy.linalg.eigh, report.write_ell / read_ell and the horizontal ellipse,
the Adjustment defaults, the command line's --ellipsoids flag and the two additive exports (the blocks and ellipsoids
themselves: tests/test_gpu_point_precision.py).

Bars.  Orthonormality ||D D' - I|| and reconstruction ||D' diag(a^2) D - C|| / lambda_max (Frobenius), worst over the
seeded set: max(64 eps, 20 x what eigh's own factors leave in the same expression on that set).  Directions, up to
sign, only where the vector's relative gap min_j |lambda_i - lambda_j| / lambda_max exceeds 1e-3: the sine of the
angle to eigh's vector within 64 eps / gap (rounding: both routines are backward stable, and a perturbation of eps
lambda_max turns an eigenvector by eps / gap).
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
GAP = 1e-3


def pack6(C):
    C = np.asarray(C, dtype=np.float64)
    return np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])


def full3(b):
    return np.array([[b[0], b[1], b[2]], [b[1], b[3], b[4]], [b[2], b[4], b[5]]])


def _rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


def block_set():
    """(tag, block [6]) over every class of the module docstring; seeded"""
    rng = np.random.default_rng(20)
    out = []
    for i in range(200):
        m = rng.standard_normal((3, 3))
        out.append(("spd", pack6(m @ m.T + 1e-3 * np.eye(3))))
    for d in ([3.0, 2.0, 1.0], [1.0, 2.0, 3.0], [2.0, 3.0, 1.0], [1e-3, 5.0, 0.7]):
        out.append(("diagonal", pack6(np.diag(d))))
    for lam in ([2.0, 2.0, 1.0], [3.0, 1.0, 1.0], [1.0, 1.0, 1.0], [5.0, 5.0, 5.0]):
        out.append(("equal", pack6(np.diag(lam))))
        for _ in range(5):
            q = _rot(rng)
            c = q @ np.diag(lam) @ q.T
            out.append(("equal", pack6(0.5 * (c + c.T))))
    for _ in range(10):
        v, w = rng.standard_normal(3), rng.standard_normal(3)
        out.append(("rank1", pack6(np.outer(v, v))))
        out.append(("rank2", pack6(np.outer(v, v) + np.outer(w, w))))
    for scale in (1e-12, 1e6):
        for _ in range(10):
            m = rng.standard_normal((3, 3))
            out.append((f"scale{scale:g}", pack6(scale * (m @ m.T + 1e-3 * np.eye(3)))))
    for k in (2, 4, 6, 8):
        for _ in range(5):
            q = _rot(rng)
            c = q @ np.diag([1.0, 10.0 ** (-k / 2), 10.0 ** (-k)]) @ q.T
            out.append((f"aniso1e{k}", pack6(0.5 * (c + c.T))))
    # the smallest eigenvalue exactly -2^-55 (decoupled from the other two): semi-axis 0
    out.append(("negative", np.array([-2.0 ** -55, 0.0, 0.0, 1.0, 0.25, 0.5])))
    out.append(("zero", np.zeros(6)))
    return out


def eigh_ell(C):
    """eigh's factors in the ellipsoid's layout: a^2 (descending, clamped at 0), D (rows), the raw eigenvalues"""
    w, V = np.linalg.eigh(C)
    return np.maximum(w[::-1], 0.0), V.T[::-1], w[::-1]


def residuals(C, a2, D):
    lmax = max(np.abs(np.linalg.eigvalsh(C)).max(), np.finfo(np.float64).tiny)
    return np.linalg.norm(D @ D.T - np.eye(3)), np.linalg.norm(D.T @ np.diag(a2) @ D - C) / lmax


def check_ellipsoids(tag, blocks, ell):
    """every property of the module docstring for ell [n][12] of blocks [n][6]; prints the measured figures and
    returns them (the GPU tests run it on the device's output)"""
    worst = dict(orth=0.0, recon=0.0, orth_eigh=0.0, recon_eigh=0.0, angle=0.0, compared=0, vectors=0)
    for b, e in zip(blocks, ell):
        C = full3(b)
        a, D = e[:3], e[3:].reshape(3, 3)
        assert np.isfinite(e).all(), (b, e)
        assert a[0] >= a[1] >= a[2] >= 0.0, (b, a)
        for v in D:  # the sign convention, on every vector
            k = int(np.argmax(np.abs(v)))
            assert v[k] > 0.0, (b, v)
        o, r = residuals(C, a ** 2, D)
        a2e, De, w = eigh_ell(C)
        oe, re = residuals(C, a2e, De)
        worst["orth"], worst["recon"] = max(worst["orth"], o), max(worst["recon"], r)
        worst["orth_eigh"], worst["recon_eigh"] = max(worst["orth_eigh"], oe), max(worst["recon_eigh"], re)
        lmax = np.abs(w).max()
        for i in range(3):
            worst["vectors"] += 1
            gap = min(abs(w[i] - w[j]) for j in range(3) if j != i) / lmax if lmax > 0 else 0.0
            if gap > GAP:
                s = np.linalg.norm(np.cross(D[i], De[i]))
                worst["compared"] += 1
                worst["angle"] = max(worst["angle"], s * gap / (64 * EPS))
                assert s <= 64 * EPS / gap, (b, i, s, gap)
    bar_o, bar_r = max(64 * EPS, 20 * worst["orth_eigh"]), max(64 * EPS, 20 * worst["recon_eigh"])
    print(f"ellipsoid {tag}: n={len(blocks)} ||DD'-I|| {worst['orth']:.2e} (eigh {worst['orth_eigh']:.2e}, bar {bar_o:.2e}) "
          f"||D'diag(a^2)D-C||/lmax {worst['recon']:.2e} (eigh {worst['recon_eigh']:.2e}, bar {bar_r:.2e}) "
          f"worst angle/bar {worst['angle']:.2f} over {worst['compared']} of {worst['vectors']} vectors")
    assert worst["orth"] <= bar_o and worst["recon"] <= bar_r
    return worst


def test_eig3_host_against_eigh(fba):
    tags, blocks = zip(*block_set())
    blocks = np.array(blocks)
    ell = fba.capi.eig3_host(blocks)
    assert ell.shape == (len(blocks), 12)
    w = check_ellipsoids("host", blocks, ell)
    assert w["compared"] > 300
    # eigenvalues against eigh's: Weyl, a backward error of 64 eps lambda_max moves none further
    for b, e in zip(blocks, ell):
        a2e = eigh_ell(full3(b))[0]
        assert np.abs(e[:3] ** 2 - a2e).max() <= 64 * EPS * max(a2e[0], np.abs(b).max())
    # the slightly negative eigenvalue: semi-axis exactly 0; the zero block: zero axes, the unit vectors
    neg = ell[tags.index("negative")]
    assert neg[2] == 0.0 and neg[1] > 0.0
    np.testing.assert_array_equal(ell[tags.index("zero")], [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1])
    # equal eigenvalues on a diagonal block: no rotation, the axes are the coordinate axes
    np.testing.assert_array_equal(fba.capi.eig3_host(pack6(np.diag([1.0, 1.0, 1.0])))[0, 3:], np.eye(3).reshape(-1))


def test_eig3_host_nan_block_gives_nans(fba):
    good = pack6(np.diag([3.0, 2.0, 1.0]))
    bad = [good.copy() for _ in range(3)]
    bad[0][1] = np.nan
    bad[1][3] = np.inf
    bad[2][5] = -np.inf
    ell = fba.capi.eig3_host(np.array([good, *bad, good]))
    assert np.isnan(ell[1:4]).all()
    np.testing.assert_array_equal(ell[0], ell[4])
    np.testing.assert_allclose(ell[0][:3], np.sqrt([3.0, 2.0, 1.0]), rtol=4 * EPS)
    assert fba.capi.eig3_host(np.zeros((0, 6))).shape == (0, 12)


def test_eig3_host_is_deterministic(fba):
    blocks = np.array([b for _, b in block_set()])
    np.testing.assert_array_equal(fba.capi.eig3_host(blocks), fba.capi.eig3_host(blocks.copy()))


# ---- host plumbing ----------------------------------------------------------------------------------------------
def _adjustment(fba, **kw):
    from fba_amd.bundle import Adjustment
    base = dict(xhat=np.zeros(1), xhatnames=["x"], iterations=1, deltasum=np.zeros(1), v=np.zeros(6),
                rsd=np.zeros((3, 5)), rms=(0.0, 0.0, 0.0), sigma02=1.0, seconds=0.0)
    base.update(kw)
    return Adjustment(**base)


def test_adjustment_defaults_are_none(fba):
    res = _adjustment(fba)
    assert res.cx_tie is None and res.ell_axes is None and res.ell_dirs is None


def test_horizontal_ellipse_by_hand(fba):
    from fba_amd import report
    # [[3, 1], [1, 3]]: eigenvalues 4 and 2, the major axis along (1, 1): 45 degrees from +Y towards +X
    np.testing.assert_allclose(report.horizontal_ellipse(3.0, 1.0, 3.0), (2.0, np.sqrt(2.0), 45.0), rtol=1e-15)
    # [[3, -1], [-1, 3]]: the major axis along (-1, 1): 135 degrees
    np.testing.assert_allclose(report.horizontal_ellipse(3.0, -1.0, 3.0), (2.0, np.sqrt(2.0), 135.0), rtol=1e-15)
    # axis-aligned: major along Y is azimuth 0, along X 90; a circle has azimuth 0
    assert report.horizontal_ellipse(1.0, 0.0, 4.0) == (2.0, 1.0, 0.0)
    assert report.horizontal_ellipse(4.0, 0.0, 1.0) == (2.0, 1.0, 90.0)
    assert report.horizontal_ellipse(2.25, 0.0, 2.25) == (1.5, 1.5, 0.0)
    # [[2, sqrt(3)/2], [sqrt(3)/2, 1]]: eigenvalues 2.5 and 0.5, the major axis 30 degrees off +X: azimuth 60
    maj, mnr, az = report.horizontal_ellipse(2.0, np.sqrt(3.0) / 2, 1.0)
    np.testing.assert_allclose((maj ** 2, mnr ** 2, az), (2.5, 0.5, 60.0), rtol=1e-14)
    for sxx, sxy, syy in ((1.0, -1e-9, 1.0 + 1e-12), (5.0, -4.9, 5.0), (1.0, 1e-300, 1.0)):
        assert 0.0 <= report.horizontal_ellipse(sxx, sxy, syy)[2] < 180.0


def test_write_ell_columns_and_round_trip(fba, tmp_path):
    from fba_amd import report
    assert report.ELL_K95 == 2.7955 and abs(report.ELL_K95 ** 2 - 7.8147) < 2e-4
    # block 0: Z apart (9); in XY the eigenvalues 2.5 along (cos 30, sin 30) and 0.5 along (-sin 30, cos 30)
    h = np.sqrt(3.0) / 2
    blocks = np.array([pack6([[2.0, h, 0.0], [h, 1.0, 0.0], [0.0, 0.0, 9.0]]),
                       pack6(np.diag([4.0, 1.0, 0.25]))])
    ell = fba.capi.eig3_host(blocks)
    data = SimpleNamespace(TIE=["T7", "A"])
    res = _adjustment(fba, cx_tie=fba.capi.tie_blocks(blocks), ell_axes=ell[:, :3], ell_dirs=ell[:, 3:].reshape(-1, 3, 3))
    assert res.cx_tie.shape == (2, 3, 3)
    np.testing.assert_array_equal(res.cx_tie, np.transpose(res.cx_tie, (0, 2, 1)))
    path = str(tmp_path / "t.ell")
    report.write_ell(path, data, res)
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert [len(r) for r in rows] == [19, 19] and [r[0] for r in rows] == ["T7", "A"]
    num = np.array([[float(x) for x in r[1:]] for r in rows])
    # sigma X Y Z | a b c | the nine cosines | horizontal semi-major, semi-minor, azimuth
    np.testing.assert_allclose(num[0, :3], np.sqrt([2.0, 1.0, 9.0]), rtol=1e-14)
    np.testing.assert_allclose(num[0, 3:6], [3.0, np.sqrt(2.5), np.sqrt(0.5)], rtol=1e-14)
    np.testing.assert_allclose(num[0, 6:15], [0, 0, 1, h, 0.5, 0, -0.5, h, 0], atol=1e-15)
    np.testing.assert_allclose(num[0, 15:], [np.sqrt(2.5), np.sqrt(0.5), 60.0], rtol=1e-14)
    np.testing.assert_allclose(num[1], [2, 1, 0.5, 2, 1, 0.5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 1, 90], rtol=1e-15)
    names, sig, axes, dirs, hor = report.read_ell(path)
    assert names == ["T7", "A"] and dirs.shape == (2, 3, 3) and hor.shape == (2, 3)
    np.testing.assert_allclose(sig, num[:, :3], rtol=0)
    np.testing.assert_allclose(axes, res.ell_axes, rtol=1e-14)
    np.testing.assert_allclose(dirs, res.ell_dirs, atol=1e-15)
    # without the outputs, or with a table of another length, nothing is written
    with pytest.raises(ValueError):
        report.write_ell(path, data, _adjustment(fba))
    with pytest.raises(ValueError):
        report.write_ell(path, SimpleNamespace(TIE=["T7"]), res)
    (tmp_path / "short.ell").write_text("T7\t1\t2\n")
    with pytest.raises(ValueError):
        report.read_ell(str(tmp_path / "short.ell"))


def test_cli_parses_ellipsoids_in_any_position(fba, monkeypatch):
    from fba_amd import batch, bundle
    calls = []
    monkeypatch.setattr(bundle, "main", lambda folder, plot=False, device=0, reliability=False, ellipsoids=False:
                        calls.append((folder, bool(plot), reliability, ellipsoids)) or 0)
    for argv in (["main", "F"], ["main", "F", "--ellipsoids"], ["main", "F", "--ellipsoids", "1"],
                 ["main", "F", "1", "--ellipsoids"], ["main", "--ellipsoids", "F", "false"],
                 ["main", "F", "--reliability", "--ellipsoids"], ["--ellipsoids", "main", "F", "1", "--reliability"]):
        assert batch.cli(argv) == 0
    assert calls == [("F", False, False, False), ("F", False, False, True), ("F", True, False, True),
                     ("F", True, False, True), ("F", False, False, True), ("F", False, True, True),
                     ("F", True, True, True)]
    # without the flag the keyword is not passed at all: a main() that does not know it still works
    monkeypatch.setattr(bundle, "main", lambda folder, plot=False, device=0, reliability=False: 0)
    assert batch.cli(["main", "F", "--reliability"]) == 0
    assert batch.parse_main(["F", "--ellipsoids", "1"]) == ("F", True, False)


def test_library_exports_the_two_symbols_at_abi_2(fba):
    lib = ctypes.CDLL(fba.capi.LIB_PATH)
    assert hasattr(lib, "fba_postfit_outputs") and hasattr(lib, "fba_eig3_host")
    assert "fba_postfit_outputs" in fba.capi.EXPORTS and "fba_eig3_host" in fba.capi.HOST_EXPORTS
    assert hasattr(fba.capi.Context, "postfit")
    P, D = ctypes.c_void_p, ctypes.c_double
    assert fba.capi.lib.fba_postfit_outputs.argtypes == [P, D, P]
    assert fba.capi.lib.fba_eig3_host.argtypes == [ctypes.c_int64, P, P]
    assert [n for n, _ in fba.capi.Postfit._fields_] == ["cx_diag", "corr", "redundancy", "wstat", "cx_tie", "ellipsoid"]
    assert ctypes.sizeof(fba.capi.Postfit) == 6 * ctypes.sizeof(P)
    assert fba.capi.lib.fba_abi_version() == 2
    # NULL arguments are argument errors before anything touches the GPU
    out = fba.capi.Postfit()
    assert fba.capi.lib.fba_postfit_outputs(None, 1.0, ctypes.byref(out)) == 1
    assert fba.capi.lib.fba_postfit_outputs(None, 1.0, None) == 1
    assert fba.capi.lib.fba_eig3_host(1, None, None) == 1 and fba.capi.lib.fba_eig3_host(0, None, None) == 0
