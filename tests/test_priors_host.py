"""CPU: the host side of prior observations of unknowns -- the two additive exports at ABI 2, fba_create_priors'
argument checks (made on the host before any GPU call, so they run here), the .pri table, report.write_prr /
read_prr, the command line's --priors option and the Adjustment defaults (the numbers: tests/test_gpu_priors.py)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import CAM0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fba_create_priors", "fba_get_priors")


def test_exports_and_abi(fba):
    """the header, capi.EXPORTS and capi.Context agree"""
    header = open(os.path.join(ROOT, "include", "fba.h")).read()
    declared = set(re.findall(r"\b(fba_[a-z_]+)\s*\(", header))
    assert declared == set(fba.capi.EXPORTS) and set(NEW) <= declared
    lib = C.CDLL(fba.capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert fba.capi.lib.fba_abi_version() == 2 and "#define FBA_ABI_VERSION 2" in header
    assert re.search(r"typedef struct fba_priors \{\s*int64_t n;[^}]*const int64_t\* index;[^}]*const double\* value;"
                     r"[^}]*const double\* sigma;[^}]*\} fba_priors;", header)
    assert [f[0] for f in fba.capi.Priors._fields_] == ["n", "index", "value", "sigma"]
    assert hasattr(fba.capi.Context, "get_priors")
    import inspect
    assert "priors" in inspect.signature(fba.capi.Context.__init__).parameters


def _create(fba, ds, index, value, sigma, world=1, split=0):
    pk, st = ds.pack(), fba.capi.make_settings(ds.settings)
    index, value, sigma = np.asarray(index, np.int64), np.asarray(value, np.float64), np.asarray(sigma, np.float64)
    pr = fba.capi.Priors(len(index), fba.capi.ptr(index).value, fba.capi.ptr(value).value, fba.capi.ptr(sigma).value)
    opts = fba.capi.Options(0, 0, world, 0, None, split)
    h = C.c_void_p()
    rc = fba.capi.lib.fba_create_priors(C.byref(pk.struct), C.byref(st), C.byref(opts), C.byref(pr), C.byref(h))
    assert rc != 0 and not h.value  # (every call of this module is refused before a context exists)
    return rc, fba.capi.last_error()


def test_argument_errors_before_the_gpu(fba):
    """FBA_ERR_ARG with a message naming the entry, from the host checks (this test runs without a GPU): an index
    outside [0, u), an index given twice, a non-finite value, a sigma that is not finite or not > 0; a split request
    with priors is FBA_ERR_UNSUPPORTED; fba_get_priors on a NULL context"""
    ds = fba.load_folder(CAM0)
    u = fba.capi.count_unknowns(ds.pack(), fba.capi.make_settings(ds.settings))
    ok = ([0, 5, u - 1], [1.0, 2.0, 3.0], [1.0, 1.0, 1.0])
    for bad in (-1, u, u + 7):
        rc, msg = _create(fba, ds, [0, bad, 2], ok[1], ok[2])
        assert rc == 1 and "index[1]" in msg and "outside" in msg
    rc, msg = _create(fba, ds, [4, 9, 4], ok[1], ok[2])
    assert rc == 1 and "duplicate index 4" in msg
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc, msg = _create(fba, ds, ok[0], [1.0, bad, 3.0], ok[2])
        assert rc == 1 and "value[1]" in msg and "finite" in msg
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        rc, msg = _create(fba, ds, ok[0], ok[1], [1.0, 1.0, bad])
        assert rc == 1 and "sigma[2]" in msg and "finite and > 0" in msg
    rc, msg = _create(fba, ds, *ok, world=2, split=1)
    assert rc == 5 and "subtree split" in msg  # FBA_ERR_UNSUPPORTED
    assert fba.capi.lib.fba_get_priors(None, None, None, None) == 1 and "fba_get_priors" in fba.capi.last_error()
    with pytest.raises(ValueError):
        fba.capi.pack_priors(([0, 1], [1.0], [1.0, 1.0]))
    assert fba.capi.pack_priors(None) == (None, None)
    assert fba.capi.pack_priors((np.zeros(0, np.int64), np.zeros(0), np.zeros(0))) == (None, None)


def _cam0_with_pri(tmp_path, fba, text, name="cam0.pri"):
    import shutil
    dst = str(tmp_path / "cam0")
    if not os.path.isdir(dst):
        shutil.copytree(CAM0, dst)
    for f in os.listdir(dst):
        if f.endswith(".pri"):
            os.remove(os.path.join(dst, f))
    if text is not None:
        with open(os.path.join(dst, name), "w") as fh:
            fh.write(text)
    return fba.load_folder(dst)


def test_pri_table(fba, tmp_path):
    """names as xhat_names gives them, w / p / k in degrees, comments and blank lines as in the other tables; a
    name that is not an estimated unknown, a duplicate and a std <= 0 are IngestErrors -- raised by the request for
    the priors, not by loading the folder"""
    from fba_amd.bundle import _priors_of
    from fba_amd.io import IngestError
    plain = _cam0_with_pri(tmp_path, fba, None)
    assert plain.priors is None and plain.priors_error == ""
    names = fba.xhat_names(plain)
    img, cam = plain.EXT[1][0], plain.EXT[1][1]
    cid = plain.INT[0][0]
    tgt = plain.TIE[2]
    rows = [(f"Xc_{img}_{cam}", 12.5, 0.05), (f"k_{img}_{cam}", 90.0, 0.5), (f"w_{img}_{cam}", -45.0, 1.0),
            (f"k2_{cid}", 1e-9, 2e-10), (f"c_{cid}", 3000.0, 1.5), (f"Z_{tgt}", 7.0, 0.01)]
    text = "# name value std\n\n" + "".join(f"{n}\t{v!r}  {s!r}\n" for n, v, s in rows)
    ds = _cam0_with_pri(tmp_path, fba, text)
    idx, val, sig = ds.priors
    assert [names[i] for i in idx] == [r[0] for r in rows] and idx.dtype == np.int64
    rad = np.pi / 180
    np.testing.assert_array_equal(val, [12.5, 90.0 * rad, -45.0 * rad, 1e-9, 3000.0, 7.0])
    np.testing.assert_array_equal(sig, [0.05, 0.5 * rad, 1.0 * rad, 2e-10, 1.5, 0.01])
    assert _priors_of(ds, True) is ds.priors and _priors_of(ds, None) is None and _priors_of(ds, False) is None
    assert _priors_of(ds, (idx, val, sig))[0] is idx
    for bad, what in ((f"Xc_{img}_nocam 1 1\n", "not an estimated unknown"), ("xp 1 1\n", "not an estimated unknown"),
                      (f"c_{cid} 1 1\nc_{cid} 2 1\n", "given twice"), (f"c_{cid} 1 0\n", "> 0"),
                      (f"c_{cid} 1 -1\n", "> 0"), (f"c_{cid} x 1\n", "finite"), (f"c_{cid} 1\n", "expected")):
        ds = _cam0_with_pri(tmp_path, fba, bad)  # loading is not touched by the bad table
        assert ds.priors is None and what in ds.priors_error
        with pytest.raises(IngestError, match=what):
            _priors_of(ds, True)
    with pytest.raises(IngestError, match="no .pri file"):
        _priors_of(plain, True)
    # an unknown the .cfg does not estimate is not in xhat_names: no prior on it
    ds = _cam0_with_pri(tmp_path, fba, f"c_{cid} 1 1\n")
    ds.settings["Estimate_c"] = 0
    from fba_amd.io import read_pri
    with pytest.raises(IngestError, match="not an estimated unknown"):
        read_pri(os.path.join(ds.folder, "cam0.pri"), ds)


def _adjustment(fba, **kw):
    from fba_amd.bundle import Adjustment
    base = dict(xhat=np.zeros(1), xhatnames=["x"], iterations=1, deltasum=np.zeros(1), v=np.zeros(6),
                rsd=np.zeros((3, 5)), rms=(0.0, 0.0, 0.0), sigma02=1.0, seconds=0.0)
    base.update(kw)
    return Adjustment(**base)


def test_prr_round_trip_and_statistics(fba, tmp_path):
    from fba_amd import report
    from fba_amd.bundle import prior_statistics
    a = _adjustment(fba)
    assert all(getattr(a, f) is None for f in ("prior_index", "prior_value", "prior_sigma", "prior_v", "prior_r", "prior_w"))
    deg = 180 / np.pi
    names = ["Xc_1_a", "w_1_a", "k_1_a", "k2_a", "X_T"]
    xhat = np.array([10.0, 0.5, -1.25, 3e-9, 7.0])
    idx = np.array([3, 0, 2, 1])
    val, sig = np.array([2e-9, 9.0, -1.0, 0.25]), np.array([1e-9, 2.0, 0.5, 0.125])
    v = xhat[idx] - val
    cxd = np.array([1.0, 0.01, 0.2, 0.5e-18, 1.0]) * 2.0  # sigma02 = 2
    r, w = prior_statistics(2.0, cxd, idx, sig, v)
    np.testing.assert_allclose(r, 1 - np.array([0.5, 0.25, 0.8, 0.64]), rtol=1e-15)
    np.testing.assert_allclose(w, v / (sig * np.sqrt(r)), rtol=1e-15)
    r0, w0 = prior_statistics(2.0, np.full(5, 2.0 * 4.0), np.array([1]), np.array([2.0]), np.array([1.0]))
    assert r0[0] == 0.0 and w0[0] == 0.0  # an uncheckable prior: w = 0, fba_reliability's convention
    res = _adjustment(fba, xhat=xhat, xhatnames=names, prior_index=idx, prior_value=val, prior_sigma=sig, prior_v=v,
                      prior_r=r, prior_w=np.array([1.0, 3.29, -3.3, 0.0]))
    path = str(tmp_path / "t.prr")
    report.write_prr(path, None, res)
    nm, tab, flag = report.read_prr(path)
    assert nm == [names[i] for i in idx] and flag.tolist() == [False, False, True, False]  # |w| > 3.29 only
    want = np.column_stack([val, sig, xhat[idx], v, r, res.prior_w])
    want[2:4, :4] *= deg  # the k_ and w_ rows in degrees; k2_ is a distortion term, not an angle
    np.testing.assert_allclose(tab, want, rtol=1e-14)
    report.write_prr(path, None, _adjustment(fba, xhat=xhat, xhatnames=names, prior_index=idx, prior_value=val,
                                             prior_sigma=sig, prior_v=v))
    assert np.isnan(report.read_prr(path)[1][:, 4:]).all()  # no covariance: r and w empty
    with pytest.raises(ValueError):
        report.write_prr(path, None, _adjustment(fba))


def test_outputs_without_priors_are_unchanged(fba, tmp_path, monkeypatch):
    """write_outputs writes .prr exactly when the adjustment carries priors; the .out's summary takes the prior count
    only then (the same Adjustment without priors gives the file it gave before, byte for byte)"""
    from fba_amd import bundle, report
    ds = fba.load_folder(CAM0)
    n, u = ds.n, fba.capi.count_unknowns(ds.pack(), fba.capi.make_settings(ds.settings))
    mu = 6 + 3 + int(ds.settings["Num_Radial_Distortions"]) + 2
    base = dict(xhat=np.linspace(1.0, 2.0, u), xhatnames=fba.xhat_names(ds), rsd=np.zeros((ds.n_pts, 5)),
                cx_diag=np.full(u, 0.25), corr=np.tile(np.eye(mu), (ds.numImg, 1, 1)), seconds=1.25)
    outs = {}
    for tag, kw in (("plain", {}), ("priors", dict(prior_index=np.array([0, 7]), prior_value=np.zeros(2),
                                                     prior_sigma=np.ones(2), prior_v=np.ones(2)))):
        d = tmp_path / tag
        d.mkdir()
        bundle.write_outputs(ds, _adjustment(fba, **base, **kw), str(d))
        outs[tag] = {f: (d / f).read_text() for f in sorted(os.listdir(d))}
    stem = os.path.splitext(ds.settings["Output_Filename"])[0]
    assert set(outs["priors"]) - set(outs["plain"]) == {stem + ".prr"}
    out_plain, out_pri = outs["plain"][ds.settings["Output_Filename"]], outs["priors"][ds.settings["Output_Filename"]]
    ic = int(ds.settings["Inner_Constraints"])
    assert "prior" not in out_plain and re.search(rf"Total Degrees of Freedom \.+ {n + 7 * ic - u}\n", out_plain)
    assert re.search(r"Number of prior observations \.+ 2\n", out_pri)
    assert re.search(rf"Total Number of Observations \.+ {n + 7 * ic + 2}\n", out_pri)
    assert re.search(rf"Total Degrees of Freedom \.+ {n + 7 * ic + 2 - u}\n", out_pri)
    # without priors write_out is the function it was: the prior rows removed, the two files are the same
    strip = [ln for ln in out_pri.splitlines() if "prior observations" not in ln]
    same = [a == b or "Total" in a for a, b in zip(strip, out_plain.splitlines())]
    assert len(strip) == len(out_plain.splitlines()) and all(same)
    for f in outs["plain"]:
        if f != ds.settings["Output_Filename"]:
            assert outs["priors"][f] == outs["plain"][f], f


def test_cli_parses_priors(fba, monkeypatch):
    from fba_amd import batch, bundle
    assert batch.parse_priors(["main", "F"]) == (["main", "F"], False)
    assert batch.parse_priors(["main", "--priors", "F", "1"]) == (["main", "F", "1"], True)
    # parse_main still gives its three values with --priors present
    assert batch.parse_main(["F", "--priors"]) == ("F", False, False)
    assert batch.parse_main(["F", "--robust", "huber", "1", "--priors", "--reliability"]) == ("F", True, True)
    calls = []
    monkeypatch.setattr(bundle, "main", lambda folder, plot=False, device=0, reliability=False, **kw:
                        calls.append((folder, bool(plot), reliability, kw)) or 0)
    assert batch.cli(["main", "F"]) == 0
    assert batch.cli(["main", "F", "--priors"]) == 0
    assert batch.cli(["main", "F", "1", "--priors", "--reliability", "--robust", "cauchy:3"]) == 0
    assert calls == [("F", False, False, {}), ("F", False, False, {"priors": True}),
                     ("F", True, True, {"robust": "cauchy", "robust_k": 3.0, "priors": True})]
    calls.clear()
    monkeypatch.setattr(batch, "find_folders", lambda p, *a, **k: [p])
    assert batch.cli(["batch", "A", "--priors", "B"]) == 0
    assert calls == [("A", False, False, {"priors": True}), ("B", False, False, {"priors": True})]
    calls.clear()
    assert batch.cli(["batch", "A"]) == 0 and calls == [("A", False, False, {})]
    assert "--priors" in batch.USAGE


def test_main_with_priors_needs_the_table(fba, tmp_path, capsys):
    """--priors without a .pri file: main returns 1 (the request fails before a context is created)"""
    from fba_amd import bundle
    ds = _cam0_with_pri(tmp_path, fba, None)
    assert bundle.main(ds.folder, False, priors=True) == 1
    assert "no .pri file" in capsys.readouterr().out
    ds = _cam0_with_pri(tmp_path, fba, "nothing 1 1\n")
    assert bundle.main(ds.folder, False, priors=True) == 1
    assert "not an estimated unknown" in capsys.readouterr().out
