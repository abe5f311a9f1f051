"""CPU: the host side of the reliability outputs -- report.write_rel, the Adjustment defaults, the command
line's --reliability flag and the additive fba_reliability export (the numbers themselves:
tests/test_gpu_reliability.py)."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest


def _adjustment(fba, **kw):
    from fba_amd.bundle import Adjustment
    base = dict(xhat=np.zeros(1), xhatnames=["x"], iterations=1, deltasum=np.zeros(1), v=np.zeros(6),
                rsd=np.zeros((3, 5)), rms=(0.0, 0.0, 0.0), sigma02=1.0, seconds=0.0)
    base.update(kw)
    return Adjustment(**base)


def test_adjustment_defaults_are_none(fba):
    res = _adjustment(fba)
    assert res.redundancy is None and res.wstat is None and res.cx_diag is None and res.corr is None


def test_write_rel_columns_flag_and_inf(fba, tmp_path):
    from fba_amd import report
    assert (report.MDB_DELTA0, report.W_CRITICAL) == (4.13, 3.29)
    data = SimpleNamespace(n_pts=3, pho_target=["T1", "T2", "T3"], pho_image=["10", "10", "11"],
                           settings={"Meas_std": 0.5, "Meas_std_y": 0.25})
    res = _adjustment(fba, redundancy=np.array([0.25, 0.64, 0.5, 0.5, 1e-11, 0.04]),
                      wstat=np.array([1.0, -3.28, 0.5, -3.3, 0.0, 2.0]))
    path = str(tmp_path / "t.rel")
    report.write_rel(path, data, res)
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert [len(r) for r in rows] == [9, 9, 9]
    assert [r[:2] for r in rows] == [["T1", "10"], ["T2", "10"], ["T3", "11"]]
    num = [[float(x) for x in r[2:8]] for r in rows]
    # r_x r_y w_x w_y as given; mdb = 4.13 sigma / sqrt(r) with sigma_x = 0.5, sigma_y = 0.25
    np.testing.assert_allclose(num[0], [0.25, 0.64, 1.0, -3.28, 4.13 * 0.5 / 0.5, 4.13 * 0.25 / 0.8], rtol=1e-14)
    np.testing.assert_allclose(num[1][:4], [0.5, 0.5, 0.5, -3.3], rtol=1e-14)
    # |w| = 3.28 is below the critical value, 3.3 above it (either component flags the row)
    assert [r[8] for r in rows] == ["", "*", ""]
    # r < 1e-10: the observation cannot be checked, its mdb prints inf; the other component is unaffected
    assert rows[2][6] == "inf" and math.isinf(num[2][4])
    assert num[2][5] == 4.13 * 0.25 / 0.2
    # an adjustment without the reliability outputs is refused, not written as an empty table
    with pytest.raises(ValueError):
        report.write_rel(path, data, _adjustment(fba))


def test_cli_parses_reliability_in_any_position(fba, monkeypatch):
    from fba_amd import batch, bundle
    calls = []
    monkeypatch.setattr(bundle, "main", lambda folder, plot=False, device=0, reliability=False:
                        calls.append((folder, bool(plot), reliability)) or 0)
    for argv in (["main", "F"], ["main", "F", "1"], ["main", "F", "0"], ["main", "F", "--reliability"],
                 ["main", "F", "--reliability", "1"], ["main", "F", "1", "--reliability"],
                 ["main", "F", "false", "--reliability"]):
        assert batch.cli(argv) == 0
    assert calls == [("F", False, False), ("F", True, False), ("F", False, False), ("F", False, True),
                     ("F", True, True), ("F", True, True), ("F", False, True)]


def test_library_exports_fba_reliability_at_abi_2(fba):
    lib = ctypes.CDLL(fba.capi.LIB_PATH)
    assert hasattr(lib, "fba_reliability")
    assert "fba_reliability" in fba.capi.EXPORTS and hasattr(fba.capi.Context, "reliability")
    assert fba.capi.lib.fba_abi_version() == 2
    # a NULL context is an argument error before anything touches the GPU
    assert fba.capi.lib.fba_reliability(None, 1.0, None, None, None, None) == 1


def test_rel_file_beside_unchanged_outputs(fba, oracle, tmp_path):
    """write_outputs on cam0 (numbers from the dense oracle, as tests/test_report.py): with redundancy / wstat set
    the .rel table appears and .out / .par / .rsd are byte-identical to the run without them"""
    import dataclasses
    import os
    from conftest import CAM0
    from fba_amd.bundle import Adjustment
    ds = fba.load_folder(CAM0)
    od = oracle.load_folder(CAM0)
    ro = oracle.adjust(od)
    cxd, corr = oracle.covariance(od, ro)
    u_img, u_cam = oracle.counts(od.settings)
    blocks = []
    for e in range(od.numImg):
        k = int(od.cam_num[np.nonzero(od.ext_index == e)[0][0]])
        idx = list(range(e * u_img, (e + 1) * u_img)) + \
            list(range(u_img * od.numImg + k * u_cam, u_img * od.numImg + (k + 1) * u_cam))
        blocks.append(corr[np.ix_(idx, idx)])
    plain = Adjustment(xhat=ro.xhat, xhatnames=ro.names, iterations=ro.iterations, deltasum=np.array(ro.deltasum),
                       v=ro.v, rsd=ro.rsd, rms=ro.rms, sigma02=ro.sigma02, seconds=1.25, cx_diag=cxd,
                       corr=np.array(blocks))
    P = oracle.weights(od)
    _, Cx = oracle.solve_dense(od, ro.A, ro.w, ro.G, P)
    r = 1.0 - P * np.einsum("ij,ij->i", ro.A @ Cx, ro.A)
    with_rel = dataclasses.replace(plain, redundancy=r, wstat=ro.v / np.sqrt(r / P))
    files = {}
    for tag, res in (("plain", plain), ("rel", with_rel)):
        out = tmp_path / tag
        out.mkdir()
        fba.bundle.write_outputs(ds, res, str(out))
        files[tag] = {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}
    stem = os.path.splitext(ds.settings["Output_Filename"])[0]
    assert set(files["rel"]) - set(files["plain"]) == {stem + ".rel"}
    date = lambda b: [ln for ln in b.splitlines() if b"Date" not in ln and b"date" not in ln]  # noqa: E731
    for f, b in files["plain"].items():
        assert date(files["rel"][f]) == date(b), f
    rows = files["rel"][stem + ".rel"].decode().splitlines()
    assert len(rows) == ds.n_pts and all(len(ln.split("\t")) == 9 for ln in rows)
