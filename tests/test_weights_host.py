"""CPU: the host side of per-observation weights and the robust loss -- the three additive exports at ABI 2, the
argument checks that need no context, report.write_wgt / read_wgt, the command line's --robust option and the
Adjustment default (the numbers, and the per-entry checks of fba_set_weights, which need a context to know the
length of the array: tests/test_gpu_weights.py)."""
import ctypes
import re
import os
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fba_set_weights", "fba_set_loss", "fba_get_weights")


def test_exports_and_abi(fba):
    header = open(os.path.join(ROOT, "include", "fba.h")).read()
    declared = set(re.findall(r"\b(fba_[a-z_]+)\s*\(", header))
    assert declared == set(fba.capi.EXPORTS) and set(NEW) <= declared
    lib = ctypes.CDLL(fba.capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert fba.capi.lib.fba_abi_version() == 2 and "#define FBA_ABI_VERSION 2" in header
    for m in ("set_weights", "set_loss", "get_weights"):
        assert hasattr(fba.capi.Context, m)
    # every new entry point carries the "no reference counterpart" note
    for name in NEW:
        assert re.search(name + r" \(no reference counterpart\)", header), name
    assert re.search(r"FBA_LOSS_NONE = 0, FBA_LOSS_HUBER = 1, FBA_LOSS_CAUCHY = 2", header)
    assert fba.capi.LOSSES == ("none", "huber", "cauchy") and fba.capi.LOSS_K == {"huber": 1.345, "cauchy": 2.385}


def test_argument_errors_before_the_gpu(fba):
    """FBA_ERR_ARG with a message, nothing touched: a NULL context; an unknown loss or a k that is 0, negative, NaN
    or Inf (checked before the context is looked at)"""
    lib, err = fba.capi.lib, fba.capi.last_error
    w = np.ones(4)
    assert lib.fba_set_weights(None, fba.capi.ptr(w)) == 1 and "fba_set_weights" in err()
    assert lib.fba_get_weights(None, fba.capi.ptr(w)) == 1 and "fba_get_weights" in err()
    assert lib.fba_set_loss(None, 0, 0.0) == 1 and "NULL context" in err()
    for loss in (-1, 3, 99):
        assert lib.fba_set_loss(None, loss, 1.0) == 1 and "unknown loss" in err()
    for loss in (1, 2):
        for k in (0.0, -1.345, float("nan"), float("inf")):
            assert lib.fba_set_loss(None, loss, k) == 1 and "must be finite and > 0" in err()
        assert lib.fba_set_loss(None, loss, 1.0) == 1 and "NULL context" in err()  # the arguments themselves pass
    # FBA_LOSS_NONE ignores k
    assert lib.fba_set_loss(None, 0, float("nan")) == 1 and "NULL context" in err()


def _adjustment(fba, **kw):
    from fba_amd.bundle import Adjustment
    base = dict(xhat=np.zeros(1), xhatnames=["x"], iterations=1, deltasum=np.zeros(1), v=np.zeros(6),
                rsd=np.zeros((3, 5)), rms=(0.0, 0.0, 0.0), sigma02=1.0, seconds=0.0)
    base.update(kw)
    return Adjustment(**base)


def test_wgt_round_trip(fba, tmp_path):
    from fba_amd import report
    assert report.WGT_FLAG == 0.5
    assert _adjustment(fba).weights is None
    data = SimpleNamespace(n_pts=3, pho_target=["T1", "T2", "T3"], pho_image=["10", "10", "11"])
    w = np.array([1.0, 1.0, 0.5, 0.49999999999999994, 1e-12, 1234.5678901234567])
    path = str(tmp_path / "t.wgt")
    report.write_wgt(path, data, _adjustment(fba, weights=w))
    lines = open(path).read().splitlines()
    assert [len(ln.split("\t")) for ln in lines] == [6, 6, 6]
    assert lines[0].split("\t") == ["1", "T1", "10", "1", "1", ""]
    rows, tgt, img, back, flag = report.read_wgt(path)
    assert rows == [1, 2, 3] and tgt == data.pho_target and img == data.pho_image
    np.testing.assert_allclose(back.reshape(-1), w, rtol=1e-14)  # 15 significant digits, as the .rsd / .rel tables
    # 0.5 itself is not flagged, the next double below it is; either component flags the row
    assert flag.tolist() == [False, True, True]
    with pytest.raises(ValueError):
        report.write_wgt(path, data, _adjustment(fba))
    with pytest.raises(ValueError):
        report.write_wgt(path, data, _adjustment(fba, weights=np.ones(4)))


def test_write_outputs_adds_only_the_wgt_file(fba, tmp_path, monkeypatch):
    """write_outputs writes .wgt exactly when the adjustment carries weights (the other writers stubbed)"""
    from fba_amd import bundle, report
    for name in ("write_out", "write_rsd", "write_par", "write_rel"):
        monkeypatch.setattr(report, name, lambda *a, **k: [])
    data = SimpleNamespace(n_pts=3, pho_target=["T1", "T2", "T3"], pho_image=["10", "10", "11"],
                           settings={"Output_Filename": "run.out"})
    bundle.write_outputs(data, _adjustment(fba), str(tmp_path))
    assert os.listdir(tmp_path) == []
    bundle.write_outputs(data, _adjustment(fba, weights=np.ones(6)), str(tmp_path))
    assert os.listdir(tmp_path) == ["run.wgt"]


def test_cli_parses_robust(fba, monkeypatch, capsys):
    from fba_amd import batch, bundle
    assert batch.parse_robust(["main", "F"]) == (["main", "F"], None, None)
    assert batch.parse_robust(["main", "F", "--robust", "huber"]) == (["main", "F"], "huber", None)
    assert batch.parse_robust(["--robust", "Cauchy:3.5", "main", "F", "1"]) == (["main", "F", "1"], "cauchy", 3.5)
    assert batch.parse_robust(["main", "F", "--robust=huber:2", "--reliability"]) == (["main", "F", "--reliability"], "huber", 2.0)
    for bad in (["--robust"], ["--robust", "tukey"], ["--robust", "huber:0"], ["--robust", "huber:-1"],
                ["--robust", "huber:x"], ["--robust", "cauchy:inf"], ["--robust", "cauchy:nan"]):
        with pytest.raises(ValueError):
            batch.parse_robust(["main", "F"] + bad)
    # parse_main still gives its three values, whatever --robust says
    assert batch.parse_main(["F", "--robust", "huber", "1", "--reliability"]) == ("F", True, True)
    calls = []
    monkeypatch.setattr(bundle, "main", lambda folder, plot=False, device=0, reliability=False, **kw:
                        calls.append((folder, bool(plot), reliability, kw)) or 0)
    assert batch.cli(["main", "F"]) == 0
    assert batch.cli(["main", "F", "--robust", "huber"]) == 0
    assert batch.cli(["main", "F", "1", "--reliability", "--robust", "cauchy:3"]) == 0
    assert calls == [("F", False, False, {}), ("F", False, False, {"robust": "huber", "robust_k": None}),
                     ("F", True, True, {"robust": "cauchy", "robust_k": 3.0})]
    assert batch.cli(["main", "F", "--robust", "tukey"]) == 2
    out = capsys.readouterr().out
    assert "1.345" in out and "2.385" in out  # the help text states the default constants
    # batch passes the option to every folder's main
    calls.clear()
    monkeypatch.setattr(batch, "find_folders", lambda p, *a, **k: [p])
    assert batch.cli(["batch", "A", "B", "--robust", "huber:1.5"]) == 0
    assert calls == [("A", False, False, {"robust": "huber", "robust_k": 1.5}),
                     ("B", False, False, {"robust": "huber", "robust_k": 1.5})]
    calls.clear()
    assert batch.cli(["batch", "A"]) == 0 and calls == [("A", False, False, {})]


def test_context_wrappers_validate_on_the_host(fba):
    """capi.Context.set_loss's names and default constants, set_weights' length check (no context: the methods are
    called on a stand-in that records what would reach the library)"""
    seen = []
    fake = SimpleNamespace(h=None, packed=SimpleNamespace(n_pts=2))
    monkey = SimpleNamespace(fba_set_loss=lambda h, loss, k: seen.append((loss, k)) or 0,
                             fba_set_weights=lambda h, w: seen.append(w) or 0)
    orig = fba.capi.lib
    fba.capi.lib = monkey
    try:
        fba.capi.Context.set_loss(fake, "huber")
        fba.capi.Context.set_loss(fake, "Cauchy")
        fba.capi.Context.set_loss(fake, "cauchy", 3.0)
        fba.capi.Context.set_loss(fake, "none")
        fba.capi.Context.set_loss(fake, 1)
        assert seen == [(1, 1.345), (2, 2.385), (2, 3.0), (0, 0.0), (1, 1.345)]
        with pytest.raises(ValueError):
            fba.capi.Context.set_loss(fake, "tukey")
        with pytest.raises(ValueError):
            fba.capi.Context.set_weights(fake, np.ones(3))
        seen.clear()
        fba.capi.Context.set_weights(fake, None)
        assert seen == [None]
    finally:
        fba.capi.lib = orig
