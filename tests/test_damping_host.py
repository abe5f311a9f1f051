"""CPU: the host side of Levenberg-Marquardt damping -- the three additive exports and fba_lm_options at ABI 2, the
NULL-context argument errors, bundle.adjust's method= keyword, the command line's --lm option and report.write_lm's
table (the numbers: tests/test_gpu_damping.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fba_set_damping", "fba_cost", "fba_adjust_lm")


def test_exports_and_abi(fba):
    """the header, capi.EXPORTS and capi.Context agree; the ABI version stays 2"""
    header = open(os.path.join(ROOT, "include", "fba.h")).read()
    declared = set(re.findall(r"\b(fba_[a-z_]+)\s*\(", header))
    assert declared == set(fba.capi.EXPORTS) and set(NEW) <= declared
    lib = C.CDLL(fba.capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert fba.capi.lib.fba_abi_version() == 2 and "#define FBA_ABI_VERSION 2" in header
    assert re.search(r"typedef struct fba_lm_options \{\s*double lambda0, up, down, lambda_min, lambda_max, ftol;\s*\} "
                     r"fba_lm_options;", header)
    assert re.search(r"int fba_set_damping\(fba_ctx\* ctx, double lambda\);", header)
    assert re.search(r"int fba_cost\(fba_ctx\* ctx, double\* cost", header)
    assert re.search(r"int fba_adjust_lm\(fba_ctx\* ctx, const fba_lm_options\* o,\s*int32_t\* trials, int32_t\* polish,"
                     r"\s*double\* hist", header)
    names = ["lambda0", "up", "down", "lambda_min", "lambda_max", "ftol"]
    assert [f[0] for f in fba.capi.LMOptions._fields_] == names
    o = fba.capi.LMOptions()
    assert [getattr(o, n) for n in names] == [1e-3, 10.0, 10.0, 1e-12, 1e8, 1e-9]  # the header's NULL defaults
    assert C.sizeof(fba.capi.LMOptions) == 48
    for m in ("set_damping", "cost", "adjust_lm"):
        assert hasattr(fba.capi.Context, m)
    assert "options" in inspect.signature(fba.capi.Context.adjust_lm).parameters


def test_null_context_is_an_argument_error(fba):
    """FBA_ERR_ARG with a message, before anything touches a GPU"""
    lib = fba.capi.lib
    out = np.zeros(3)
    assert lib.fba_set_damping(None, 1.0) == 1 and "fba_set_damping" in fba.capi.last_error()
    assert lib.fba_cost(None, fba.capi.ptr(out)) == 1 and "fba_cost" in fba.capi.last_error()
    assert lib.fba_adjust_lm(None, None, None, None, None) == 1 and "fba_adjust_lm" in fba.capi.last_error()


def test_python_keywords(fba):
    """bundle.adjust(method=, lm_options=), main(method=), Adjustment.lm_history (default None), batch_run(lm=)"""
    from fba_amd import batch, bundle
    p = inspect.signature(bundle.adjust).parameters
    assert "method" in p and p["method"].default == "gn" and p["lm_options"].default is None
    assert inspect.signature(bundle.main).parameters["method"].default == "gn"
    assert bundle.Adjustment.__dataclass_fields__["lm_history"].default is None
    assert inspect.signature(batch.batch_run).parameters["lm"].default is None
    with pytest.raises(ValueError):
        bundle.adjust(None, method="newton")


def test_command_line_option(fba):
    """--lm and --lm=lambda0 anywhere; main()'s keywords only when the option is given"""
    from fba_amd import batch
    assert batch.parse_lm(["main", "F"]) == (["main", "F"], None)
    assert batch.parse_lm(["main", "--lm", "F"]) == (["main", "F"], True)
    assert batch.parse_lm(["main", "F", "--lm=0.5", "--reliability"]) == (["main", "F", "--reliability"], 0.5)
    for bad in ("--lm=0", "--lm=-1", "--lm=inf", "--lm=nan", "--lm=x"):
        with pytest.raises(ValueError):
            batch.parse_lm([bad])
    assert batch._lm_kw(None) == {} and batch._lm_kw(True) == {"method": "lm", "lm_options": None}
    assert batch._lm_kw(0.5) == {"method": "lm", "lm_options": {"lambda0": 0.5}}
    # parse_main still gives its three values with --lm present
    assert batch.parse_main(["F", "--lm"]) == ("F", False, False)
    assert batch.parse_main(["F", "--lm=2", "1", "--reliability"]) == ("F", True, True)
    assert "--lm" in batch.USAGE and batch.cli(["main", "F", "--lm=0"]) == 2
    o = fba.capi.LMOptions(**batch._lm_kw(0.5)["lm_options"])
    assert o.lambda0 == 0.5 and o.up == 10.0 and o.ftol == 1e-9


def test_write_lm_table(fba, tmp_path):
    """one tab-separated row per trial and polish pass: number, lambda, cost, deltasum, accepted"""
    from fba_amd import report
    hist = np.array([[1e-3, 2500.125, 310.5, 1.0], [1e-4, 2600.0, 12.25, 0.0], [1e-3, 914.4266, 0.5, 1.0],
                     [0.0, 914.4265999, 1.4e-7, 1.0]])
    path = str(tmp_path / "x.lm")
    report.write_lm(path, hist)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    assert lines[0] == "1\t0.001\t2500.125\t310.5\t1"
    assert lines[1] == "2\t0.0001\t2600\t12.25\t0"
    assert lines[3] == "4\t0\t914.4265999\t1.4e-07\t1"
    np.testing.assert_array_equal(np.loadtxt(path)[:, 1:], hist)
