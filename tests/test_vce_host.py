"""Host side of the variance component estimation (no GPU): fba_vce_host -- csrc/fba_vce.h's group arithmetic, the one
k_vce_sums / k_vce_finish run on the device -- against numpy on the r, t of the dense restatement (tests/vce_ref.py)
of scenes A-D, its edge cases and refusals, report.write_vce's table and a stand-alone sanitizer program
(tests/vce_check.cpp).

Bars, none from a run of the code under test: the sums to 1e-13 relative (index order against np.add.at's index order:
the same additions; 720 terms of one sign would allow 720 x 1.1e-16 = 8e-14 for another order); the estimate, the factor
and the status from those sums by the same formula, to 4 ulp.
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import vce_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fish-eye_bundle_adjustment_amd", "csrc")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("vce_host")


def test_exports(fba):
    lib = fba.capi.lib
    for name in ("fba_vce", "fba_vce_host"):
        assert hasattr(lib, name) and name in fba.capi.EXPORTS
    assert hasattr(fba.capi.Context, "vce") and fba.capi.lib.fba_abi_version() == 2
    assert fba.capi.VCE_STATUS == ("ok", "empty", "weak", "clipped")


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_host_matches_numpy_on_the_restatement(fba, oracle, root, name):
    """every round's r, t of the restatement through fba_vce_host: sums, estimates, factors, statuses"""
    s = vr.restated(fba, oracle, root, name)
    for k in range(s.a.rounds):
        sums, s2, f, st = fba.capi.vce_host(s.group, s.a.r[k], s.a.t[k], s.n_groups)
        ref = vr.group_sums(s.group, s.a.r[k], s.a.t[k], s.n_groups)
        np.testing.assert_allclose(sums, ref, rtol=1e-13, atol=0)
        est = [vr.group_estimate(*ref[g]) for g in range(s.n_groups)]
        np.testing.assert_allclose(s2, [e[0] for e in est], rtol=1e-15 * 4)
        np.testing.assert_allclose(f, [e[1] for e in est], rtol=1e-15 * 4)
        assert st.tolist() == [e[2] for e in est]
        np.testing.assert_allclose(s.a.table[k, : s.n_groups, 3], s2, rtol=1e-13)


def test_edge_cases(fba):
    vh = fba.capi.vce_host
    # an empty group
    sums, s2, f, st = vh([0, 2], [2.0, 2.0], [2.0, 2.0], 3)
    assert st.tolist() == [vr.OK, vr.EMPTY, vr.OK] and s2[1] == 1.0 and f[1] == 1.0 and sums[1].tolist() == [0, 0, 0]
    # all ids -1
    sums, s2, f, st = vh([-1] * 4, [1.0] * 4, [2.0] * 4, 2)
    assert st.tolist() == [vr.EMPTY, vr.EMPTY] and sums[2].tolist() == [4.0, 8.0, 4.0]
    # R below min_redundancy (the default 1, and a caller's)
    _, s2, f, st = vh([0, 1, 1], [0.5, 1.0, 1.0], [9.0, 1.0, 1.0], 2)
    assert st.tolist() == [vr.WEAK, vr.OK] and s2[0] == 1.0 and f[0] == 1.0
    _, _, _, st = vh([0, 1, 1], [0.5, 1.0, 1.0], [9.0, 1.0, 1.0], 2, min_redundancy=2.5)
    assert st.tolist() == [vr.WEAK, vr.WEAK]
    # T = 0: CLIPPED at 1 / clip; an estimate above clip
    _, s2, f, st = vh([0, 0, 1, 1], [1.0] * 4, [0.0, 0.0, 1e4, 1e4], 2)
    assert st.tolist() == [vr.CLIPPED, vr.CLIPPED] and s2.tolist() == [0.01, 100.0]
    np.testing.assert_allclose(f, [10.0, 0.1], rtol=4e-16)
    _, s2, _, st = vh([0, 0], [1.0, 1.0], [0.0, 0.0], 1, clip=4.0)
    assert st.tolist() == [vr.CLIPPED] and s2[0] == 0.25
    # a NaN row
    with pytest.raises(fba.capi.FBAError) as e:
        vh([0, 0], [1.0, np.nan], [1.0, 1.0], 1)
    assert e.value.code == 6
    # n_groups 1 and 256
    _, s2, _, st = vh([0, 0, 0], [1.0] * 3, [1.0] * 3, 1)
    assert st.tolist() == [vr.OK] and s2[0] == 1.0
    g = np.arange(768) % 256
    sums, s2, _, st = vh(g, np.full(768, 0.5), np.ones(768), 256)
    assert (st == vr.OK).all() and (s2 == 2.0).all() and (sums[:256, 2] == 3).all() and sums[256, 2] == 0
    # no rows at all
    sums, _, _, st = vh([], [], [], 2)
    assert st.tolist() == [vr.EMPTY, vr.EMPTY] and not sums.any()


@pytest.mark.parametrize("kw", [dict(n_groups=0), dict(n_groups=257), dict(group=[0, 2]), dict(group=[0, -2]),
                                dict(max_rounds=0), dict(tol=np.nan), dict(tol=-1.0), dict(min_redundancy=np.inf),
                                dict(min_redundancy=-1.0), dict(clip=0.5), dict(clip=np.nan)])
def test_refused_arguments(fba, kw):
    args = dict(group=[0, 1], n_groups=2)
    args.update(kw)
    group, ng = args.pop("group"), args.pop("n_groups")
    with pytest.raises(fba.capi.FBAError) as e:
        fba.capi.vce_host(group, [1.0] * len(group), [1.0] * len(group), ng, **args)
    assert e.value.code == 1 and "fba_vce_host" in str(e.value)


def test_vce_table_round_trip(fba, tmp_path):
    from fba_amd import report
    rng = np.random.default_rng(5)
    tab = rng.uniform(0.5, 900.0, (3, 4, 4))
    tab[:, :, 2] = [[700, 20, 0, 6]] * 3
    res = SimpleNamespace(vce_component=np.array([0.385, 3.98, 1.0, 1.0]), vce_sigma=np.array([0.186, 0.599, np.nan, np.nan]),
                          vce_status=np.array([0, 3, 1, 0]), vce_table=tab, vce_rounds=3,
                          vce_names=["x", "y", "(no group)", "(priors)"])
    path = os.path.join(str(tmp_path), "t.vce")
    report.write_vce(path, res)
    names, rows, sr, comp, sig, words, hist = report.read_vce(path)
    assert names == res.vce_names and rows.tolist() == [700, 20, 0, 6] and words == ["OK", "CLIPPED", "EMPTY", "OK"]
    np.testing.assert_allclose(sr, tab[-1, :, 0], rtol=1e-14)
    np.testing.assert_allclose(comp, res.vce_component, rtol=1e-14)
    np.testing.assert_allclose(sig[:2], res.vce_sigma[:2], rtol=1e-14)
    assert np.isnan(sig[2:]).all()
    np.testing.assert_allclose(hist, tab, rtol=1e-14)
    with pytest.raises(ValueError):
        report.write_vce(path, object())


def test_cli_parsing(fba):
    from fba_amd import batch
    assert batch.parse_vce(["f", "--vce"]) == (["f"], "xy")
    assert batch.parse_vce(["--vce=camera_xy", "f"]) == (["f"], "camera_xy")
    assert batch.parse_vce(["f"]) == (["f"], None)
    with pytest.raises(ValueError):
        batch.parse_vce(["--vce=rows"])
    assert batch.parse_main(["f", "--vce=camera", "--reliability"]) == ("f", False, True)
    assert batch.cli(["main", "f", "--vce", "--robust", "huber"]) == 2


def test_sanitizer_program(tmp_path):
    """tests/vce_check.cpp: the header routines over the edge cases, compiled with the host compiler under
    AddressSanitizer and UBSan, run directly"""
    exe = os.path.join(str(tmp_path), "vce_check")
    # host code only: each sanitizer option applies to the host compilation (-Xarch_host), none to a device pass
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "vce_check.cpp"),
                    os.path.join(CSRC, "fba_api_host.cpp"), os.path.join(CSRC, "fba_plan.cpp"), os.path.join(CSRC, "fba_order.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and all(ln.startswith("ok ") for ln in lines), r.stdout + r.stderr
    assert len(lines) >= 8
