"""Host side of the data snooping (no GPU): fba_snoop_host -- csrc/fba_snoop.h's selection, the one k_snoop_stat /
k_snoop_seg / k_snoop_pick run on the device -- against the selection of the dense restatement (tests/snoop_ref.py) on
the restatement's own W of scenes A, C and P, its edge cases and refusals, report.write_snp's table, the command
line's option and a stand-alone sanitizer program (tests/snoop_check.cpp: the header routines and build_point_list).

The selection is discrete: every comparison is exact (the restated scenes keep every W 2 % away from crit, so the two
implementations cannot disagree on a rounding).
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import snoop_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fish-eye_bundle_adjustment_amd", "csrc")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("snoop_host")


def test_exports(fba):
    lib = fba.capi.lib
    for name in ("fba_snoop", "fba_snoop_host"):
        assert hasattr(lib, name) and name in fba.capi.EXPORTS
    assert hasattr(fba.capi.Context, "snoop") and fba.capi.lib.fba_abi_version() == 2
    assert fba.capi.SNOOP_STATE == ("active", "excluded", "readmitted")


@pytest.mark.parametrize("name", ["A", "C", "P"])
def test_host_matches_the_restatement(fba, oracle, root, name):
    """every round's W and state of the restatement through fba_snoop_host: the picks and the re-admissions"""
    s = sr.restated(fba, oracle, root, name)
    a = s.a
    tie, img = np.asarray(s.od.tie_index), np.asarray(s.od.ext_index)
    state = np.zeros(len(tie), dtype=np.uint8)
    state[s.pre] = sr.EXCLUDED
    assert a.rounds >= 2 and (name != "A" or (len(a.picks[0]) >= 1 and len(a.picks[1]) >= 1))
    for k in range(a.rounds):
        pick, back, bits = fba.capi.snoop_host(a.W[k], state, tie, img)
        assert np.nonzero(pick)[0].tolist() == a.picks[k].tolist() and np.nonzero(back)[0].tolist() == a.backs[k].tolist()
        assert bits == 0
        state = a.state[k]
    assert a.table[-1, :2].tolist() == [0, 0] and a.table[-1, 2] == len(s.rows)


def test_edge_cases(fba):
    sh = fba.capi.snoop_host
    tie, img = [0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2]
    kw = dict(min_img_points=1, max_share=1.0)
    # no candidates
    pick, back, bits = sh([1, 2, 3, 1, 2, 3], [0] * 6, tie, img, **kw)
    assert not pick.any() and not back.any() and bits == 0
    # the local-maximum rule: row 0 wins its tie point and its image, its neighbours wait
    pick, _, _ = sh([9, 5, 1, 8, 1, 4], [0] * 6, tie, img, **kw)
    assert pick.tolist() == [True, False, False, False, False, False]
    # equal W: the lower row wins
    pick, _, _ = sh([7, 7, 1, 1, 1, 1], [0] * 6, tie, img, **kw)
    assert pick.tolist() == [True, False, False, False, False, False]
    # a two-ray tie point is never eligible; a control observation skips the condition
    pick, _, _ = sh([9, 1, 9, 9], [0] * 4, [0, 0, -1, -1], [0, 1, 1, 1], **kw)
    assert pick.tolist() == [False, False, True, False]
    # an image at min_img_points keeps its points
    pick, _, _ = sh([9, 5, 1, 8, 1, 4], [0] * 6, tie, img, min_img_points=2, max_share=1.0)
    assert not pick.any()
    # the max_share stop: the pick would make 1 of 6 > 5 %
    pick, back, bits = sh([9, 5, 1, 8, 1, 4], [0] * 6, tie, img, min_img_points=1)
    assert not pick.any() and not back.any() and bits == 2
    # the back-check runs only where nothing is picked; a re-admitted point is never a candidate again
    pick, back, _ = sh([1, 2, 9, np.nan, 3.29, 9], [0, 0, 1, 1, 1, 2], tie, img, min_rays=1, **kw)
    assert not pick.any() and back.tolist() == [False, False, False, False, True, False]
    pick, back, _ = sh([9, 2, 9, 1, 1, 1], [0, 0, 1, 0, 1, 0], tie, img, min_rays=1, **kw)
    assert pick.tolist() == [True, False, False, False, False, False] and not back.any()
    # a caller's crit
    pick, _, _ = sh([9, 5, 1, 8, 1, 4], [0] * 6, tie, img, crit=9.5, **kw)
    assert not pick.any()
    # empty lists
    pick, back, bits = sh([], [], [], [])
    assert pick.size == 0 and back.size == 0 and bits == 0
    pick, back, bits = sh([], [], [], [], n_tie=3, n_img=2)
    assert pick.size == 0 and bits == 0


@pytest.mark.parametrize("kw", [dict(max_rounds=0), dict(min_rays=0), dict(min_img_points=0), dict(crit=0.0), dict(crit=-1.0),
                                dict(crit=np.nan), dict(crit=np.inf), dict(max_share=0.0), dict(max_share=1.5),
                                dict(max_share=np.nan), dict(tie=[0, 5]), dict(img=[0, -1]), dict(img=[0, 2]),
                                dict(state=[0, 3])])
def test_refused_arguments(fba, kw):
    args = dict(W=[1.0, 1.0], state=[0, 0], tie=[0, 0], img=[0, 1], n_tie=1, n_img=2)
    args.update(kw)
    with pytest.raises(fba.capi.FBAError) as e:
        fba.capi.snoop_host(**args)
    assert e.value.code == 1 and "fba_snoop_host" in str(e.value)


def test_snp_table_round_trip(fba, tmp_path):
    from fba_amd import report
    n = 9
    data = SimpleNamespace(pho_image=[str(1000 + i // 3) for i in range(n)], pho_target=[f"P{i:06d}" for i in range(n)])
    ex = np.zeros(n, dtype=np.uint8)
    ex[[2, 7]] = 1
    ex[4] = 2
    rng = np.random.default_rng(5)
    res = SimpleNamespace(snoop_excluded=ex, snoop_stat=rng.uniform(0.1, 20.0, n), v=rng.normal(0, 2.0, 2 * n),
                          snoop_table=np.array([[2, 0, 3, 17.25], [0, 1, 2, 3.1], [0, 0, 2, 3.05]]), snoop_rounds=3)
    path = os.path.join(str(tmp_path), "t.snp")
    report.write_snp(path, data, res)
    rows, imgs, pts, words, stat, v, hist = report.read_snp(path)
    assert rows.tolist() == [2, 4, 7] and words == ["EXCLUDED", "READMITTED", "EXCLUDED"]
    assert imgs == ["1000", "1001", "1002"] and pts == ["P000002", "P000004", "P000007"]
    np.testing.assert_allclose(stat, res.snoop_stat[rows], rtol=1e-14)
    np.testing.assert_allclose(v, res.v.reshape(-1, 2)[rows], rtol=1e-14)
    np.testing.assert_allclose(hist, res.snoop_table, rtol=1e-14)
    with pytest.raises(ValueError):
        report.write_snp(path, data, object())


def test_cli_parsing(fba):
    from fba_amd import batch
    assert batch.parse_snoop(["f", "--snoop"]) == (["f"], True)
    assert batch.parse_snoop(["--snoop=4.1", "f"]) == (["f"], 4.1)
    assert batch.parse_snoop(["f"]) == (["f"], None)
    for bad in ("--snoop=0", "--snoop=-2", "--snoop=x", "--snoop=inf"):
        with pytest.raises(ValueError):
            batch.parse_snoop([bad])
    assert batch.parse_main(["f", "--snoop=4", "--reliability"]) == ("f", False, True)
    assert batch.cli(["main", "f", "--snoop", "--robust", "huber"]) == 2


def test_adjust_refuses_snoop_with_robust(fba):
    with pytest.raises(ValueError):
        fba.adjust(None, snoop=True, robust="huber")


def test_sanitizer_program(tmp_path):
    """tests/snoop_check.cpp: the header routines and build_point_list over the edge cases, compiled with the host
    compiler under AddressSanitizer and UBSan, run directly"""
    exe = os.path.join(str(tmp_path), "snoop_check")
    # host code only: each sanitizer option applies to the host compilation (-Xarch_host), none to a device pass
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "snoop_check.cpp"),
                    os.path.join(CSRC, "fba_api_host.cpp"), os.path.join(CSRC, "fba_plan.cpp"), os.path.join(CSRC, "fba_order.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and all(ln.startswith("ok ") for ln in lines), r.stdout + r.stderr
    assert len(lines) >= 9
