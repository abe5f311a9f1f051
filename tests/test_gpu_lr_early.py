"""k_lin_reduce's early queue: the camera entries' observation sums run on waves 4-7 while waves
0-3 are in the point phases (B) and (C), the waves meet at LDS arrival counters instead of workgroup barriers, and
every LDS row is written once, in (A).  Which wave sums which (part, entry) item, and how many of them are done
before (C) ends, now differs from launch to launch; the results must not.

The scenes, contexts and comparisons are test_gpu_lr_queue's (its CASES, _scene, _oracle, _check_every_pass and
their bars: xhat per group and per element at max(1e-9, 20 x the oracle's own spread of that pass), deltasum at
1e-9 of the first, the iteration count, adjust() bit-equal to the stepped loop).  No bar of its own.

1. test_run_to_run_bitwise     accumulate() eight times at one xhat: the whole reduce buffer bit-equal every time.
                               A camera sum read before its early task stored it, a U row read before (C) wrote it
                               or a raw Jp row overwritten before (B) read it is a race, and shows as a difference.
                               `chunk-nk1` has 17 observation parts over 160 observations (9 or 10 each).
2. test_control_chunk          `few`: its control chunk has no points, so waves 0-3 pass (B) and (C) at once while
                               the early tasks run; the oracle after every pass.
3. test_chunk_extremes         nK = 5: `full`, one chunk of 64 points x 4 observations = 256 (every thread of (A),
                               (B) and (C) busy, every observation part 42 or 43 long), and `tiny`, a two-camera
                               scene whose first camera has one regular point of two observations -- a chunk of
                               its own, four of its six observation parts empty -- ahead of the second camera's
                               chunk (the other points, seen through both cameras, are general points).  The
                               oracle after every pass.
4. test_damped_orders_bitwise  `chunk` under set_damping(1e-3): the WH = true instantiation reading lambda; the
                               reduce buffer and the step bit-equal under FBA_LR_ORDER 0-3.
"""
import re

import numpy as np
import pytest

from test_gpu_lr_queue import ORDERS,_Hip, _check_every_pass, _ctx, _oracle, _scene, _set_env, _weights

pytestmark = pytest.mark.gpu

RUNS = 8
# seeds: of 1..6 the one at which the dense oracle's own two variants (explicit inverse, LU) agree best in deltasum
# (full: 1.0e-10 of the first at seed 4, 2.1e-10 .. 2.7e-8 at the others; tiny: 6.3e-11 at seed 2, up to 1.0e-9),
# the bar being 1e-9; neither has a deltasum within 1.25x of Threshold_Value (asserted by _check_every_pass)
FULL = dict(n_img=12, n_tie=64, seed=4, obs_per_point=4)
TINY = dict(n_img=12, n_tie=60, seed=2, obs_per_point=4, n_cam=2, cam_layout="blocks")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("lr_early"), "scenes": {}, "oracle": {}}


@pytest.mark.parametrize("case", ["chunk", "chunk-nk1", "chunk-nk8-radial", "dense", "wide-hbm", "chunk-weighted"])
def test_run_to_run_bitwise(fba, work, case, monkeypatch):
    _set_env(monkeypatch, case)
    ds = _scene(fba, work, case)["ds"]
    hip = _Hip()
    ctx = _ctx(fba, ds, _weights(case, 2 * ds.n_pts))
    try:
        bufs = []
        for _ in range(RUNS):
            ctx.accumulate()
            ctx.synchronize()
            bufs.append(hip.d2h(*ctx.reduce_buffer()))
    finally:
        ctx.close()
    assert np.isfinite(bufs[0]).all() and np.abs(bufs[0]).max() > 0
    for r in range(1, RUNS):
        assert bufs[r].tobytes() == bufs[0].tobytes(), \
            f"run {r} differs from run 0 in {int((bufs[r] != bufs[0]).sum())} of {bufs[0].size} entries"


def test_control_chunk(fba, oracle, work, monkeypatch):
    _set_env(monkeypatch, "few")
    s = _scene(fba, work, "few")
    assert s["ds"].n_pts > 18  # the control observations are there: a chunk without points
    _check_every_pass(fba, s["ds"], _oracle(oracle, work, s, "few"), None, "early few")


def _tiny_scene(synth):
    """TINY with one regular point of two observations alone in the first camera: of the points seen through camera
    0 only, the first keeps two of its observations, and every other one gets one of its image points measured a
    second time (fresh noise), which makes it a general point and leaves the geometry as it is"""
    sc = synth.generate(**TINY)
    cam_o = sc["cam"][sc["img"]]
    n_tie = len(sc["X0"])
    only = [np.array([(cam_o[sc["pid"] == j] == k).all() for j in range(n_tie)]) for k in (0, 1)]
    assert only[0].sum() >= 2 and only[1].sum() >= 1, "the seed gives no points seen through one camera only"
    first = int(np.nonzero(only[0])[0][0])
    keep = np.ones(len(sc["img"]), bool)
    keep[np.nonzero(sc["pid"] == first)[0][2:]] = False
    dup = np.array([np.nonzero(sc["pid"] == j)[0][0] for j in np.nonzero(only[0])[0][1:]])
    rng = np.random.default_rng(TINY["seed"])
    out = dict(sc)
    out["img"] = np.concatenate([sc["img"][keep], sc["img"][dup]])
    out["pid"] = np.concatenate([sc["pid"][keep], sc["pid"][dup]])
    out["xy"] = np.concatenate([sc["xy"][keep], sc["xy"][dup] + rng.normal(0, 0.3, (len(dup), 2))])
    return out, int(only[1].sum())


def _extreme(fba, work, name):
    if name not in work["scenes"]:
        from fba_amd import synth
        if name == "full":
            sc, n_other = synth.generate(**FULL), 0
        else:
            sc, n_other = _tiny_scene(synth)
        folder = synth.write_folder(sc, str(work["root"] / name), nk=5)
        work["scenes"][name] = {"folder": folder, "ds": fba.load_folder(folder), "n_other": n_other}
    return work["scenes"][name]


def _extreme_oracle(oracle, work, s, name):
    from test_gpu_block_shapes import _errors, _solve_lu
    if name not in work["oracle"]:
        od = oracle.load_folder(s["folder"])
        ro, lu = oracle.adjust(od), oracle.adjust(od, solver=_solve_lu)
        assert lu.iterations == ro.iterations
        work["oracle"][name] = dict(
            ro=ro, lu=lu, spread=[_errors(lu.xhat_hist[i], ro.xhat_hist[i], ro) for i in range(ro.iterations + 1)],
            spread_dsum=np.abs(np.array(lu.deltasum) - np.array(ro.deltasum)) / ro.deltasum[0])
    return work["oracle"][name]


@pytest.mark.parametrize("name", ["full", "tiny"])
def test_chunk_extremes(fba, oracle, work, name, monkeypatch, capfd):
    for k in ("FBA_LR_ORDER", "FBA_PAIR_TERMS", "FBA_ND_LEAF"):
        monkeypatch.delenv(k, raising=False)
    s = _extreme(fba, work, name)
    ds = s["ds"]
    capfd.readouterr()
    ctx = _ctx(fba, ds, None, verbose=True)
    ctx.close()
    m = re.search(r"chunks (\d+), pair keys", capfd.readouterr().err)
    assert m, "the context's verbose line"
    # the case still has the shape it was written for
    if name == "full":
        assert ds.n_pts == 256 and int(m.group(1)) == 1
    else:
        assert 1 <= s["n_other"] <= 64 and int(m.group(1)) == 2
    _check_every_pass(fba, ds, _extreme_oracle(oracle, work, s, name), None, f"early {name}")


def test_damped_orders_bitwise(fba, work, monkeypatch):
    ds = _scene(fba, work, "chunk")["ds"]
    hip = _Hip()
    runs = {}
    for order in ORDERS:
        _set_env(monkeypatch, "chunk", order)
        ctx = _ctx(fba, ds, None)
        try:
            ctx.set_damping(1e-3)
            ctx.accumulate()
            ctx.synchronize()
            buf = hip.d2h(*ctx.reduce_buffer())
            runs[order] = (buf, ctx.step(), ctx.get_xhat())
        finally:
            ctx.close()
    assert np.isfinite(runs[0][0]).all() and np.abs(runs[0][0]).max() > 0
    for order in ORDERS[1:]:
        assert runs[order][0].tobytes() == runs[0][0].tobytes(), \
            f"reduce buffer: FBA_LR_ORDER={order} differs in {int((runs[order][0] != runs[0][0]).sum())} entries"
        assert runs[order][1] == runs[0][1]
        assert runs[order][2].tobytes() == runs[0][2].tobytes()
    # the damping reached the point blocks: an undamped context's reduce buffer differs
    ctx = _ctx(fba, ds, None)
    try:
        ctx.accumulate()
        ctx.synchronize()
        assert hip.d2h(*ctx.reduce_buffer()).tobytes() != runs[0][0].tobytes()
    finally:
        ctx.close()
