"""k_lin_reduce's phase (D) as a wave-granular task queue (camera entries, image keys, pair keys; DESIGN 2
item 1): the result must not depend on which wave ran which task, nor on the order the tasks are handed out.

Per case, two checks:

(a) test_task_orders_bitwise.  Contexts under FBA_LR_ORDER = 0 (the default), 1 (camera, image, pair), 2 (image,
    pair, camera) and 3 (image, camera, pair): accumulate() at the same xhat and the whole reduce buffer read
    back must be equal bit for bit, then adjust() must give bit-equal xhat and deltasum histories.  A camera sum
    read ahead of a late camera task, an image-key unit split across two tasks or an item run twice or not at
    all shows up here.
(b) test_default_order_every_pass.  The default order against the dense oracle after EVERY pass, with the
    comparison and the bars of test_gpu_block_shapes._every_pass (restated in _check_every_pass, since that helper
    is tied to its ROWS table): xhat per group and per element at max(1e-9, 20 x the oracle's own spread of that
    pass -- explicit bordered inverse against an LU solve), deltasum at 1e-9 of the first, the iteration count,
    adjust() bit-equal to the stepped loop.

Cases -- the smallest shapes at which the queue can go wrong (task counts at nK = 5: 8 camera tasks of 64 items,
16 / lanes image-key units and 64 pair-key items per task):

few            3 images, 6 tie points of 3 observations: one chunk of 18 observations, one part-filled task of the
               image keys (9 units) and of the pair keys (9 items); most waves find the queue empty at once.  18
               tie observations cannot carry a free network's datum and 10 camera unknowns (36 equations for 46
               unknowns; the dense oracle diverges, or divides by a zero redundancy with the camera fixed), so
               this case has inner constraints OFF: three control points (9 observations, a control chunk of
               their own: no points, no pair keys) carry the datum, and the distortion terms are not estimated.
chunk          12 images x 40 points of 4 observations, nK = 5: one ordinary chunk (160 observations), part-filled
               last tasks of every kind (455 camera items, 36 units, ~111 pair items).
chunk-nk1      the same at nK = 1: CAM_SPLIT = 18, 486 camera items (the most of any nK).
chunk-nk8      the same at nK = 8: CAM_SPLIT = 4, 416 camera items, chunks of <= 32 points and <= 1024 terms (two
               chunks).  160 observations do not determine eight radial terms: with them estimated the dense
               oracle's own two variants (explicit inverse, LU) differ in deltasum by 2.1e-6 of the first on this
               seed and by >= 2.1e-7 on every seed 1..60 (and under the other four camera types, a tenth of the
               noise or a narrower field), so _every_pass's fixed deltasum bar of 1e-9 is beyond what the
               reference itself reproduces (measured on the GPU: 1.0e-6, every xhat group within its bar).
               This case therefore holds the radial terms fixed (Estimate_Radial_Distortions 0; the kernel is
               still the nK = 8 instantiation with its 416 camera items; oracle's own deltasum spread 1.1e-11).
chunk-nk8-radial  the same with the eight radial terms estimated, all 13 camera columns live: check (a) only, for
               the reason above.
dense          a convergent network, 40 images x 60 points of 38 observations (30 images cannot reach image keys of
               <= 2 observations: a point of 38 observations has 703 pair terms, so a chunk holds two points and
               its ~40 image keys 76 observations): the 4-lane image keys, and U-row chunks (no pair tasks).
dense-partials the same under FBA_PAIR_TERMS=0: the same chunks take the pair-partial path, ~770 pair keys each --
               36 pair tasks, more than the eight waves.
wide-hbm       one tie point seen by 65 of 70 images: 2,080 pair terms > chunk_terms = 2,048, so its chunk's term
               lists stay in HBM (stage_terms false) -- under FBA_PAIR_TERMS=0, since by default a chunk of one
               point (one term per key) is a U-row chunk and registers no pair keys at all; 98 pair tasks.
chunk-weighted `chunk` with non-uniform weights (set_weights): the WH = true instantiation; the oracle with the
               weighted P (test_gpu_weights._solvers).

Seeds: no entry of the oracle's deltasum history lies within a factor 1.25 of Threshold_Value (asserted).
"""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = (0, 1, 2, 3)
NODIST = {"Estimate_Radial_Distortions": "0", "Estimate_Decentering_Distortions": "0"}
CHUNK = ("grid", dict(n_img=12, n_tie=40, seed=3, obs_per_point=4))
DENSE = ("convergent", dict(n_img=40, n_tie=60, seed=1, obs_per_point=38))
WIDE = ("grid", dict(n_img=70, n_tie=300, seed=1, obs_per_point=4, n_wide=1, wide_min_obs=65))
# lanes: the image-key lanes the context must report; pair_keys / urow_terms: whether it must register any
CASES = {
    "few": dict(scene=("grid", dict(n_img=3, n_tie=9, seed=1, obs_per_point=3, n_control=3)), nk=5, cfg=NODIST,
                lanes=8, pair_keys=True, urow_terms=False),
    "chunk": dict(scene=CHUNK, nk=5, lanes=8, pair_keys=True, urow_terms=False),
    "chunk-nk1": dict(scene=CHUNK, nk=1, lanes=8, pair_keys=True),
    "chunk-nk8": dict(scene=CHUNK, nk=8, cfg={"Estimate_Radial_Distortions": "0"}, lanes=8, pair_keys=True),
    "chunk-nk8-radial": dict(scene=CHUNK, nk=8, lanes=8, pair_keys=True, every_pass=False),
    "dense": dict(scene=DENSE, nk=5, lanes=4, urow_terms=True),
    "dense-partials": dict(scene=DENSE, nk=5, lanes=4, env={"FBA_PAIR_TERMS": "0"}, pair_keys=True, urow_terms=False),
    "wide-hbm": dict(scene=WIDE, nk=5, lanes=8, env={"FBA_PAIR_TERMS": "0"}, pair_keys=True, urow_terms=False),
    "chunk-weighted": dict(scene=CHUNK, nk=5, lanes=8, weight_seed=3, pair_keys=True, urow_terms=False),
}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the module's scene folders, datasets and oracle runs: computed once, shared by both tests"""
    return {"root": tmp_path_factory.mktemp("lr_queue"), "scenes": {}, "oracle": {}}


def _scene(fba, work, case):
    c = CASES[case]
    kind, kw = c["scene"]
    key = (kind, tuple(sorted(kw.items())), c["nk"], tuple(sorted(c.get("cfg", {}).items())))
    if key not in work["scenes"]:
        from fba_amd import synth
        sc = (synth.generate_convergent if kind == "convergent" else synth.generate)(**kw)
        folder = synth.write_folder(sc, str(work["root"] / f"s{len(work['scenes'])}"), nk=c["nk"],
                                    cfg_overrides=c.get("cfg"))
        work["scenes"][key] = {"folder": folder, "ds": fba.load_folder(folder), "key": key}
    return work["scenes"][key]


def _weights(case, n):
    """log-uniform in [0.1, 10], x and y rows drawn independently; None: unweighted"""
    seed = CASES[case].get("weight_seed")
    return None if seed is None else 10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def _set_env(monkeypatch, case, order=None):
    for k in ("FBA_LR_ORDER", "FBA_PAIR_TERMS", "FBA_ND_LEAF"):
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[case].get("env", {}).items():
        monkeypatch.setenv(k, v)
    if order is not None:
        monkeypatch.setenv("FBA_LR_ORDER", str(order))


def _ctx(fba, ds, wt, **kw):
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)
    if wt is not None:
        ctx.set_weights(wt)
    return ctx


class _Hip:
    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so")
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def d2h(self, ptr, n):
        a = np.empty(n)
        assert self.lib.hipMemcpy(a.ctypes.data, ptr, n * 8, 2) == 0
        return a


@pytest.mark.parametrize("case", sorted(CASES))
def test_task_orders_bitwise(fba, work, case, monkeypatch, capfd):
    ds = _scene(fba, work, case)["ds"]
    wt = _weights(case, 2 * ds.n_pts)
    hip = _Hip()
    runs = {}
    for order in ORDERS:
        _set_env(monkeypatch, case, order)
        capfd.readouterr()
        ctx = _ctx(fba, ds, wt, verbose=True)
        try:
            m = re.search(r"chunks (\d+), pair keys (\d+), U-row pair terms (\d+), image keys (\d+) \((\d+) lanes each\)",
                          capfd.readouterr().err)
            assert m, "the context's verbose line"
            n_chunks, n_pk, n_tt, n_ik, lanes = (int(g) for g in m.groups())
            ctx.accumulate()
            ctx.synchronize()
            buf = hip.d2h(*ctx.reduce_buffer())
            it, dsum = ctx.adjust()
            runs[order] = (buf, ctx.get_xhat(), it, dsum)
        finally:
            ctx.close()
    c = CASES[case]
    print(f"lr-queue {case}: chunks {n_chunks}, pair keys {n_pk}, U-row terms {n_tt}, image keys {n_ik} on {lanes} lanes; "
          f"{runs[0][2]} passes")
    # the case still has the shape it was written for
    assert lanes == c["lanes"]
    if "pair_keys" in c:
        assert (n_pk > 0) == c["pair_keys"]
    if "urow_terms" in c:
        assert (n_tt > 0) == c["urow_terms"]
    assert np.isfinite(runs[0][0]).all() and np.abs(runs[0][0]).max() > 0
    for order in ORDERS[1:]:
        for q, name in enumerate(("reduce buffer", "xhat")):
            a, b = runs[0][q], runs[order][q]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
                f"{name}: FBA_LR_ORDER={order} differs from the default in {int((a != b).sum())} of {a.size} entries"
        assert runs[order][2] == runs[0][2]
        assert runs[order][3].tobytes() == runs[0][3].tobytes(), (order, runs[order][3], runs[0][3])


def _oracle(oracle, work, s, case):
    """the dense oracle's run, its LU variant and the oracle's own spread per pass (test_gpu_block_shapes._oracle,
    with the weighted P where the case has weights)"""
    from test_gpu_block_shapes import _errors, _solve_lu
    key = (s["key"], CASES[case].get("weight_seed"))
    if key not in work["oracle"]:
        od = oracle.load_folder(s["folder"])
        wt = _weights(case, od.n)
        if wt is None:
            ro, lu = oracle.adjust(od), oracle.adjust(od, solver=_solve_lu)
        else:
            from test_gpu_weights import _solvers
            inv, lus = _solvers(oracle, wt)
            ro, lu = oracle.adjust(od, solver=inv), oracle.adjust(od, solver=lus)
        assert lu.iterations == ro.iterations
        work["oracle"][key] = dict(
            ro=ro, lu=lu, spread=[_errors(lu.xhat_hist[i], ro.xhat_hist[i], ro) for i in range(ro.iterations + 1)],
            spread_dsum=np.abs(np.array(lu.deltasum) - np.array(ro.deltasum)) / ro.deltasum[0])
    return work["oracle"][key]


def _check_every_pass(fba, ds, ref, wt, tag):
    """test_gpu_block_shapes._every_pass's comparison of the stepped loop, at its bars"""
    from test_gpu_block_shapes import _errors, _fmt
    ro = ref["ro"]
    thr = ds.settings["threshold"]
    near = [d for d in ro.deltasum if thr / 1.25 <= d <= thr * 1.25]
    assert not near, f"{tag}: the oracle's deltasum {near} is within 1.25x of Threshold_Value: pick another seed"
    ctx = _ctx(fba, ds, wt)
    try:
        hist, dsum = [ctx.buildxhat()], []
        for _ in range(ro.iterations):
            dsum.append(ctx.step())
            hist.append(ctx.get_xhat())
    finally:
        ctx.close()
    np.testing.assert_array_equal(hist[0], ro.xhat_hist[0])
    failed = []
    for i in range(1, ro.iterations + 1):
        err, spread = _errors(hist[i], ro.xhat_hist[i], ro), ref["spread"][i]
        e_d = abs(dsum[i - 1] - ro.deltasum[i - 1]) / ro.deltasum[0]
        print(f"lr-queue {tag} pass {i} (error/oracle's own spread): deltasum={e_d:.1e}/{ref['spread_dsum'][i - 1]:.1e} "
              + _fmt(err, spread))
        failed += [(i, g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
        if not e_d <= 1e-9:
            failed.append((i, "deltasum", e_d, ref["spread_dsum"][i - 1]))
    assert not failed, failed  # (pass, group, error, the oracle's own spread)
    ctx = _ctx(fba, ds, wt)
    try:
        it, _ = ctx.adjust()
        xhat = ctx.get_xhat()
    finally:
        ctx.close()
    assert it == ro.iterations
    np.testing.assert_array_equal(xhat, hist[-1])


@pytest.mark.parametrize("case", sorted(c for c in CASES if CASES[c].get("every_pass", True)))
def test_default_order_every_pass(fba, oracle, work, case, monkeypatch):
    _set_env(monkeypatch, case)
    s = _scene(fba, work, case)
    ref = _oracle(oracle, work, s, case)
    _check_every_pass(fba, s["ds"], ref, _weights(case, 2 * s["ds"].n_pts), case)
