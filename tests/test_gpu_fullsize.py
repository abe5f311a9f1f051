"""GPU parity at BASELINE.json's scene sizes (synthetic fish-eye configs 3-5, synth.py).

* config 3 (200 images x 5,000 tie points, 50k image points) and a control-point scene: the whole
  adjustment (main.m:407-494) against the C restatement oracle/fba_cpu.c solving the reference's
  bordered system directly ("kkt") -- same iteration count, xhat <= 1e-9 relative per element and
  per parameter group (distortion terms in scaled units, conftest.elem_rel_err), sigma0^2 <= 1e-9.
* config 4 (1,000 x 50,000, the bench workload): the whole adjustment against the same oracle --
  iteration count, deltasum history, xhat, sigma0^2, RMS and v.
* config 5 (4,000 x 200,000, 2M image points): every Gauss-Newton pass to convergence against the C
  oracle's direct solve of the dense bordered system (each to its own stop: there the threshold sits at
  the rounding floor of deltasum; converged xhat, sigma0^2); then
  size-independent properties of the converged run -- bit-identical repeat runs, monotone convergence below Threshold_Value within
  Iteration_Cap, and sigma0^2 = 1 +- 5% (the generator's noise equals Meas_std, so the a posteriori
  variance factor of a correct adjustment is ~1).
"""
import os

import numpy as np
import pytest

from conftest import dist_scaling_of, distortion_scale, elem_rel_err, group_rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fbo():
    import fba_cpu
    fba_cpu.build()
    return fba_cpu


def _scene(config, root, **kw):
    from fba_amd import synth
    folder = os.path.join(root, f"c{config}")
    if not os.path.exists(os.path.join(folder, ".done")):
        synth.make_config(config, folder, **kw)
        open(os.path.join(folder, ".done"), "w").close()
    return folder


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fullsize"))


def _ctx(fba, ds):
    return fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))


def _check_adjust(fba, fbo, oracle, folder):
    ds = fba.load_folder(folder)
    od = oracle.load_folder(folder)
    ref = fbo.CpuAdjustment(od, solver="kkt")
    it = ref.adjust()
    _, s02 = ref.residuals()
    res = fba.adjust(ds)
    assert res.iterations == it
    dsc = dist_scaling_of(od)
    err = group_rel_err(res.xhat, ref.xhat, ref.names, dsc)
    assert max(err.values()) <= 1e-9, err
    err = elem_rel_err(res.xhat, ref.xhat, ref.names, dsc)
    print("per-element relative error per group:", {g: f"{e:.2e}" for g, e in err.items()})
    assert max(err.values()) <= 1e-9, err
    assert abs(res.sigma02 - s02) <= 1e-9 * s02
    np.testing.assert_allclose(res.deltasum, ref.deltasum, rtol=0, atol=1e-9 * ref.deltasum[0])


def test_config3_adjust_matches_oracle(fba, fbo, oracle, scenes):
    _check_adjust(fba, fbo, oracle, _scene(3, scenes))


@pytest.mark.parametrize("env", [{"FBA_CHOL_FLOW": "0"}, {"FBA_BWD_LEVELS": "1"},
                                 {"FBA_CHOL_FLOW": "0", "FBA_BWD_LEVELS": "1"},
                                 {"FBA_FLOW_BLOCK": "1"}, {"FBA_FLOW_BLOCK": "2"}, {"FBA_FLOW_BLOCK": "3"},
                                 {"FBA_FLOW_BLOCK": "1", "FBA_FLOW_SPLIT": "1"},
                                 {"FBA_FLOW_BLOCK": "1", "FBA_FLOW_MSPLIT": "8"},
                                 {"FBA_FLOW_MERGE": "0"}, {"FBA_ND_LEAF": "60"}, {"FBA_PAIR_TERMS": "1000"}],
                         ids=["per-level-factor", "per-level-backward", "both", "whole-block-updates",
                              "whole-block-but-last-group", "whole-block-then-quarters", "whole-block-partials", "whole-block-merged-partials",
                              "no-level-merging", "nd-leaf-60", "pair-terms-from-u-rows"])
def test_config3_fallback_paths_match_oracle(fba, fbo, oracle, scenes, env, monkeypatch):
    """The non-default solve paths (read per context in chol_setup): the per-level k_panel launches
    instead of the persistent k_chol_flow (with k_border_gram -> k_border_combine), and the per-level
    k_bwd_wave backward solve instead of k_bwd_flow -- the paths build_flow's order check falls back
    to, and the one the 2-rank rehearsal used.  FBA_FLOW_BLOCK: k_chol_flow's whole-block update records
    (syrk_block_body; config 3 is latency-bound, so its default is quarter records) for every writer
    group, for all but each target's last group, or for the leading groups with the quarter records
    chained after them; with one source per
    record (FBA_FLOW_SPLIT=1) or merged writer groups of up to 8 sources (FBA_FLOW_MSPLIT=8), so targets
    are summed through the 128 x 128 scratch partials the last arriving record combines.  FBA_FLOW_MERGE=0:
    one writer group per source level (no merging of consecutive levels); FBA_ND_LEAF=60: smaller
    nested-dissection leaves (another block pattern); FBA_PAIR_TERMS=1000: every chunk's pair terms
    reduced by k_red_blocks from the observations' U rows (AccPlan::ck_tm; the grid's keys hold ~12 terms
    each, so by default they take the partial rows)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_adjust(fba, fbo, oracle, _scene(3, scenes))


@pytest.mark.parametrize("env", [{}, {"FBA_PAIR_TERMS": "0"}], ids=["default", "pair-partials"])
def test_convergent_config3_adjust_matches_oracle(fba, fbo, oracle, scenes, env, monkeypatch):
    """config 3's counts (200 images x 5,000 tie points) as a convergent network (synth.
    generate_convergent: every tie point seen by 10 images drawn from the whole block, the reference's
    close-range setting): a dense reduced camera system, so the factorisation takes its dense-chain,
    MFMA-throughput form.  Whole adjustment against the C oracle's direct bordered solve.  Its chunks'
    pair keys hold ~1 term each, so by default their terms are reduced from U rows (AccPlan::ck_tm);
    FBA_PAIR_TERMS=0 forces the partial rows."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from fba_amd import synth
    folder = os.path.join(scenes, "c3_convergent")
    if not os.path.exists(os.path.join(folder, ".done")):
        synth.make_config(3, folder, network="convergent")
        open(os.path.join(folder, ".done"), "w").close()
    _check_adjust(fba, fbo, oracle, folder)


def test_control_points_adjust_matches_oracle(fba, fbo, oracle, tmp_path):
    """No inner constraints: 40 control points fix the datum (the cam0 configuration, at scale)."""
    from fba_amd import synth
    folder = synth.write_folder(synth.generate(120, 3000, seed=21, n_control=40), str(tmp_path / "ctl"))
    _check_adjust(fba, fbo, oracle, folder)


def test_config3_covariance_matches_oracle(fba, fbo, oracle, scenes):
    """fba_covariance at config 3 (u = 16,210): the camera-side diagonal of Cx (1e-8 relative) and the
    EOP/IOP correlation blocks (1e-8 absolute) against the dense inverse of the C oracle's last bordered
    reduced system [S G; G' 0] (the camera block of the bordered inverse of the full normal matrix,
    main.m:432); every tie-point variance positive and finite."""
    import scipy.linalg as sla
    folder = _scene(3, scenes)
    ds = fba.load_folder(folder)
    od = oracle.load_folder(folder)
    ref = fbo.CpuAdjustment(od, solver="kkt")
    ref.adjust()
    _, s02 = ref.residuals()
    uc = ref.u_c
    K = np.zeros((uc + 7, uc + 7))
    K[:uc, :uc] = ref.S
    K[:uc, uc:] = ref.G
    K[uc:, :uc] = ref.G.T
    C = sla.inv(K)[:uc, :uc]
    sc = distortion_scale(ref.names[:uc], dist_scaling_of(od))
    res = fba.adjust(ds)
    want = s02 * np.diag(C) / sc ** 2
    # bars: measured 4.4e-10 relative on the diagonal and 1.1e-9 absolute on the correlations (round 6,
    # profiles/r06_v7_measured_errors.log: the selected inverse of the Cholesky factor against the dense
    # inverse of the C oracle's own last normal matrix), held to ~20x / ~10x that
    print(f"config 3 diag(Cx): max relative error {np.max(np.abs(res.cx_diag[:uc] - want) / np.abs(want)):.2e}")
    np.testing.assert_allclose(res.cx_diag[:uc], want, rtol=1e-8)
    d = np.sqrt(np.diag(C))
    corr = C / np.outer(d, d)
    cam = 6 * od.numImg
    worst = 0.0
    for e in range(0, od.numImg, 17):
        idx = list(range(6 * e, 6 * e + 6)) + list(range(cam, cam + 10))
        worst = max(worst, float(np.max(np.abs(res.corr[e] - corr[np.ix_(idx, idx)]))))
        np.testing.assert_allclose(res.corr[e], corr[np.ix_(idx, idx)], rtol=0, atol=1e-8)
    print(f"config 3 correlation blocks: max absolute error {worst:.2e}")
    tie = res.cx_diag[uc:]
    assert np.isfinite(tie).all() and (tie > 0).all()


def test_config4_adjust_matches_oracle(fba, fbo, oracle, scenes):
    """The bench workload, converged: the whole adjustment (main.m:407-494) against the C oracle
    solving the reference's bordered system [S G; G' 0] directly -- same iteration count, the whole
    deltasum history, xhat <= 1e-9 relative per parameter group (distortion terms in the scaled
    units), sigma0^2 <= 1e-9 (main.m:601) and RMSx / RMSy (main.m:594-598) <= 1e-9."""
    folder = _scene(4, scenes)
    ds = fba.load_folder(folder)
    od = oracle.load_folder(folder)
    ref = fbo.CpuAdjustment(od, solver="kkt")
    it = ref.adjust()
    v_ref, s02 = ref.residuals()
    res = fba.adjust(ds, covariance=False)
    assert res.iterations == it
    np.testing.assert_allclose(res.deltasum, ref.deltasum, rtol=0, atol=1e-9 * ref.deltasum[0])
    err = group_rel_err(res.xhat, ref.xhat, ref.names, dist_scaling_of(od))
    assert max(err.values()) <= 1e-9, err
    err = elem_rel_err(res.xhat, ref.xhat, ref.names, dist_scaling_of(od))
    print("per-element relative error per group:", {g: f"{e:.2e}" for g, e in err.items()})
    assert max(err.values()) <= 1e-9, err
    assert abs(res.sigma02 - s02) <= 1e-9 * s02
    rms_ref = (np.sqrt(np.mean(v_ref[0::2] ** 2)), np.sqrt(np.mean(v_ref[1::2] ** 2)))
    assert abs(res.rms[0] - rms_ref[0]) <= 1e-9 * rms_ref[0] and abs(res.rms[1] - rms_ref[1]) <= 1e-9 * rms_ref[1]
    # per observation: v = A delta + w of the last linearisation (main.m:569)
    # (measured 4.0e-13 of the scale, round 6: profiles/r06_v7_measured_errors.log; held to 1e-10)
    print(f"config 4 v: max |dv| / max |v| = {np.max(np.abs(res.v - v_ref)) / np.max(np.abs(v_ref)):.2e}")
    assert np.max(np.abs(res.v - v_ref)) <= 1e-10 * np.max(np.abs(v_ref))


DISTORTION = ("k1", "k2", "k3", "k4", "k5", "p1", "p2")
# config 5: how far two exact CPU restatements land apart per element after each of the first passes
# (the direct bordered KKT solve vs the block-sparse Cholesky of oracle/fba_cpu.c, both from the same
# start; profiles/r04_c5_elem_spread.log): the first passes' large corrections make the small entries
# sensitive (the group scale agrees to 1e-9 / 1e-11); from pass 3 on both agree to <= 2.1e-10 per element
C5_ELEM_SPREAD = {1: 3.0e-8, 2: 4.7e-9}
# the per-element bars of those passes: the HIP path measured 9.6e-8 and 2.1e-9 (round 6,
# profiles/r06_v12_config5_errors.log), so the bars sit about 2x and 5x above that. In spread units
# they are ~7x and ~2x, down from the 20x of round 5 (6e-7 / 9.4e-8)
C5_ELEM_BAR = {1: 2e-7, 2: 1e-8}


def test_config5_adjust_matches_oracle(fba, fbo, oracle, scenes):
    """config 5 (4,000 images x 200,000 tie points, 2M image points, u_c = 24,010), converged: every
    Gauss-Newton pass against the C oracle solving the dense bordered system [S G; G' 0] (4.6 GB)
    directly, each run to the reference's stop rule (main.m:412, :490-493); xhat after the last update
    (main.m:484-493) and sigma0^2 (main.m:601).

    Pass by pass while deltasum is above the stop rule's rounding floor: deltasum <= 1e-9 relative; xhat
    <= 1e-9 per parameter group, except the distortion groups after the FIRST pass (the linearisation at
    the start values: the C oracle itself moves k1 by 1.2e-7 / 2.1e-7 when only its OpenMP thread count
    changes, profiles/r03_order_spread_c5.log) -- 5e-8 there (measured: 2.6e-8 for k1, round 6); per element the
    first two passes are held to C5_ELEM_BAR (2e-7 / 1e-8: ~7x / ~2x the spread of two exact restatements,
    C5_ELEM_SPREAD), later passes to 1e-9.  At convergence deltasum is the sum of |delta| over 624,010 unknowns of rounding-level
    corrections, ~1e-6 -- the very Threshold_Value 1e-6 -- so WHEN it drops below the threshold is decided
    by rounding: two exact CPU restatements stop after 9 and 7 passes (profiles/r04_c5_elem_spread.log).
    Each run therefore stops by its own rule; the passes both stay within 3 of each other, and the
    converged xhat agree to 1e-9 per element and per group, sigma0^2 and RMSx / RMSy to 1e-9."""
    folder = _scene(5, scenes)
    ds = fba.load_folder(folder)
    od = oracle.load_folder(folder)
    ref = fbo.CpuAdjustment(od, solver="kkt")
    ctx = _ctx(fba, ds)
    dsc = dist_scaling_of(od)
    thr, cap = ds.settings["threshold"], ds.settings["Iteration_Cap"]
    try:
        d_ref = d = 100.0  # main.m:407
        it_ref = it = 0
        while (d_ref > thr and it_ref < cap) or (d > thr and it < cap):  # main.m:412, :490-493, each run by its own deltasum
            if d_ref > thr and it_ref < cap:
                it_ref += 1
                d_ref = ref.step()
            if d > thr and it < cap:
                it += 1
                d = ctx.step()
            if it != it_ref or ref.deltasum[-1] < 1e3 * thr:
                continue  # below the comparison range: the tail is rounding noise
            assert abs(d - d_ref) <= 1e-9 * ref.deltasum[0], (it, d, d_ref)
            x = ctx.get_xhat()
            err = group_rel_err(x, ref.xhat, ref.names, dsc)
            print(f"pass {it} group:", {g: f"{e:.2e}" for g, e in err.items()})
            for g, e in err.items():
                assert e <= (5e-8 if it == 1 and g in DISTORTION else 1e-9), (it, g, e)
            err = elem_rel_err(x, ref.xhat, ref.names, dsc)
            print(f"pass {it} element:", {g: f"{e:.2e}" for g, e in err.items()})
            assert max(err.values()) <= C5_ELEM_BAR.get(it, 1e-9), (it, err)
        print(f"stopped after {it} passes (oracle {it_ref}); last deltasum {d:.3e} (oracle {d_ref:.3e})")
        assert d <= thr and d_ref <= thr and it < cap and it_ref < cap and abs(it - it_ref) <= 3
        x = ctx.get_xhat()
        for err in (group_rel_err(x, ref.xhat, ref.names, dsc), elem_rel_err(x, ref.xhat, ref.names, dsc)):
            print("converged:", {g: f"{e:.2e}" for g, e in err.items()})
            assert max(err.values()) <= 1e-9, err
        v_ref, s02 = ref.residuals()
        v, _, st = ctx.residuals()
        print(f"sigma0^2 {st[3]:.15g} (oracle {s02:.15g})")
        assert abs(st[3] - s02) <= 1e-9 * s02
        rms_ref = (np.sqrt(np.mean(v_ref[0::2] ** 2)), np.sqrt(np.mean(v_ref[1::2] ** 2)))
        assert abs(st[0] - rms_ref[0]) <= 1e-9 * rms_ref[0] and abs(st[1] - rms_ref[1]) <= 1e-9 * rms_ref[1]
    finally:
        ctx.close()
        ref.close()


def test_config5_properties(fba, scenes):
    folder = _scene(5, scenes)
    ds = fba.load_folder(folder)
    runs = []
    for _ in range(2):
        ctx = _ctx(fba, ds)
        try:
            runs.append(([ctx.step() for _ in range(2)], ctx.get_xhat()))
        finally:
            ctx.close()
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])  # deterministic
    res = fba.adjust(ds)
    d = np.array(res.deltasum)
    assert d[-1] <= ds.settings["threshold"] and res.iterations < ds.settings["Iteration_Cap"]
    assert (np.diff(d[:3]) < 0).all()
    assert abs(res.sigma02 - 1.0) <= 0.05, res.sigma02
    assert np.isfinite(res.xhat).all()
    assert np.isfinite(res.cx_diag).all() and (res.cx_diag > 0).all()  # fba_covariance at 2M image points


@pytest.mark.parametrize("world", [2, 8])
def test_config4_two_rank_shards_match_single_context(fba, scenes, world):
    """The multi-GPU split at the bench scene: `world` rank contexts (fba_partition's tie-point shards)
    on one GPU, their compact reduce buffers (~6 MB: co-visible image-pair blocks, diagonal blocks,
    camera rows, RHS row) summed on the host as the RCCL all-reduce would, reproduce the single
    context's iterates to 1e-10 over two Gauss-Newton passes; the deltasum shares add up to the
    single context's deltasum.  world = 8: the bench's default solve at --gpus 8, as rank contexts."""
    import ctypes
    folder = _scene(4, scenes)
    ds = fba.load_folder(folder)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    mk = lambda **kw: fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)  # noqa: E731
    single = mk()
    ranks = [mk(rank=r, world=world) for r in range(world)]
    try:
        d_first = None
        for _ in range(2):
            d1 = single.step()
            d_first = d_first or d1
            for c in ranks:
                c.accumulate()
                c.synchronize()
            bufs = [c.reduce_buffer() for c in ranks]
            assert all(n == bufs[0][1] for _, n in bufs) and bufs[0][1] * 8 < 16e6
            total = np.zeros(bufs[0][1])
            for p, n in bufs:
                a = np.empty(n)
                assert hip.hipMemcpy(a.ctypes.data, p, n * 8, 2) == 0
                total += a
            for p, n in bufs:
                assert hip.hipMemcpy(p, total.ctypes.data, n * 8, 1) == 0
            parts = [c.solve_update() for c in ranks]
            assert abs(sum(parts) - d1) <= 1e-9 * d_first
        xs = single.get_xhat()
        xr = sum(c.get_xhat(owned_only=True) for c in ranks)
        od_dsc = dist_scaling_of(__import__("fba_oracle").load_folder(folder))
        err = group_rel_err(xr, xs, fba.xhat_names(ds), od_dsc)
        assert max(err.values()) <= 1e-10, err
    finally:
        single.close()
        for c in ranks:
            c.close()


@pytest.mark.parametrize("config,world", [(3, 2), (4, 2), (5, 2), ("3-convergent", 2), (4, 8)])
def test_subtree_split_two_ranks_match_single_context(fba, scenes, config, world):
    """The subtree-split factorisation (fba_options.split): two rank contexts on one
    GPU, each factoring its own subtrees of the elimination tree inside fba_accumulate, their reduce
    buffers (the top blocks of the Schur complement, the top rows' accumulated diagonal, the subtree
    columns' Gram partials and inner-constraint weight sums) summed on the host as the RCCL all-reduce
    would; each then factors the top columns, back-substitutes and updates.  Over two Gauss-Newton passes
    at configs 3, 4 and 5 the ranks' owned entries reassemble the single context's xhat to 1e-10 per
    parameter group (1e-9 at config 5, below) and 1e-9 per element, and the deltasum shares add up to the single context's
    deltasum.  (One GPU stands in for two: the collective itself is unmeasured here.)  "3-convergent":
    config 3's counts as a convergent network -- a dense reduced system whose elimination tree is a chain,
    so the split falls back to the replicated solve (fba_solve_mode), with its chunks' pair terms reduced
    from U rows (AccPlan::ck_tm) on each rank.  (4, 8): eight rank contexts -- the priced cut (DESIGN.md
    section 7) may leave some ranks no subtree, only their tie points' linearisation and the top."""
    if config == "3-convergent":
        from fba_amd import synth
        folder = os.path.join(scenes, "c3_convergent")
        if not os.path.exists(os.path.join(folder, ".done")):
            synth.make_config(3, folder, network="convergent")
            open(os.path.join(folder, ".done"), "w").close()
    else:
        folder = _scene(config, scenes)
    # config 5's radial-distortion direction is the ill-conditioned one (the oracle's KKT solve reports
    # rcond ~1e-16): reduction-order rounding moves k1 by up to ~2e-10 of its group there (2.9e-11 at
    # config 3, 1.3e-12 at config 4), so config 5 is held to the oracle test's own 1e-9
    _split_ranks_match_single_context(fba, folder, world, 1e-9 if config == 5 else 1e-10)


def _split_ranks_match_single_context(fba, folder, world, group_bar, honoured=False):
    """the body of test_subtree_split_two_ranks_match_single_context on `folder`; honoured: fba_solve_mode
    must report the split on every rank (a fallback to the replicated solve would test nothing)"""
    import ctypes
    ds = fba.load_folder(folder)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    mk = lambda **kw: fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)  # noqa: E731
    single = mk()
    ranks = [mk(rank=r, world=world, split=True) for r in range(world)]
    try:
        if honoured:
            assert all(c.split for c in ranks)
        d_first = None
        for _ in range(2):
            d1 = single.step()
            d_first = d_first or d1
            for c in ranks:
                c.accumulate()
                c.synchronize()
            bufs = [c.reduce_buffer() for c in ranks]
            assert all(n == bufs[0][1] for _, n in bufs)
            total = np.zeros(bufs[0][1])
            for p, n in bufs:
                a = np.empty(n)
                assert hip.hipMemcpy(a.ctypes.data, p, n * 8, 2) == 0
                total += a
            for p, n in bufs:
                assert hip.hipMemcpy(p, total.ctypes.data, n * 8, 1) == 0
            parts = [c.solve_update() for c in ranks]
            assert abs(sum(parts) - d1) <= 1e-9 * d_first, (parts, d1)
        xs = single.get_xhat()
        xr = sum(c.get_xhat(owned_only=True) for c in ranks)
        names = fba.xhat_names(ds)
        dsc = dist_scaling_of(__import__("fba_oracle").load_folder(folder))
        err = group_rel_err(xr, xs, names, dsc)
        print("split vs single, relative error per group:", {g: f"{e:.2e}" for g, e in err.items()})
        assert max(err.values()) <= group_bar, err
        err = elem_rel_err(xr, xs, names, dsc)
        print("split vs single, relative error per element:", {g: f"{e:.2e}" for g, e in err.items()})
        assert max(err.values()) <= 1e-9, err
    finally:
        single.close()
        for c in ranks:
            c.close()


def test_subtree_split_covariance_matches_single_context(fba, scenes):
    """fba_covariance with the subtree split (config 3, two rank contexts on one GPU, host-summed reduce
    buffers): each rank's selected inverse runs over its own subtrees and the top -- the Takahashi
    recurrence of a column reads only its ancestors -- with the border's H from the all-reduced per-block
    Gram partials; a rank writes the camera-side variances of its own rows (the top's on rank 0), its
    points' variances and the correlation blocks of its images, so the ranks' outputs sum to the single
    context's diag(Cx) and correlation blocks.  Bars: 1e-8 relative on diag(Cx), 1e-9 absolute on the
    correlations (the two contexts factor the same system in another reduction order)."""
    _split_covariance_matches_single_context(fba, _scene(3, scenes), 2)


def test_subtree_split_covariance_eight_ranks_match_single_context(fba, scenes):
    """test_subtree_split_covariance_matches_single_context's body at config 4 on eight rank contexts, as
    test_subtree_split_two_ranks_match_single_context[4-8] runs the adjustment, at the same bars: the priced
    cut may leave some ranks no subtree, and every rank's selected inverse runs over seven other ranks'
    never-factored columns (fba_cov.hip, launch_covariance), which no output may read."""
    _split_covariance_matches_single_context(fba, _scene(4, scenes), 8)


def _split_covariance_matches_single_context(fba, folder, world):
    """the body of test_subtree_split_covariance_matches_single_context on `folder`"""
    import ctypes
    ds = fba.load_folder(folder)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    mk = lambda **kw: fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)  # noqa: E731
    single = mk()
    ranks = [mk(rank=r, world=world, split=True) for r in range(world)]
    try:
        assert all(c.split for c in ranks)
        for _ in range(2):
            single.step()
            for c in ranks:
                c.accumulate()
                c.synchronize()
            _sum_buffers(hip, ranks)
            for c in ranks:
                c.solve_update()
        s02 = 1.0
        cd1, cr1 = single.covariance(s02)
        parts = [c.covariance(s02) for c in ranks]
        cd2 = sum(p[0] for p in parts)
        cr2 = sum(p[1] for p in parts)
        rel = np.max(np.abs(cd2 - cd1) / np.abs(cd1))
        print(f"split covariance vs single ({world} ranks): diag(Cx) {rel:.2e} relative, correlations {np.max(np.abs(cr2 - cr1)):.2e}")
        # the C-ABI does not say which columns a rank owns: a rank without a subtree shows as one that
        # writes no camera-side variance (rank 0 always writes the top's)
        u_c = len(cd1) - 3 * ds.pack().n_tie
        print(f"split covariance: {sum(not np.any(p[0][:u_c] != 0) for p in parts)} of {world} ranks write no "
              f"camera-side variance; images per rank {[int(np.any(p[1] != 0, axis=(1, 2)).sum()) for p in parts]}")
        assert np.all(cd1 > 0) and rel <= 1e-8, rel
        np.testing.assert_allclose(cr2, cr1, rtol=0, atol=1e-9)
        # every entry written by exactly one rank: no image block or variance on two
        assert np.all(sum((p[0] != 0).astype(np.int32) for p in parts) <= 1)
        assert np.all(sum(np.any(p[1] != 0, axis=(1, 2)).astype(np.int32) for p in parts) <= 1)
    finally:
        single.close()
        for c in ranks:
            c.close()


def test_handoff_timeout_fails_safe(fba, scenes, monkeypatch):
    """A device hand-off timeout in the factorisation (every poll bounded, fba_chol.hip) must not leave a
    wrong iterate behind: with the poll bound forced down to one sleep (FBA_FLAG_SPINS at context
    creation: this context's bound, scal[SCAL_SPINS]) some wait of k_chol_flow / k_bwd_flow expires, the
    abort reaches every other wait, the step returns FBA_ERR_HIP and xhat is exactly as before it.  A
    context created beside it with the default bound is unaffected (the bound is per context), and the
    failed context, its bound restored (fba_set_spin_bound), then steps normally (the sync words are
    re-zeroed ahead of every factorisation) and matches the fresh context bit for bit."""
    folder = _scene(3, scenes)
    ds = fba.load_folder(folder)
    monkeypatch.setenv("FBA_FLAG_SPINS", "1")
    ctx = _ctx(fba, ds)
    monkeypatch.delenv("FBA_FLAG_SPINS")
    fresh = _ctx(fba, ds)
    try:
        x0 = ctx.get_xhat()
        with pytest.raises(fba.capi.FBAError) as ei:
            ctx.step()
        assert ei.value.code == 3 and "timeout" in str(ei.value), ei.value  # FBA_ERR_HIP
        assert np.array_equal(ctx.get_xhat(), x0)
        ctx.set_spin_bound(0)
        d, d_fresh = ctx.step(), fresh.step()
        assert d == d_fresh and np.array_equal(ctx.get_xhat(), fresh.get_xhat())
    finally:
        ctx.close()
        fresh.close()


def _sum_buffers(hip, ranks):
    """the all-reduce of the ranks' reduce buffers, on the host"""
    bufs = [c.reduce_buffer() for c in ranks]
    assert all(n == bufs[0][1] for _, n in bufs)
    total = np.zeros(bufs[0][1])
    for p, n in bufs:
        a = np.empty(n)
        assert hip.hipMemcpy(a.ctypes.data, p, n * 8, 2) == 0
        total += a
    for p, n in bufs:
        assert hip.hipMemcpy(p, total.ctypes.data, n * 8, 1) == 0


def test_subtree_split_abort_reaches_every_rank(fba, scenes):
    """Subtree split (config 3, two rank contexts on one GPU): a hand-off timeout inside rank 0's flow A
    (run in fba_accumulate) leaves its top-block contributions incomplete.  The abort travels in the
    reduce buffer (its last slot), so after the sum EVERY rank skips flow B and the update and returns
    FBA_ERR_HIP with xhat as before -- not only the rank that timed out.  With the bound restored, the
    next accumulations / solves of both ranks reassemble the single context's iterates: the first pass's
    deltasum shares add up to its deltasum, and after the second pass xhat agrees to 1e-9 per group and
    per element."""
    import ctypes
    folder = _scene(3, scenes)
    ds = fba.load_folder(folder)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    mk = lambda **kw: fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)  # noqa: E731
    single = mk()
    ranks = [mk(rank=r, world=2, split=True) for r in range(2)]
    try:
        assert all(c.split for c in ranks)
        x0 = [c.get_xhat() for c in ranks]
        ranks[0].set_spin_bound(1)
        for c in ranks:
            c.accumulate()
            c.synchronize()
        _sum_buffers(hip, ranks)
        for c, x in zip(ranks, x0):
            with pytest.raises(fba.capi.FBAError) as ei:
                c.solve_update()
            assert ei.value.code == 3, ei.value
            assert np.array_equal(c.get_xhat(), x)
        ranks[0].set_spin_bound(0)
        d_first = None
        for _ in range(2):
            d1 = single.step()
            d_first = d_first or d1
            for c in ranks:
                c.accumulate()
                c.synchronize()
            _sum_buffers(hip, ranks)
            parts = [c.solve_update() for c in ranks]
            assert abs(sum(parts) - d1) <= 1e-9 * d_first
        xr = sum(c.get_xhat(owned_only=True) for c in ranks)
        dsc = dist_scaling_of(__import__("fba_oracle").load_folder(folder))
        names = fba.xhat_names(ds)
        # (after one pass from the start, reduction-order rounding moves k1, the ill-conditioned radial
        # direction, by ~1e-9 of its group (8.5e-10 in round 4, 1.0e-9 in round 5); the second pass contracts
        # it, as in the two-pass test above)
        err = group_rel_err(xr, single.get_xhat(), names, dsc)
        assert max(err.values()) <= 1e-9, err
        err = elem_rel_err(xr, single.get_xhat(), names, dsc)
        assert max(err.values()) <= 1e-9, err
    finally:
        single.close()
        for c in ranks:
            c.close()


def test_subtree_split_pivot_failure_reaches_every_rank(fba, scenes):
    """Subtree split (config 3, two rank contexts on one GPU): a non-positive pivot inside rank 0's flow A
    (rank 0's image EOPs set to NaN, so its subtree blocks are NaN: the potrf's `d > 0` test fails) is
    reported through the reduce buffer (the pivot-failure slot after the abort flag), so EVERY rank
    returns FBA_ERR_NOT_SPD for that step -- the ranks agree that it failed.  With xhat restored, the next
    passes of both ranks reassemble the single context's iterates."""
    import ctypes
    folder = _scene(3, scenes)
    ds = fba.load_folder(folder)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    mk = lambda **kw: fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)  # noqa: E731
    single = mk()
    ranks = [mk(rank=r, world=2, split=True) for r in range(2)]
    try:
        assert all(c.split for c in ranks)
        x0 = [c.get_xhat() for c in ranks]
        bad = x0[0].copy()
        bad[:6 * ds.numImg] = np.nan
        ranks[0].set_xhat(bad)
        for c in ranks:
            c.accumulate()
            c.synchronize()
        _sum_buffers(hip, ranks)
        for c in ranks:
            with pytest.raises(fba.capi.FBAError) as ei:
                c.solve_update()
            assert ei.value.code == 4 and "not positive definite" in str(ei.value), ei.value
        for c, x in zip(ranks, x0):
            c.set_xhat(x)
        for _ in range(2):
            d1 = single.step()
            for c in ranks:
                c.accumulate()
                c.synchronize()
            _sum_buffers(hip, ranks)
            parts = [c.solve_update() for c in ranks]
            assert abs(sum(parts) - d1) <= 1e-9 * d1
        xr = sum(c.get_xhat(owned_only=True) for c in ranks)
        dsc = dist_scaling_of(__import__("fba_oracle").load_folder(folder))
        names = fba.xhat_names(ds)
        err = elem_rel_err(xr, single.get_xhat(), names, dsc)
        assert max(err.values()) <= 1e-9, err
    finally:
        single.close()
        for c in ranks:
            c.close()


def test_subtree_split_guards(fba, scenes, tmp_path, monkeypatch):
    """The split's contract at its edges: one solve per accumulation (a second fba_solve_update of the same
    accumulation is refused with FBA_ERR_ARG instead of running flow B on spent tickets); the per-level
    backward solve (FBA_BWD_LEVELS=1), which knows neither the ranks' column ownership nor the split's
    border scales, is refused at creation (FBA_ERR_UNSUPPORTED) like the per-level factorisation; and a
    split request on a block pattern that cannot be cut (12 images: one block of image rows) falls back
    to the replicated solve, which fba_solve_mode / Context.split report."""
    import ctypes
    folder = _scene(3, scenes)
    ds = fba.load_folder(folder)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    mk = lambda d, **kw: fba.capi.Context(d.pack(), fba.capi.make_settings(d.settings), **kw)  # noqa: E731
    ranks = [mk(ds, rank=r, world=2, split=True) for r in range(2)]
    try:
        for c in ranks:
            c.accumulate()
            c.synchronize()
        _sum_buffers(hip, ranks)
        for c in ranks:
            c.solve_update()
        with pytest.raises(fba.capi.FBAError) as ei:
            ranks[0].solve_update()
        assert ei.value.code == 1 and "one fba_solve_update per fba_accumulate" in str(ei.value)
    finally:
        for c in ranks:
            c.close()
    monkeypatch.setenv("FBA_BWD_LEVELS", "1")
    with pytest.raises(fba.capi.FBAError) as ei:
        mk(ds, rank=0, world=2, split=True)
    assert ei.value.code == 5, ei.value
    monkeypatch.delenv("FBA_BWD_LEVELS")
    from fba_amd import synth
    small = fba.load_folder(synth.write_folder(synth.generate(12, 240, seed=17), str(tmp_path / "s12")))
    c = mk(small, rank=0, world=2, split=True)
    try:
        assert not c.split
    finally:
        c.close()


# Partial Estimate_* flag sets (tests/flag_masks.py) at the size where the block Cholesky has many blocks.
# MASKED_CONTROL_SEED: chosen on the CPU so that exact restatements in oracle/fba_cpu.c agree far below the
# bars -- without a border "kkt" and "chol" are the same dense Cholesky (identical results), so the
# independent pair is "kkt" against "sparse" (the block-sparse Cholesky on the device's block pattern) and
# "kkt" on 3 threads: <= 1.2e-12 per element, sigma0^2 <= 3.0e-15, 9 iterations each (required: 5e-11);
# and so that the stop rule is not decided by rounding: the last two deltasums are 7.2e-6 and 4.9e-7 around
# Threshold_Value 1e-6 (seed 32's ninth is 1.08e-6).
# Config 3 under c_k_only: "kkt" / "chol" / "sparse" agree <= 2.5e-12 per element, 6 iterations each.
MASKED_CONTROL_SEED = 33


def _masked_scene(kind, root):
    """"control": 200 images x 5,000 points, 40 of them control points, under mix_a (Omega, Zc, yp, radial
    off: two zero rows with a unit diagonal in every image's 6 x 6 block, so in every 128-row block of
    k_chol_flow, and a 4-of-10 camera block).  "config3": config 3 (free network: the inner-constraint
    border) under c_k_only (xp, yp, decentering off)."""
    import flag_masks as fm
    from fba_amd import synth
    folder = os.path.join(root, "masked_" + kind)
    if not os.path.exists(os.path.join(folder, ".done")):
        if kind == "control":
            sc = synth.generate(200, 5000, seed=MASKED_CONTROL_SEED, n_control=40)
            synth.write_folder(sc, folder, cfg_overrides=fm.MASKS["mix_a"])
        else:
            n_img, n_tie = synth.CONFIGS[3]
            synth.write_folder(synth.generate(n_img, n_tie, seed=1003), folder, cfg_overrides=fm.MASKS["c_k_only"])
        open(os.path.join(folder, ".done"), "w").close()
    return folder


@pytest.mark.parametrize("kind", ["control", "config3"])
def test_masked_adjust_matches_oracle(fba, fbo, oracle, scenes, kind):
    """The whole adjustment under a partial mask at 200 images x 5,000 points against the C oracle's direct
    solve, at _check_adjust's bars: a control-point scene under mix_a and config 3 (the border) under the
    camera mask c_k_only."""
    folder = _masked_scene(kind, scenes)
    od = oracle.load_folder(folder)
    assert oracle.counts(od.settings) == ((4, 4) if kind == "control" else (6, 6))
    _check_adjust(fba, fbo, oracle, folder)


@pytest.mark.parametrize("kind", ["control", "config3"])
def test_masked_subtree_split_two_ranks_match_single_context(fba, scenes, kind):
    """test_subtree_split_two_ranks_match_single_context's body on the two masked scenes, at its own bars
    (1e-10 per group, 1e-9 per element, the deltasum shares), with the split honoured on both ranks
    (fba_solve_mode): the unit rows' `once` / `rown` handling of k_border_rhs under the split."""
    _split_ranks_match_single_context(fba, _masked_scene(kind, scenes), 2, 1e-10, honoured=True)


def test_masked_subtree_split_covariance_matches_single_context(fba, scenes):
    """test_subtree_split_covariance_matches_single_context's body on config 3 under c_k_only: the ranks'
    (6 + 6)^2 correlation blocks and u-long variances sum to the single context's."""
    _split_covariance_matches_single_context(fba, _masked_scene("config3", scenes), 2)
