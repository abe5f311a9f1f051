"""GPU: variance component estimation over observation groups -- fba_vce (csrc/fba_vce.hip) against the dense numpy
restatement (tests/vce_ref.py), its redundancy sum, its self-consistency, its shapes and contract, and
adjust(..., vce=...) / fba_cli.py main --vce end to end.

Scenes (vce_ref.SCENES): synth.generate(noise=0) at nk 2, fish-eye, plus planted noise per group.  Conditions on the
inputs, asserted on the restatement alone (vce_ref.restated): every planted sigma recovered within 15 %, no deltasum
within 1.25x of Threshold_Value.  The device is compared against the restatement, never against the truth.

Bars, none from a device run:
  round k (0-based), R, T and sigma2 of every group, relative: (k + 1) x max(1e-8, 20 x the restatement's own spread on
      that quantity, its explicit inverse against its LU / symmetric solve) -- test_gpu_reliability.py's rule and floor
      for r; the errors of round k feed the weights of round k + 1, hence the factor
  component: the product of the rounds' sigma2, so the sum of their bars
  xhat and sigma0^2: test_gpu_weights.py's -- per group and element max(1e-9, 20 x the restatement's spread),
      sigma0^2 at max(1e-9, 20 x its spread)
  redundancy sum: n x 1e-8
  the sums against numpy on the device's own reliability outputs (shapes): 1e-11 relative to sum |terms| -- another
      order of at most 1536 fp64 additions, 1536 x 1.1e-16 = 1.7e-13, and r, t recomputed from rounded outputs
  everything else is bitwise.
Measured on the device: DESIGN.md 6i, profiles/vce_gpu_errors.log (the "vce ..." prints of this module).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import vce_ref as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("vce_gpu")


def _ctx(fba, ds, **kw):
    return fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)


def _vce(fba, ds, group, ng, ctx_kw=None, **opts):
    """a fresh context through fba_vce: (result dict, xhat, v, stats, weights)"""
    ctx = _ctx(fba, ds, **(ctx_kw or {}))
    try:
        out = ctx.vce(group, ng, **opts)
        v, _, st = ctx.residuals()
        return out, ctx.get_xhat(), v, st, ctx.get_weights()
    finally:
        ctx.close()


def _dof(ds, ctx_u, n_prior=0):
    return 2 * len(ds.pack().img) + n_prior - ctx_u + (7 if int(ds.settings["Inner_Constraints"]) else 0)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_matches_restatement(fba, oracle, root, name):
    from test_gpu_block_shapes import _errors, _fmt
    s = vr.restated(fba, oracle, root, name)
    a, b, ng = s.a, s.b, s.n_groups
    u = len(a.xhat)
    out, xhat, v, st, wts = _vce(fba, s.ds, s.group, ng)
    assert out["rounds"] == a.rounds and out["converged"] == a.converged and out["iterations"] == len(a.deltasum)
    assert out["status"][: ng + 1].tolist() == a.status.tolist() and out["status"][ng + 1] == vr.EMPTY
    tab = out["table"]
    assert tab.shape == (a.rounds, ng + 2, 4)
    n = s.od.n
    cbar = 0.0
    failed = []
    for k in range(a.rounds):
        np.testing.assert_array_equal(tab[k, : ng + 1, 2], a.table[k, :, 2])
        e_sum = tab[k, :, 0].sum() - _dof(s.ds, u)
        line = [f"vce {name} round {k + 1}: sum R - (n-u+d) {e_sum:.2e} (error/bar, restatement's own spread)"]
        assert abs(e_sum) <= n * 1e-8
        for q, qn in ((0, "R"), (1, "T"), (3, "sigma2")):
            ref = a.table[k, :ng, q]
            err = np.abs(tab[k, :ng, q] - ref) / np.abs(ref)
            spread = np.abs(b.table[k, :ng, q] - ref) / np.abs(ref)
            bar = (k + 1) * np.maximum(1e-8, 20 * spread)
            line.append(f"{qn} {err.max():.1e}/{bar[np.argmax(err / bar)]:.1e} ({spread.max():.1e})")
            if not (err <= bar).all():
                failed.append((k, qn, err.tolist(), bar.tolist()))
            if q == 3:
                cbar += bar.max()
        print(" ".join(line))
    e_c = np.abs(out["component"][:ng] - a.component) / a.component
    spread = _errors(b.xhat, a.xhat, a)
    err = _errors(xhat, a.xhat, a)
    s_s02 = abs(b.sigma02 - a.sigma02) / a.sigma02
    e_s02 = abs(st[3] - a.sigma02) / a.sigma02
    print(f"vce {name}: rounds {out['rounds']} component error {e_c.max():.1e} (bar {cbar:.1e}) sigma02 {e_s02:.1e}/{s_s02:.1e} "
          + _fmt(err, spread))
    assert not failed, failed
    assert (e_c <= cbar).all()
    assert (out["component"][ng:] == 1.0).all()
    bad = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
    assert not bad, bad
    assert e_s02 <= max(1e-9, 20 * s_s02)
    np.testing.assert_allclose(wts, 1.0 / np.concatenate([out["component"], [1.0]])[np.where(s.group < 0, ng + 2, s.group)],
                               rtol=1e-13)


# ---- 2. the redundancy sum with priors ---------------------------------------------------------------------------------
def test_redundancy_sum_with_priors(fba, oracle, root):
    """scene C plus priors on the first image's six EOPs: the priors' entry closes the sum in every round"""
    s = vr.restated(fba, oracle, root, "C")
    ng = s.n_groups
    x0 = oracle.buildxhat(s.od)[0]
    u = len(x0)
    pri = (np.arange(6), x0[:6], np.array([1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3]))
    out, _, _, st, _ = _vce(fba, s.ds, s.group, ng, ctx_kw=dict(priors=pri))
    tab = out["table"]
    assert out["status"][ng + 1] == vr.OK and (tab[:, ng + 1, 2] == 6).all()
    for k in range(out["rounds"]):
        e_sum = tab[k, :, 0].sum() - _dof(s.ds, u, 6)
        print(f"vce C+priors round {k + 1}: sum R - (n+n_prior-u+d) {e_sum:.2e}, priors R {tab[k, ng + 1, 0]:.4f} T {tab[k, ng + 1, 1]:.4f}")
        assert abs(e_sum) <= s.od.n * 1e-8
        assert 0.0 < tab[k, ng + 1, 0] < 6.0 and tab[k, ng + 1, 1] >= 0.0
    assert st[5] == 2 * len(s.ds.pack().img) + 6 - u


# ---- 3. self-consistency, no oracle ------------------------------------------------------------------------------------
def test_self_consistency(fba, oracle, root):
    s = vr.restated(fba, oracle, root, "A")
    ng, grp = s.n_groups, s.group
    c1, c2, c3 = _ctx(fba, s.ds), _ctx(fba, s.ds), _ctx(fba, s.ds)
    try:
        out = c1.vce(grp, ng)
        assert out["converged"]
        x1, w1 = c1.get_xhat(), c1.get_weights()
        np.testing.assert_allclose(w1, 1.0 / out["component"][grp], rtol=1e-13)
        # a fresh context given those weights and adjusted: v, r and the group ratios are the datum's invariants
        # (scene A is a free network: its xhat depends on the path through the inner constraints)
        c2.set_weights(w1)
        c2.adjust()
        v2, _, st2 = c2.residuals()
        _, _, red, _ = c2.reliability(st2[3], corr=False)
        pv2 = w1 * (v2 / vr.MEAS_STD) ** 2
        ratio = np.array([pv2[grp == g].sum() / red[grp == g].sum() for g in range(ng)])
        print(f"vce self-consistency: sum p v^2 / sum r per group {ratio}")
        assert (np.abs(ratio - 1.0) <= 1e-3).all()  # tol: the converged round's sigma2, no rescale followed it
        # bitwise: the re-weighted context and a fresh one given its weights and its xhat take the same step and
        # report the same reliability
        c3.set_weights(w1)
        c3.set_xhat(x1)
        c1.step()
        c3.step()
        np.testing.assert_array_equal(c1.get_xhat(), c3.get_xhat())
        ra, rb = c1.residuals(), c3.residuals()
        for p, q in zip(ra, rb):
            np.testing.assert_array_equal(p, q)
        for p, q in zip(c1.reliability(ra[2][3]), c3.reliability(rb[2][3])):
            np.testing.assert_array_equal(p, q)
    finally:
        for c in (c1, c2, c3):
            c.close()


def test_fresh_weighted_context_reaches_the_same_solution(fba, oracle, root):
    """scene C (its datum is fixed by control points, so the solution does not depend on the path): a fresh context
    given fba_vce's weights through fba_set_weights and adjusted gives its xhat within the weighted solver spread"""
    from test_gpu_block_shapes import _errors, _fmt
    s = vr.restated(fba, oracle, root, "C")
    out, x1, _, _, w1 = _vce(fba, s.ds, s.group, s.n_groups)
    ctx = _ctx(fba, s.ds)
    try:
        ctx.set_weights(w1)
        ctx.adjust()
        x2 = ctx.get_xhat()
    finally:
        ctx.close()
    spread, err = _errors(s.b.xhat, s.a.xhat, s.a), _errors(x2, x1, s.a)
    print("vce fresh weighted context (error/restatement's own spread): " + _fmt(err, spread))
    bad = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
    assert not bad, bad


# ---- 4. shapes ---------------------------------------------------------------------------------------------------------
def _numpy_round(fba, ds, group, ng):
    """the first round's sums in numpy from a twin context's own reliability outputs"""
    ctx = _ctx(fba, ds)
    try:
        ctx.adjust()
        v, _, st = ctx.residuals()
        _, _, red, _ = ctx.reliability(st[3], corr=False)
    finally:
        ctx.close()
    t = (v / vr.MEAS_STD) ** 2
    mag = vr.group_sums(group, np.abs(red), t, ng)
    return vr.group_sums(group, red, t, ng), mag


SHAPES = {
    "one-group": dict(scene="A", ng=1, group=lambda n, tie: np.zeros(n, np.int32)),
    "256-groups": dict(scene="A", ng=256, group=lambda n, tie: (np.arange(n) // 6).astype(np.int32), opts=dict(min_redundancy=5.0)),
    "half-ungrouped": dict(scene="A", ng=2, group=lambda n, tie: np.where(np.arange(n) % 4 < 2, -1, np.arange(n) % 2).astype(np.int32)),
    # group 2: every row of the first ten tie points (60 observations: the device orders its observations by point)
    "absent-from-blocks": dict(scene="A", ng=3, group=lambda n, tie: np.where(np.repeat(tie, 2) < 10, 2, np.arange(n) % 2).astype(np.int32)),
    "multiple-of-256": dict(scene="A256", ng=2, group=lambda n, tie: (np.arange(n) % 2).astype(np.int32)),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(fba, root, shape):
    """the group sums of one round against numpy on the device's own r and v, the statuses from those sums by
    vce_ref.group_estimate, and a full run that ends"""
    from fba_amd import synth
    sp = SHAPES[shape]
    if sp["scene"] == "A256":  # scene A with 128 points: 768 observations, three full blocks of 256
        folder = os.path.join(str(root), "vce_A256")
        if not os.path.isdir(folder):
            vr.SCENES["A256"] = dict(vr.SCENES["A"], gen=dict(vr.SCENES["A"]["gen"], n_tie=128))
            folder = vr.scene_folder(synth, root, "A256")
    else:
        folder = vr.scene_folder(synth, root, sp["scene"])
    ds = fba.load_folder(folder)
    n = 2 * len(ds.pack().img)
    assert shape != "multiple-of-256" or n == 2 * 768
    group, ng, opts = sp["group"](n, np.asarray(ds.pack().tie)), sp["ng"], sp.get("opts", {})
    assert group.max() < ng
    ref, mag = _numpy_round(fba, ds, group, ng)
    out, _, _, _, _ = _vce(fba, ds, group, ng, max_rounds=1, **opts)
    tab = out["table"][0]
    np.testing.assert_array_equal(tab[: ng + 1, 2], ref[:, 2])
    err = np.abs(tab[: ng + 1, :2] - ref[:, :2]) / np.maximum(mag[:, :2], 1e-300)
    print(f"vce shape {shape}: n={n} groups={ng} max sum error {err.max():.1e} (bar 1e-11)")
    assert (err <= 1e-11).all()
    est = [vr.group_estimate(*ref[g], **{k: v for k, v in opts.items() if k in ("min_redundancy", "clip")}) for g in range(ng)]
    assert out["status"][:ng].tolist() == [e[2] for e in est]
    np.testing.assert_allclose(tab[:ng, 3], [e[0] for e in est], rtol=1e-10)
    assert out["rounds"] == 1 and (out["component"] == 1.0).all()
    if shape == "256-groups":
        assert (out["status"][:ng] == vr.WEAK).sum() > ng // 2 and (out["status"][:ng] == vr.EMPTY).sum() == ng - n // 6
    full, xhat, _, st, _ = _vce(fba, ds, group, ng, **opts)
    assert 1 <= full["rounds"] <= 10 and np.isfinite(xhat).all() and np.isfinite(st[3])
    assert abs(full["table"][-1, :, 0].sum() - out["table"][0, :, 0].sum()) <= n * 1e-8


# ---- 5. contracts, bitwise ---------------------------------------------------------------------------------------------
def test_two_fresh_contexts_are_bitwise_equal(fba, oracle, root):
    s = vr.restated(fba, oracle, root, "C")
    a = _vce(fba, s.ds, s.group, s.n_groups)
    b = _vce(fba, s.ds, s.group, s.n_groups)
    for k in ("component", "table", "status"):
        np.testing.assert_array_equal(a[0][k], b[0][k])
    assert (a[0]["rounds"], a[0]["iterations"], a[0]["converged"]) == (b[0]["rounds"], b[0]["iterations"], b[0]["converged"])
    for p, q in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(p, q)


def test_one_round_leaves_the_weighting_alone(fba, oracle, root):
    s = vr.restated(fba, oracle, root, "A")
    c1, c2 = _ctx(fba, s.ds), _ctx(fba, s.ds)
    try:
        out = c1.vce(s.group, s.n_groups, max_rounds=1)
        it, _ = c2.adjust()
        c2.step()
        assert out["rounds"] == 1 and out["iterations"] == it + 1 and not out["converged"]
        np.testing.assert_array_equal(c1.get_xhat(), c2.get_xhat())
        np.testing.assert_array_equal(c1.get_weights(), np.ones(s.od.n))  # no weights were switched on
        for p, q in zip(c1.residuals(), c2.residuals()):
            np.testing.assert_array_equal(p, q)
        assert c1.step() == c2.step()
        np.testing.assert_array_equal(c1.get_xhat(), c2.get_xhat())
    finally:
        c1.close()
        c2.close()


@pytest.mark.parametrize("case", ["world2", "loss", "damping", "pending", "bad-id", "bad-option"])
def test_refusals_leave_the_context_untouched(fba, oracle, root, case):
    s = vr.restated(fba, oracle, root, "A")
    kw = dict(rank=0, world=2) if case == "world2" else {}
    c1, c2 = _ctx(fba, s.ds, **kw), _ctx(fba, s.ds, **kw)

    def step(c, refuse):
        group, ng, opts, code = s.group, s.n_groups, {}, 5
        if case == "bad-id":
            group, code = np.where(np.arange(s.od.n) == 7, ng, s.group), 1
        if case == "bad-option":
            opts, code = dict(clip=0.5), 1
        if case == "pending":
            code = 1
        c.accumulate()
        if case == "world2" and not refuse:
            return 0.0  # (one rank of two: its share of the normal equations alone is not solved here)
        if case == "pending":
            c.solve_update_async()
        if refuse:
            with pytest.raises(fba.capi.FBAError) as e:
                c.vce(group, ng, **opts)
            assert e.value.code == code and "fba_vce" in str(e.value)
            if case == "world2":
                return 0.0
        return c.solve_finish() if case == "pending" else c.solve_update()

    try:
        for c in (c1, c2):
            if case == "loss":
                c.step()
                c.set_loss("huber")
            if case == "damping":
                c.set_damping(1e-3)
        d1, d2 = step(c1, True), step(c2, False)
        assert d1 == d2
        np.testing.assert_array_equal(c1.get_xhat(case == "world2"), c2.get_xhat(case == "world2"))
        d1, d2 = step(c1, False), step(c2, False)
        assert d1 == d2
        np.testing.assert_array_equal(c1.get_xhat(case == "world2"), c2.get_xhat(case == "world2"))
    finally:
        c1.close()
        c2.close()


def test_allocations_return(fba, oracle, root):
    s = vr.restated(fba, oracle, root, "D")
    before = fba.capi.live_allocations()
    ctx = _ctx(fba, s.ds)
    ctx.set_timing(True)
    out = ctx.vce(s.group, s.n_groups)
    ms = ctx.timings()
    assert out["rounds"] >= 1 and ms[7] > 0.0 and not ms[:7].any()
    assert fba.capi.live_allocations() > before
    ctx.close()
    assert fba.capi.live_allocations() == before


# ---- 6. end to end -----------------------------------------------------------------------------------------------------
def _flagged(path):
    with open(path) as fh:
        return {i for i, ln in enumerate(fh) if ln.rstrip("\n").split("\t")[-1] == "*"}


def test_adjust_vce_camera_xy(fba, oracle, root, tmp_path):
    from fba_amd import report
    s = vr.restated(fba, oracle, root, "C")
    res = fba.adjust(s.ds, vce="camera_xy", reliability=True)
    ng = s.n_groups
    assert res.vce_names == ["cam0.x", "cam0.y", "cam1.x", "cam1.y", "(no group)", "(priors)"]
    out, xhat, v, st, wts = _vce(fba, s.ds, s.group, ng)
    np.testing.assert_array_equal(res.vce_component, out["component"])
    np.testing.assert_array_equal(res.vce_table, out["table"])
    np.testing.assert_array_equal(res.xhat, xhat)
    np.testing.assert_array_equal(res.weights, wts)
    assert res.sigma02 == st[3] and res.vce_rounds == out["rounds"] and res.iterations == out["iterations"]
    np.testing.assert_allclose(res.vce_sigma[:ng], np.sqrt(out["component"][:ng]) * vr.MEAS_STD, rtol=1e-15)
    assert np.isnan(res.vce_sigma[ng:]).all() and res.redundancy is not None
    path = os.path.join(str(tmp_path), "c.vce")
    report.write_vce(path, res)
    names, rows, sr, comp, sig, words, hist = report.read_vce(path)
    assert names == res.vce_names and words == [report.VCE_STATUS[i] for i in res.vce_status]
    np.testing.assert_allclose(comp, res.vce_component, rtol=1e-14)
    np.testing.assert_allclose(hist, res.vce_table, rtol=1e-14)
    np.testing.assert_array_equal(rows, res.vce_table[-1, :, 2])
    with pytest.raises(ValueError):
        fba.adjust(s.ds, vce="xy", robust="huber")
    with pytest.raises(ValueError):
        fba.adjust(s.ds, vce="rows")


def test_cli_main_vce_xy(fba, oracle, root):
    """fba_cli.py main <folder> --vce=xy --reliability on scene A: the .vce table parses back to the restatement's
    rounds, and the .rel table flags another set of measurements than the unweighted run's"""
    from fba_amd import report
    s = vr.restated(fba, oracle, root, "A")
    rel, vce = os.path.join(s.folder, "synth.rel"), os.path.join(s.folder, "synth.vce")
    assert fba.main(s.folder, reliability=True) == 0
    plain = _flagged(rel)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fba_cli.py"), "main", s.folder, "--vce=xy", "--reliability"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    weighted = _flagged(rel)
    names, rows, sr, comp, sig, words, hist = report.read_vce(vce)
    print(f"vce cli: flagged measurements {len(plain)} unweighted, {len(weighted)} re-weighted, {len(plain & weighted)} in both")
    assert names == ["x", "y", "(no group)", "(priors)"] and words == ["OK", "OK", "EMPTY", "EMPTY"]
    assert hist.shape == (s.a.rounds, 4, 4) and rows.tolist() == [720, 720, 0, 0]
    np.testing.assert_allclose(comp[:2], s.a.component, rtol=1e-6)
    np.testing.assert_allclose(sig[:2], np.sqrt(s.a.component) * vr.MEAS_STD, rtol=1e-6)
    assert plain != weighted
