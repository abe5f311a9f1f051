"""GPU: Baarda data snooping -- fba_snoop (csrc/fba_snoop.hip) against the dense numpy restatement
(tests/snoop_ref.py) round by round, its weights, its shapes and contracts, and adjust(..., snoop=...) /
fba_cli.py main --snoop end to end.

Scenes (snoop_ref.SCENES): vce_ref's geometry with synth.generate's noise at Meas_std and planted blunders of 10 - 20
sigma.  Conditions on the inputs, asserted on the restatement alone (snoop_ref.restated): it converges, excludes exactly
the planted points and re-admits exactly the pre-excluded ones, no W or W~ of any round lies within 2 % of crit, no
deltasum within 1.25x of Threshold_Value.  The device is compared against the restatement, never against the truth.

A round's statistics are read by running a fresh context with max_rounds = k: the picks of the last allowed round are
found and not applied, so `stat` is round k's W and `excluded` the state before it.

Bars, none from a device run:
  the eliminated and re-admitted sets, the rounds and the iteration counts: equal
  W of an active point: test_gpu_reliability.py's bar on w -- |dW| <= W bar_r / (2 r) + 10 vtol max W, r the redundancy
      number of the row that gives W, bar_r = max(1e-8, 20 x the restatement's two-route spread on r in that round),
      vtol = max(1e-9, 20 x its spread on sigma0^2)
  W~ of an excluded point: W~ max(1e-8, 20 x the restatement's two-route relative spread on W~ in that round) + the
      same residual term
  xhat and sigma0^2 (scene C, fixed datum): test_gpu_weights.py's -- per group and element max(1e-9, 20 x the
      restatement's spread), sigma0^2 at max(1e-9, 20 x its spread)
  the weights: fl(fl(1e-6 s0)^2) on the excluded rows -- exactly that, which is 1e-12 s0^2 to the rounding of 1e-6, of
      the product and of its square, 4 x 2^-52 -- and bitwise the starting weight elsewhere
  W against the device's own reliability outputs (shapes): 4 ulp -- the same q and v through the same formula
  everything else is bitwise.
Measured on the device: DESIGN.md 6j, profiles/snoop_gpu_errors.log (the "snoop ..." prints of this module).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import snoop_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW = np.float64(1e-6) ** 2  # an excluded row's weight at s0 = 1


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("snoop_gpu")


def _ctx(fba, ds, **kw):
    return fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)


def _pre(n, rows):
    ex = np.zeros(n, dtype=np.uint8)
    ex[list(rows)] = 1
    return ex


def _snoop(fba, ds, pre=(), weights=None, **opts):
    """a fresh context through fba_snoop: (result dict, xhat, v, stats, weights)"""
    ctx = _ctx(fba, ds)
    try:
        if weights is not None:
            ctx.set_weights(weights)
        out = ctx.snoop(_pre(len(ds.pack().img), pre) if len(pre) else None, **opts)
        v, _, st = ctx.residuals()
        return out, ctx.get_xhat(), v, st, ctx.get_weights()
    finally:
        ctx.close()


def _shape_folder(synth, root, name, n_tie):
    sr.SCENES[name] = dict(gen=dict(sr.SCENES["A"]["gen"], n_tie=n_tie), plant="six")
    return sr.scene_folder(synth, root, name)


# ---- 1. against the restatement, round by round ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C", "P"])
def test_matches_restatement(fba, oracle, root, name):
    from test_gpu_block_shapes import _errors, _fmt
    s = sr.restated(fba, oracle, root, name)
    a, b = s.a, s.b
    n = s.od.n // 2
    vtol = max(1e-9, 20 * abs(b.sigma02 - a.sigma02) / a.sigma02)
    full, xhat, v, st, wts = _snoop(fba, s.ds, s.pre)
    assert full["rounds"] == a.rounds and full["converged"] and full["iterations"] == len(a.deltasum) and full["status_bits"] == 0
    np.testing.assert_array_equal(full["table"][:, :3], a.table[:, :3])
    np.testing.assert_array_equal(full["excluded"], a.state[-1])
    failed = []
    for k in range(a.rounds):
        out = full if k == a.rounds - 1 else _snoop(fba, s.ds, s.pre, max_rounds=k + 1)[0]
        assert out["rounds"] == k + 1 and out["iterations"] == sum(a.iters[: k + 1])
        # the state before round k: the sets every earlier round eliminated and re-admitted
        np.testing.assert_array_equal(out["excluded"], a.before[k] if k < a.rounds - 1 else a.state[-1])
        assert out["table"][k, :2].tolist() == [len(a.picks[k]), len(a.backs[k])]
        ex = a.before[k] == sr.EXCLUDED
        W, ref = out["stat"], a.W[k]
        err = np.abs(W - ref)
        own = np.abs(b.W[k] - ref)
        bar_r = max(1e-8, 20 * float(np.abs(b.r[k] - a.r[k])[~ex].max()))
        resid = 10 * vtol * ref.max()
        bar = np.where(ex, 0.0, ref * bar_r / (2 * a.r[k])) + resid
        line = f"snoop {name} round {k + 1}: W error/bar {err[~ex].max():.1e}/{bar[~ex][np.argmax(err[~ex] / bar[~ex])]:.1e} (restatement's own spread {own[~ex].max():.1e})"
        if ex.any():
            rel = max(1e-8, 20 * float((own[ex] / ref[ex]).max()))
            bar[ex] = ref[ex] * rel + resid
            line += f" W~ error/bar {err[ex].max():.1e}/{bar[ex][np.argmax(err[ex] / bar[ex])]:.1e} ({own[ex].max():.1e})"
        print(line + f" largest active W {out['table'][k, 3]:.6f} ({a.table[k, 3]:.6f})")
        if not (err <= bar).all():
            failed.append((k, int(np.argmax(err / bar)), float(err.max())))
        assert abs(out["table"][k, 3] - a.table[k, 3]) <= bar[~ex].max()
    # the leave-one-out identity (a figure, no bar): a blunder's W while active against its W~ once excluded
    first = {int(r): (k, a.W[k][r]) for k in range(a.rounds) for r in a.picks[k]}
    for r, (k, w) in sorted(first.items()):
        print(f"snoop {name} leave-one-out: PHO row {r} W {w:.4f} in round {k + 1}, W~ {full['stat'][r]:.4f} at the end "
              f"(restatement {a.W[-1][r]:.4f}), nonlinear difference {abs(full['stat'][r] - w) / w:.1e}")
    spread, err = _errors(b.xhat, a.xhat, a), _errors(xhat, a.xhat, a)
    s_s02 = abs(b.sigma02 - a.sigma02) / a.sigma02
    e_s02 = abs(st[3] - a.sigma02) / a.sigma02
    print(f"snoop {name}: rounds {full['rounds']} sigma02 {e_s02:.1e}/{s_s02:.1e} " + _fmt(err, spread))
    assert not failed, failed
    if name == "C":  # a fixed datum: the solution does not depend on the path
        bad = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
        assert not bad, bad
        assert e_s02 <= max(1e-9, 20 * s_s02)
    # the weights: 1e-12 on the excluded rows, bitwise the starting weight on every other, the re-admitted included
    np.testing.assert_array_equal(wts, np.where(np.repeat(a.state[-1] == sr.EXCLUDED, 2), LOW, 1.0))
    np.testing.assert_array_equal(wts, a.wt)


def test_user_weights_are_restored(fba, oracle, root):
    """scene P under user weights (squares, so their sqrt weights are exact): the excluded rows hold (1e-6 sqrt(w))^2 --
    the one product and its square --, every other row its weight bit for bit, the re-admitted rows included"""
    s = sr.restated(fba, oracle, root, "P")
    n = s.od.n
    w0 = np.array([1.0, 0.25, 4.0, 0.5625])[np.arange(n) % 4]
    out, _, _, _, wts = _snoop(fba, s.ds, s.pre, weights=w0)
    ex = np.repeat(out["excluded"] == 1, 2)
    assert ex.any() and (out["excluded"] == 2).any()
    np.testing.assert_array_equal(wts[~ex], w0[~ex])
    np.testing.assert_array_equal(wts[ex], (np.float64(1e-6) * np.sqrt(w0[ex])) ** 2)
    np.testing.assert_allclose(wts[ex], 1e-12 * w0[ex], rtol=4 * 2.0 ** -52)


# ---- 2. shapes: the device against its own reliability outputs and the host's selection -------------------------------
SHAPES = {"wide-image": 240, "three-blocks": 128}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(fba, root, shape):
    """wide-image: an image with 200 points and more, over three passes of the 64 lanes; three-blocks: 768
    observations, three full blocks of 256.  W of round 1 against max |w| of fba_reliability on a twin context, the
    round's picks against fba_snoop_host on that W, and a full run that ends with exactly those blunders out"""
    from fba_amd import synth
    folder, rows, _ = _shape_folder(synth, root, "S" + shape, SHAPES[shape])
    ds = fba.load_folder(folder)
    pk = ds.pack()
    n = len(pk.img)
    per_img = np.bincount(np.asarray(pk.img))
    assert (shape == "wide-image" and per_img.max() >= 200) or (shape == "three-blocks" and n == 768)
    ctx = _ctx(fba, ds)
    try:
        ctx.adjust()
        _, _, st = ctx.residuals()
        _, _, _, wst = ctx.reliability(st[3], corr=False)
    finally:
        ctx.close()
    Wref = np.abs(wst).reshape(-1, 2).max(axis=1)
    one = _snoop(fba, ds, max_rounds=1, max_share=1.0)[0]
    err = np.abs(one["stat"] - Wref) / np.maximum(Wref, 1e-300)
    print(f"snoop shape {shape}: n={n} largest image {per_img.max()} W against the reliability outputs {err.max():.1e} (bar 8.9e-16)")
    assert (err <= 4 * 2.0 ** -52).all()
    assert not one["excluded"].any() and not one["converged"]
    pick, back, bits = fba.capi.snoop_host(one["stat"], np.zeros(n, np.uint8), np.asarray(pk.tie), np.asarray(pk.img),
                                           n_tie=pk.n_tie, n_img=pk.n_img, max_share=1.0)
    assert pick.any() and not back.any() and bits == 0 and one["table"][0, 0] == pick.sum()
    two = _snoop(fba, ds, max_rounds=2, max_share=1.0)[0]
    np.testing.assert_array_equal(two["excluded"], pick.astype(np.uint8))
    full = _snoop(fba, ds, max_share=1.0)[0]
    assert full["converged"] and set(rows) <= set(np.nonzero(full["excluded"] == 1)[0])


def test_no_candidates_changes_nothing(fba, oracle, root):
    """scene N: one round, converged, and the context is bitwise the one fba_adjust leaves"""
    s = sr.restated(fba, oracle, root, "N")
    c1, c2 = _ctx(fba, s.ds), _ctx(fba, s.ds)
    try:
        out = c1.snoop()
        it, _ = c2.adjust()
        assert out["rounds"] == 1 and out["converged"] and out["iterations"] == it and not out["excluded"].any()
        assert out["table"][0, :3].tolist() == [0, 0, 0] and 0 < out["table"][0, 3] < sr.CRIT
        np.testing.assert_array_equal(c1.get_xhat(), c2.get_xhat())
        np.testing.assert_array_equal(c1.get_weights(), np.ones(s.od.n))  # no weights were switched on
        for p, q in zip(c1.residuals(), c2.residuals()):
            np.testing.assert_array_equal(p, q)
        assert c1.step() == c2.step()
        np.testing.assert_array_equal(c1.get_xhat(), c2.get_xhat())
    finally:
        c1.close()
        c2.close()


# ---- 3. contracts, bitwise ---------------------------------------------------------------------------------------------
def test_two_fresh_contexts_are_bitwise_equal(fba, oracle, root):
    s = sr.restated(fba, oracle, root, "P")
    a, b = _snoop(fba, s.ds, s.pre), _snoop(fba, s.ds, s.pre)
    for k in ("excluded", "stat", "table"):
        np.testing.assert_array_equal(a[0][k], b[0][k])
    assert [a[0][k] for k in ("rounds", "iterations", "converged", "status_bits")] == [b[0][k] for k in ("rounds", "iterations", "converged", "status_bits")]
    for p, q in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(p, q)


def test_one_round_tests_only(fba, oracle, root):
    """max_rounds = 1 on scene A: the picks are reported, nothing is changed -- weights and xhat as fba_adjust's"""
    s = sr.restated(fba, oracle, root, "A")
    c1, c2 = _ctx(fba, s.ds), _ctx(fba, s.ds)
    try:
        out = c1.snoop(max_rounds=1)
        it, _ = c2.adjust()
        assert out["rounds"] == 1 and out["iterations"] == it and not out["converged"] and not out["excluded"].any()
        assert out["table"][0, :3].tolist() == [len(s.a.picks[0]), 0, 0]
        np.testing.assert_array_equal(c1.get_xhat(), c2.get_xhat())
        np.testing.assert_array_equal(c1.get_weights(), np.ones(s.od.n))
        for p, q in zip(c1.residuals(), c2.residuals()):
            np.testing.assert_array_equal(p, q)
        assert c1.step() == c2.step()
        np.testing.assert_array_equal(c1.get_xhat(), c2.get_xhat())
    finally:
        c1.close()
        c2.close()


def test_max_share_stop(fba, oracle, root):
    """scene A under max_share = 0.5 %: 4 picks of 720 points pass it, nothing is applied, bit 1 is set"""
    s = sr.restated(fba, oracle, root, "A")
    out, _, _, _, wts = _snoop(fba, s.ds, max_share=0.005)
    assert out["rounds"] == 1 and not out["converged"] and out["status_bits"] == 2 and not out["excluded"].any()
    assert out["table"][0, :3].tolist() == [len(s.a.picks[0]), 0, 0]
    np.testing.assert_array_equal(wts, np.ones(s.od.n))


@pytest.mark.parametrize("case", ["world2", "loss", "damping", "pending", "bad-option"])
def test_refusals_leave_the_context_untouched(fba, oracle, root, case):
    s = sr.restated(fba, oracle, root, "A")
    kw = dict(rank=0, world=2) if case == "world2" else {}
    c1, c2 = _ctx(fba, s.ds, **kw), _ctx(fba, s.ds, **kw)

    def step(c, refuse):
        opts, code = {}, 5
        if case == "bad-option":
            opts, code = dict(crit=-1.0), 1
        if case == "pending":
            code = 1
        c.accumulate()
        if case == "world2" and not refuse:
            return 0.0  # (one rank of two: its share of the normal equations alone is not solved here)
        if case == "pending":
            c.solve_update_async()
        if refuse:
            with pytest.raises(fba.capi.FBAError) as e:
                c.snoop(**opts)
            assert e.value.code == code and "fba_snoop" in str(e.value)
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


def test_snooped_context_against_a_fresh_one(fba, oracle, root):
    """a snooped context and a fresh one given its weights and its xhat: the step, the residuals and fba_reliability
    are bitwise equal"""
    s = sr.restated(fba, oracle, root, "A")
    c1, c3 = _ctx(fba, s.ds), _ctx(fba, s.ds)
    try:
        out = c1.snoop()
        assert out["converged"]
        x1, w1 = c1.get_xhat(), c1.get_weights()
        c3.set_weights(w1)
        c3.set_xhat(x1)
        assert c1.step() == c3.step()
        np.testing.assert_array_equal(c1.get_xhat(), c3.get_xhat())
        ra, rb = c1.residuals(), c3.residuals()
        for p, q in zip(ra, rb):
            np.testing.assert_array_equal(p, q)
        for p, q in zip(c1.reliability(ra[2][3]), c3.reliability(rb[2][3])):
            np.testing.assert_array_equal(p, q)
    finally:
        c1.close()
        c3.close()


def test_allocations_return(fba, oracle, root):
    s = sr.restated(fba, oracle, root, "C")
    before = fba.capi.live_allocations()
    ctx = _ctx(fba, s.ds)
    ctx.set_timing(True)
    out = ctx.snoop()
    ms = ctx.timings()
    assert out["rounds"] == s.a.rounds and ms[7] > 0.0 and not ms[:7].any()
    assert fba.capi.live_allocations() > before
    ctx.close()
    assert fba.capi.live_allocations() == before


# ---- 4. end to end -----------------------------------------------------------------------------------------------------
def test_adjust_snoop_leaves_no_flagged_active_point(fba, oracle, root):
    s = sr.restated(fba, oracle, root, "A")
    res = fba.adjust(s.ds, snoop=True, reliability=True)
    assert np.nonzero(res.snoop_excluded == 1)[0].tolist() == s.rows and res.snoop_rounds == s.a.rounds and res.snoop_converged
    act = np.repeat(res.snoop_excluded != 1, 2)
    print(f"snoop adjust: largest |w| of an active row {np.abs(res.wstat[act]).max():.4f}, sigma02 {res.sigma02:.4f}, "
          f"over the active rows {res.sigma02_active:.4f}")
    assert (np.abs(res.wstat[act]) <= sr.CRIT).all()
    np.testing.assert_array_equal(res.weights, np.where(act, 1.0, LOW))
    assert res.iterations == len(s.a.deltasum) + 1
    n, u = s.a.A.shape
    vtpv = float(np.sum(res.weights * (res.v / sr.MEAS_STD) ** 2))
    np.testing.assert_allclose(res.sigma02_active, vtpv / (n - 2 * len(s.rows) - u + 7), rtol=1e-12)
    with pytest.raises(ValueError):
        fba.adjust(s.ds, snoop=True, robust="huber")


def test_adjust_snoop_then_vce(fba, oracle, root):
    """the excluded rows join no group: the .vce table's "(no group)" entry counts exactly their rows"""
    s = sr.restated(fba, oracle, root, "A")
    res = fba.adjust(s.ds, snoop=True, vce="xy")
    assert np.nonzero(res.snoop_excluded == 1)[0].tolist() == s.rows
    assert res.vce_names == ["x", "y", "(no group)", "(priors)"]
    assert res.vce_table[-1, :, 2].tolist() == [720 - len(s.rows), 720 - len(s.rows), 2 * len(s.rows), 0]
    ex = np.repeat(res.snoop_excluded == 1, 2)
    np.testing.assert_allclose(res.weights[ex], LOW, rtol=2.0 ** -52)
    np.testing.assert_allclose(res.weights[~ex], (1.0 / res.vce_component[:2])[np.arange(s.od.n) % 2][~ex], rtol=1e-13)


def test_cli_main_snoop(fba, oracle, root):
    """fba_cli.py main <folder> --snoop --reliability on scene C: the .snp table parses back to the planted rows"""
    from fba_amd import report
    s = sr.restated(fba, oracle, root, "C")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fba_cli.py"), "main", s.folder, "--snoop", "--reliability"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows, imgs, pts, words, stat, v, hist = report.read_snp(os.path.join(s.folder, "synth.snp"))
    assert rows.tolist() == s.rows and words == ["EXCLUDED"] * len(s.rows)
    assert imgs == [s.ds.pho_image[i] for i in s.rows] and pts == [s.ds.pho_target[i] for i in s.rows]
    np.testing.assert_array_equal(hist[:, :3], s.a.table[:, :3])
    np.testing.assert_allclose(stat, s.a.W[-1][s.rows], rtol=1e-6)
    assert (stat > sr.CRIT).all() and os.path.isfile(os.path.join(s.folder, "synth.rel"))
