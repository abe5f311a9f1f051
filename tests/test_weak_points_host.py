"""The exact reference and the scenes of tests/test_gpu_weak_points.py, checked on the host (no GPU).

1. test_helper_matches_dense_mp   exact_solve.solve (block form) against exact_solve.solve_dense (mp.lu_solve and
                                  mp.inverse of the full bordered N) on 4 images x 10 points with one twin pair and two
                                  weak points: delta, the tie points' cofactor blocks, the camera-side diagonal and
                                  a Cx a' agree to 1e-40 of the largest entry, with and without G, with and without
                                  user weights.
2. test_helper_matches_oracle     on the plain base scene (no twins) the helper's delta is oracle.solve_dense's within
                                  the suite's 1e-9 bars: the helper answers the oracle's question.
3. test_tier_conditioning         cond(V) of every weak point, from the oracle's A at the start values, within a factor
                                  5 of K_COND (2500 / B)^2; every strong point below 1e3.  K_COND = 4.0: the geometric
                                  mean of the four weak points of chunk-fisheye-B30 is 2.78e4 = 4.0 x (2500 / 30)^2.
4. test_yardstick_cap             per scene (and for the second pass and the damped pass of the chunk scenes at tier
                                  0.3) the fp64 yardsticks -- oracle.solve_schur's delta, the plain NumPy block form of
                                  V^-1 + T C T' and a Cx a' -- against the exact solve, in every metric the GPU tests
                                  use: 20 x the yardstick stays <= 1e-3 (weak_scenes.CAP).  The figures are printed
                                  ("weak-host ..." lines).
"""
import numpy as np
import pytest

import exact_solve
import weak_scenes as ws

K_COND = 4.0


@pytest.fixture(scope="module")
def synth():
    import fba_import
    fba_import.load()
    from fba_amd import synth
    return synth


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("weak_host"), "scenes": {}}


def scene(synth, oracle, work, name):
    return ws.load(synth, oracle, work["root"], work["scenes"], name)


# ---- 1. the block form against the dense form, both in mp -------------------------------------------------------
def _rel40(a, b):
    """max |a - b| / max |b| over two equally shaped nests of mp numbers, in mp"""
    from mpmath import mp, mpf
    fa, fb = np.asarray(a, dtype=object).reshape(-1), np.asarray(b, dtype=object).reshape(-1)
    assert fa.shape == fb.shape
    with mp.workdps(exact_solve.DPS):
        return max(abs(mpf(x) - mpf(y)) for x, y in zip(fa, fb)) / max(abs(mpf(y)) for y in fb)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("border", [False, True], ids=["control", "free"])
def test_helper_matches_dense_mp(synth, oracle, tmp_path, border, weighted):
    b = ws.build(synth, "chunk", "fisheye", 30.0, base=dict(n_img=3, n_tie=8, seed=5, obs_per_point=3),
                 n_control=0 if border else 3, pairs=(0,), n_weak=2)
    od = oracle.load_folder(ws.write(synth, b, str(tmp_path / "tiny")))
    assert od.numImg == 4 and od.numGCP == 10 and len(b["weak"]) == 2
    x0, _ = oracle.buildxhat(od)
    # weights over two decades: they show that both forms carry P alike; both forms lose cond(N) x 1e-51, and the
    # dense LU of this 4-image network (cond(N) ~ 1e9 unweighted) has no digits to spare for six decades at 1e-40
    wt = 10.0 ** np.random.default_rng(7).uniform(-1.0, 1.0, od.n) if weighted else None
    lin = ws.linearise(oracle, od, x0, wt)
    assert (lin["G"] is not None) == border
    uc = ws.uc_of(oracle, od)
    blk = exact_solve.solve(lin["A"], lin["w"], lin["P"], uc, lin["G"], raw=True)
    dns = exact_solve.solve_dense(lin["A"], lin["w"], lin["P"], uc, lin["G"])
    err = {k: _rel40(blk[k], dns["mp"][k]) for k in ("delta", "cx_tie", "cx_cam_diag", "aCa")}
    cond = ws.point_conds(lin["A"], lin["P"], uc)
    print(f"weak-host helper vs dense mp (border {border}, weighted {weighted}): u={len(x0)} n={od.n} cond(V) up to "
          f"{cond.max():.1e} " + " ".join(f"{k} {float(v):.1e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= 1e-40, (k, float(v))
    # and the rounded outputs are the dense form's
    rnd = exact_solve.solve(lin["A"], lin["w"], lin["P"], uc, lin["G"])
    for k in err:
        np.testing.assert_array_equal(rnd[k], dns[k])


# ---- 2. the helper answers the oracle's question ----------------------------------------------------------------
@pytest.mark.parametrize("typ", ["fisheye", "pinhole"])
def test_helper_matches_oracle(synth, oracle, tmp_path, typ):
    from conftest import SMALL_SCENE_FLOOR, elem_rel_err, group_rel_err
    base = dict(ws.BASE)
    sc = synth.generate(base.pop("n_img"), base.pop("n_tie"), typ=typ, n_control=ws.N_CONTROL, **base)
    od = oracle.load_folder(synth.write_folder(sc, str(tmp_path / "plain"), nk=ws.NK))
    x0, names = oracle.buildxhat(od)
    lin = ws.linearise(oracle, od, x0)
    uc = ws.uc_of(oracle, od)
    assert ws.point_conds(lin["A"], lin["P"], uc).max() < 1e3
    ex = exact_solve.solve(lin["A"], lin["w"], lin["P"], uc, lin["G"])
    d_o, Cx = oracle.solve_dense(od, lin["A"], lin["w"], lin["G"], lin["P"])
    x1 = x0 + oracle.descale(od, ex["delta"], lin["dsc"])
    x1_o = x0 + oracle.descale(od, d_o, lin["dsc"])
    g = group_rel_err(x1_o, x1, names, lin["dsc"])
    e = elem_rel_err(x1_o, x1, names, lin["dsc"], floor=SMALL_SCENE_FLOOR)
    e_d = float(np.abs(d_o - ex["delta"]).max() / np.abs(ex["delta"]).max())
    nt = (len(x0) - uc) // 3
    blocks = np.array([Cx[uc + 3 * t:uc + 3 * t + 3, uc + 3 * t:uc + 3 * t + 3] for t in range(nt)])
    e_b = ws.block_errors(blocks, ex["cx_tie"], list(range(nt)), [])["weak_block"]
    e_q = float(np.abs(lin["P"] * (np.einsum("ij,jk,ik->i", lin["A"], Cx, lin["A"]) - ex["aCa"])).max())
    print(f"weak-host helper vs oracle.solve_dense ({typ}): xhat per group {max(g.values()):.1e} per element "
          f"{max(e.values()):.1e} delta {e_d:.1e} tie blocks {e_b:.1e} p a Cx a' {e_q:.1e}")
    assert max(g.values()) <= 1e-9 and max(e.values()) <= 1e-9 and e_d <= 1e-9
    assert e_b <= 1e-9 and e_q <= 1e-9


# ---- 3. the tiers are what they say -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ws.SCENES))
def test_tier_conditioning(synth, oracle, work, name):
    s = scene(synth, oracle, work, name)
    b, lin = s["b"], s["lin"]
    cond = ws.point_conds(lin["A"], lin["P"], ws.uc_of(oracle, s["od"]))
    nominal = K_COND * (ws.DEPTH / b["B"]) ** 2
    weak = cond[b["weak"]]
    print(f"weak-host cond {name}: weak {weak.min():.2e} .. {weak.max():.2e} (nominal {nominal:.2e}) strong up to "
          f"{cond[b['strong']].max():.1f}"
          + (f" cut {cond[b['cut']].min():.2e} .. {cond[b['cut']].max():.2e}" if b["cut"] else ""))
    assert len(weak) == 4 and (weak >= nominal / 5).all() and (weak <= nominal * 5).all()
    assert (cond[b["strong"]] < 1e3).all()
    if b["cut"]:  # two rays of base B once the third observation is excluded: the tier's conditioning, by the weights
        assert len(b["cut"]) == 6 and (cond[b["cut"]] >= nominal / 5).all() and (cond[b["cut"]] <= nominal * 5).all()
        assert (lin["P"] == lin["P"].min()).sum() == 12 and lin["P"].min() == ws.EXCLUDE * lin["P"].max()


# ---- 4. the yardstick and its cap -------------------------------------------------------------------------------
CASES = sorted(ws.SCENES) + [f"chunk-{t}-B0.3:{k}" for t in ("fisheye", "pinhole") for k in ("pass2", "damped")]


@pytest.mark.parametrize("case", CASES)
def test_yardstick_cap(synth, oracle, work, case):
    name, _, kind = case.partition(":")
    s = scene(synth, oracle, work, name)
    lin, lam = s["lin"], 0.0
    if kind == "pass2":
        if "ep" not in s:
            s["ep"] = ws.exact_pass(oracle, s["od"], lin)
        lin = ws.linearise(oracle, s["od"], s["ep"]["x1"], s["b"]["weights"])
        assert np.isfinite(lin["A"]).all() and np.isfinite(lin["w"]).all()
    elif kind == "damped":
        lam = ws.LAMBDA
    ep = ws.exact_pass(oracle, s["od"], lin, lam)
    if not kind:
        s["ep"] = ep
    import fba_import
    y = ws.yardsticks(s, lin, ep, fba_import.load().capi.eig3_host)
    if lam:  # no post-fit output after a damped solve (include/fba.h)
        y = {k: v for k, v in y.items() if k in ws.PASS_METRICS}
    print(f"weak-host yardstick {case}: " + " ".join(f"{k} {v:.1e}" for k, v in y.items()))
    r = 1.0 - lin["P"] * ep["exact"]["aCa"]
    d = 0 if lin["G"] is None else lin["G"].shape[1]
    if not lam:
        assert abs(r.sum() - (lin["A"].shape[0] - lin["A"].shape[1] + d)) <= 1e-9 and r.min() > 0 and r.max() < 1
    for k, v in y.items():
        assert 20 * v <= ws.CAP, (k, v)
