"""Prior observations of unknowns on the GPU (fba_create_priors / fba_get_priors: k_prior_cam, k_gen_point's prior
terms, k_prior_resid) against the dense oracle with the prior rows appended.

The oracle is composed here from oracle/fba_oracle.py's functions (gn): a Gauss-Newton loop over oracle.build_awg;
per pass the rows sc[index] e_index -- sc = oracle.descale(od, ones(u), dist_scaling), 1 / dist_scaling on the
distortion unknowns, whose columns are in scaled units -- appended to A, x[index] - l to w and 1 / sigma^2 to P;
solved by the explicit inverse (oracle.solve_dense) and by test_gpu_block_shapes._solve_lu; oracle.descale on delta.
The image residuals are the reference's v = A delta + w, a prior's is xhat[index] - l at the final xhat,
sigma0^2 = (v'Pv + sum p v^2) / (n + n_prior - u).

Bars: none of its own.  xhat after every pass, per group and per element: max(1e-9, 20 x the oracle's own spread of
that pass and group), the explicit inverse against the LU solve of the same augmented system
(test_gpu_block_shapes._every_pass); every deltasum by the same rule on the scale of the first (flag_masks.bars'
"deltasum_hist": with three images' priors as the whole datum the oracle's two routes are 1.4e-9 apart on it).  sigma0^2 at vtol = max(1e-9, 20 x that pair's spread on sigma0^2),
RMS at vtol, v and RSD at 10 vtol of their largest entry, diag(Cx) at max(1e-8, 20 x the oracle's own spread on it)
(test_gpu_weights.check_solution / check_adjustment).  r and w of the image measurements AND of the priors in one
vector: test_gpu_reliability._reference / _check with the augmented A, w, P -- the redundancy sum is then
n + n_prior - u (+ 7).  Prior residuals: the xhat bar of the unknown's group times the group's scale.  The oracle's
two routes must agree on the iteration count, and no deltasum may lie within 1.25x of Threshold_Value
(test_gpu_weights.weighted_oracle's guard).  The measured errors of one run, with the oracle's own spreads beside
them: profiles/priors_gpu_errors.log (the "priors ..." prints of this module).
"""
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import distortion_scale, param_groups

pytestmark = pytest.mark.gpu


# ---- the oracle with prior rows ---------------------------------------------------------------------------------
def gn(oracle, od, pri, lu=False, x0=None, steps=None, wt=None, loss=None, k=None):
    """main.m:407-494 with the prior rows appended (steps: exactly that many passes from x0, for IRLS)"""
    from test_gpu_block_shapes import _solve_lu
    from test_gpu_weights import loss_factor
    s = od.settings
    idx, l, sig = pri
    x, names = oracle.buildxhat(od)
    if x0 is not None:
        x = np.array(x0, dtype=np.float64)
    u, m = len(x), len(idx)
    P0 = oracle.weights(od) * (1.0 if wt is None else wt)
    pp = 1.0 / np.asarray(sig, dtype=np.float64) ** 2
    hist, dsum, deltasum, count = [x.copy()], [], 100.0, 0
    cap = s["Iteration_Cap"] if steps is None else steps
    while deltasum > s["threshold"] or steps is not None:
        count += 1
        A, w, G, dsc = oracle.build_awg(od, x)
        P = P0 * loss_factor(loss, k, P0, w) if loss else P0
        sc = oracle.descale(od, np.ones(u), dsc)
        Ap = np.zeros((m, u))
        Ap[np.arange(m), idx] = sc[idx]
        Aa, wa, Pa = np.vstack([A, Ap]), np.concatenate([w, x[idx] - l]), np.concatenate([P, pp])
        delta = _solve_lu(od, Aa, wa, G, Pa) if lu else oracle.solve_dense(od, Aa, wa, G, Pa)[0]
        delta = oracle.descale(od, delta, dsc)
        x = x + delta
        hist.append(x.copy())
        deltasum = float(np.sum(np.abs(delta)))
        dsum.append(deltasum)
        if count >= cap:
            break
    v, vp = A @ delta + w, x[idx] - l
    n = len(v)
    vtpv_p = float(np.sum(pp * vp ** 2))
    sigma02 = (float(v @ (P * v)) + vtpv_p) / (n + m - u)
    aug = SimpleNamespace(A=Aa, w=wa, G=G, v=np.concatenate([v, vp]), dist_scaling=dsc, sigma02=sigma02, xhat=x, names=names)
    return SimpleNamespace(xhat=x, names=names, iterations=count, deltasum=dsum, xhat_hist=hist, A=A, w=w, G=G,
                           dist_scaling=dsc, delta=delta, v=v, vp=vp, P=P, Pa=Pa, rsd=oracle.build_rsd(od, v, x),
                           rms=(float(np.sqrt(np.mean(v[0::2] ** 2))), float(np.sqrt(np.mean(v[1::2] ** 2)))),
                           sigma02=sigma02, vtpv_p=vtpv_p, dof=n + m - u, aug=aug, eff=P / oracle.weights(od))


def reference(oracle, od, pri, rel=True, **kw):
    """the explicit-inverse run `ro`, the LU run `lu`, the oracle's own spread per pass, the bars of the module
    docstring and (rel) r / w's reference over image measurements and priors"""
    from test_gpu_block_shapes import _errors
    from test_gpu_reliability import _reference
    from test_gpu_weights import _Weighted
    ro, lu = gn(oracle, od, pri, **kw), gn(oracle, od, pri, lu=True, **kw)
    assert lu.iterations == ro.iterations
    if "steps" not in kw:
        thr = od.settings["threshold"]
        near = [d for d in ro.deltasum if thr / 1.25 <= d <= thr * 1.25]
        assert not near, f"the oracle's deltasum {near} is within 1.25x of Threshold_Value: pick other values"
    s_s02 = abs(lu.sigma02 - ro.sigma02) / ro.sigma02
    ref = dict(od=od, pri=pri, ro=ro, lu=lu, s_s02=s_s02, vtol=max(1e-9, 20 * s_s02),
               spread=[_errors(lu.xhat_hist[i], ro.xhat_hist[i], ro) for i in range(ro.iterations + 1)],
               spread_dsum=np.abs(np.array(lu.deltasum) - np.array(ro.deltasum)) / ro.deltasum[0])
    if rel:
        ref["rel"] = _reference(_Weighted(oracle, ro.Pa), od, ro.aug, lu)
    return ref


def index_of(names, wanted):
    pos = {nm: i for i, nm in reversed(list(enumerate(names)))}
    return np.array([pos[nm] for nm in wanted], dtype=np.int64)


def from_covariance(oracle, od, idx, f, seed=7, base=None, block=0):
    """sigma_j = f sqrt(cx_diag_j) of the unpriored oracle run, l_j = xhat_j + sigma_j N(0, 1) from default_rng(seed):
    its draws [block len(idx), (block + 1) len(idx))"""
    base = base or oracle.adjust(od)
    cd = oracle.covariance(od, base)[0]
    sig = f * np.sqrt(cd[idx])
    z = np.random.default_rng(seed).standard_normal((block + 1, len(idx)))[block]
    return idx, base.xhat[idx] + sig * z, sig


# ---- checks -----------------------------------------------------------------------------------------------------
def _ctx(fba, ds, **kw):
    return fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings), **kw)


def check_passes(tag, fba, ds, ref):
    """xhat after every pass (test_gpu_block_shapes._every_pass's rule) and every deltasum (flag_masks.bars');
    -> the last xhat"""
    from test_gpu_block_shapes import _errors, _fmt
    ro = ref["ro"]
    ctx = _ctx(fba, ds, priors=ref["pri"])
    try:
        hist, dsum = [ctx.buildxhat()], []
        for _ in range(ro.iterations):
            dsum.append(ctx.step())
            hist.append(ctx.get_xhat())
    finally:
        ctx.close()
    failed = []
    for i in range(1, ro.iterations + 1):
        err, spread = _errors(hist[i], ro.xhat_hist[i], ro), ref["spread"][i]
        e_d = abs(dsum[i - 1] - ro.deltasum[i - 1]) / ro.deltasum[0]
        print(f"priors {tag} pass {i} (error/oracle's own spread): deltasum={e_d:.1e}/{ref['spread_dsum'][i - 1]:.1e} "
              + _fmt(err, spread))
        failed += [(i, g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
        if not e_d <= max(1e-9, 20 * ref["spread_dsum"][i - 1]):
            failed.append((i, "deltasum", e_d, ref["spread_dsum"][i - 1]))
    assert not failed, failed  # (pass, group, error, the oracle's own spread)
    return hist[-1]


def unit_bars(names, dist_scaling, x, idx, rel_of_group):
    """per prior: a relative xhat bar of its unknown's group times the group's scale (conftest.group_rel_err's:
    distortion terms in scaled units), in the unknown's own units"""
    sc = distortion_scale(names, dist_scaling)
    bar = np.zeros(len(idx))
    for g, members in param_groups(names).items():
        scale = np.max(np.abs(x[members] * sc[members]))
        for j in np.nonzero(np.isin(idx, members))[0]:
            bar[j] = rel_of_group(g) * scale / sc[idx[j]]
    return bar


def prior_bar(ref):
    """the xhat bar of the last pass, per prior"""
    ro = ref["ro"]
    return unit_bars(ro.names, ro.dist_scaling, ro.xhat, ref["pri"][0], lambda g: max(1e-9, 20 * ref["spread"][-1][g]))


def check_result(tag, oracle, ref, res, ds, rel=True):
    """a whole fba.adjust(..., priors=, reliability=True) against reference()"""
    import flag_masks as fm
    from test_gpu_reliability import _check
    from test_gpu_weights import _Weighted, cov_diag
    ro, lu, vtol, od = ref["ro"], ref["lu"], ref["vtol"], ref["od"]
    assert res.iterations == ro.iterations
    e_s02 = abs(res.sigma02 - ro.sigma02) / ro.sigma02
    e_v = float(np.abs(res.v - ro.v).max() / np.abs(ro.v).max())
    e_rsd = float(np.abs(res.rsd[:, 1:] - ro.rsd[:, 1:]).max() / np.abs(ro.rsd[:, 1:]).max())
    bar_p = prior_bar(ref)
    e_p = np.abs(res.prior_v - ro.vp)
    worst = int(np.argmax(e_p / bar_p))
    cdo, cdl = cov_diag(oracle, od, ro.aug, ro.Pa), cov_diag(oracle, od, lu.aug, lu.Pa)
    own = max(fm.cov_self_spread(_Weighted(oracle, ro.Pa), od, ro.aug)[0], float(np.max(np.abs(cdl - cdo) / cdo)))
    e_c = float(np.max(np.abs(res.cx_diag - cdo) / np.abs(cdo)))
    print(f"priors {tag} converged (error/oracle's own spread): it {res.iterations} n_prior {len(ro.vp)} dof {ro.dof} "
          f"sigma02={e_s02:.1e}/{ref['s_s02']:.1e} v={e_v:.1e} rsd={e_rsd:.1e} prior v worst error/bar "
          f"{e_p[worst]:.1e}/{bar_p[worst]:.1e} diag(Cx)={e_c:.1e}/{own:.1e}")
    assert e_s02 <= vtol
    np.testing.assert_allclose(res.rms[:2], ro.rms[:2], rtol=vtol)
    assert e_v <= 10 * vtol and e_rsd <= 10 * vtol
    assert (e_p <= bar_p).all(), (worst, e_p[worst], bar_p[worst])
    np.testing.assert_allclose(res.cx_diag, cdo, rtol=max(1e-8, 20 * own), atol=0)
    np.testing.assert_array_equal(res.prior_index, ref["pri"][0])
    if rel:
        both = SimpleNamespace(redundancy=np.concatenate([res.redundancy, res.prior_r]),
                               wstat=np.concatenate([res.wstat, res.prior_w]))
        print(f"priors {tag}: r_prior {res.prior_r.min():.3g}..{res.prior_r.max():.3g} max|w_prior| {np.abs(res.prior_w).max():.2f}")
        _check(f"priors {tag}", both, ref["rel"], od, ro.aug)


def run_case(tag, fba, oracle, folder, pri, ds=None):
    od = oracle.load_folder(folder)
    ref = reference(oracle, od, pri)
    ds = ds or fba.load_folder(folder)
    last = check_passes(tag, fba, ds, ref)
    res = fba.adjust(ds, priors=pri, reliability=True)
    np.testing.assert_array_equal(res.xhat, last)  # fba_adjust is the stepped loop
    check_result(tag, oracle, ref, res, ds)
    return ref, res


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return {"root": tmp_path_factory.mktemp("priors"), "scenes": {}, "cache": {}}


# ---- 1. the datum from GNSS alone -------------------------------------------------------------------------------
GNSS_SIGMA = 20.0


def gnss_scene(fba, work, ic="0"):
    """test_gpu_block_shapes' u129 scene (20 images x 300 points, seed 9, nK = 4) without its border: no control
    point, no inner constraints -- the position priors are the whole datum"""
    key = "gnss" + ic
    if key not in work["scenes"]:
        from fba_amd import synth
        sc = synth.generate(20, 300, seed=9, obs_per_point=6)
        folder = synth.write_folder(sc, str(work["root"] / key), nk=4, cfg_overrides={"Inner_Constraints": ic})
        work["scenes"][key] = dict(sc=sc, folder=folder, ds=fba.load_folder(folder))
    return work["scenes"][key]


def gnss_priors(fba, s, images=None, blunder=None):
    """Xc Yc Zc of the images: l = C_true + N(0, 20) from default_rng(123) (one draw per coordinate of the images
    used, in their order), sigma = 20; blunder: (prior number, sigmas) added to that value"""
    names = fba.xhat_names(s["ds"])
    images = list(range(20) if images is None else images)
    ext = s["ds"].EXT
    idx = index_of(names, [f"{c}_{ext[i][0]}_{ext[i][1]}" for i in images for c in ("Xc", "Yc", "Zc")])
    l = (s["sc"]["C_true"][images] + np.random.default_rng(123).normal(0.0, GNSS_SIGMA, (len(images), 3))).reshape(-1)
    if blunder:
        l[blunder[0]] += blunder[1] * GNSS_SIGMA
    return idx, l, np.full(len(idx), GNSS_SIGMA)


@pytest.mark.parametrize("leaf,images", [(None, None), (12, None), (None, (0, 7, 17))])
def test_datum_from_gnss_alone(fba, oracle, work, monkeypatch, leaf, images):
    """a free network with neither control points nor inner constraints, held by position priors alone: all 20
    images, in one image block and cut by FBA_ND_LEAF = 12 (11 padding slots, priors on images of both blocks: the
    table's rows go through the slot order), and three images only (9 priors, redundancies down to 0.006)"""
    from test_gpu_block_shapes import ROWS, assert_shape
    row = "u129" if leaf is None else "u129-leaf12"
    if leaf is None:
        monkeypatch.delenv("FBA_ND_LEAF", raising=False)
    else:
        monkeypatch.setenv("FBA_ND_LEAF", str(leaf))
    s = gnss_scene(fba, work)
    assert ROWS[row]["leaf"] == leaf
    assert_shape(fba, s["ds"], row)
    pri = gnss_priors(fba, s, images)
    ref, res = run_case(f"gnss leaf={leaf} images={'all' if images is None else images}", fba, oracle, s["folder"], pri, s["ds"])
    assert ref["ro"].dof == 2 * s["ds"].n_pts + len(pri[0]) - len(res.xhat)


def test_gnss_blunder_is_found(fba, oracle, work, monkeypatch):
    """+10 sigma on one GNSS coordinate (prior 31: Yc of the 11th image): that prior has the largest |w| of all
    priors, in the oracle and on the GPU, at the oracle's value (check_result's w bar)"""
    monkeypatch.delenv("FBA_ND_LEAF", raising=False)
    s = gnss_scene(fba, work)
    pri = gnss_priors(fba, s, blunder=(31, 10.0))
    ref, res = run_case("gnss blunder", fba, oracle, s["folder"], pri, s["ds"])
    wo = ref["rel"]["w"][-len(pri[0]):]
    print(f"priors gnss blunder: oracle |w| {abs(wo[31]):.2f} at 31, next {np.abs(np.delete(wo, 31)).max():.2f}; GPU "
          f"{abs(res.prior_w[31]):.2f}, next {np.abs(np.delete(res.prior_w, 31)).max():.2f}")
    assert int(np.argmax(np.abs(wo))) == 31 and int(np.argmax(np.abs(res.prior_w))) == 31


# ---- 2. cam0 with a mix -----------------------------------------------------------------------------------------
# which 31 draws of default_rng(7) a cam0 case takes: the first 31 for f = 3; for f = 0.1 the fifth 31.  With tight
# priors and the inner constraints together (stage3_pinhole, f = 0.1) the oracle's last deltasum sits near
# Threshold_Value = 1e-6 whatever the draw -- blocks 0..3 give 8.1e-7 (4 passes), 1.16e-6 (5), 9.7e-7 (4), 9.9e-7 (4),
# all inside reference()'s 1.25x guard; block 4 gives 1.62e-6 then 1.2e-8 (5 passes) and is clear of it
CAM0_DRAWS = {3.0: 0, 0.1: 4}


def cam0_mix(oracle, od, f, base=None):
    """31 priors: the six EOPs of the first and the sixth image, c, k1, k2, p1 and the first five tie points' X Y Z
    (regular points: they take the general path because of their priors)"""
    names = oracle.buildxhat(od)[1]
    u_img, u_cam = oracle.counts(od.settings)
    cid = names[u_img * od.numImg].split("_", 1)[1]
    tie0 = u_img * od.numImg + u_cam * od.numCam
    idx = np.concatenate([np.arange(0, 6), np.arange(5 * u_img, 5 * u_img + 6),
                          index_of(names, [f"{h}_{cid}" for h in ("c", "k1", "k2", "p1")]), np.arange(tie0, tie0 + 15)])
    assert len(idx) == 31 and names[idx[13]].startswith("k1_") and names[idx[14]].startswith("k2_")
    return from_covariance(oracle, od, idx, f, base=base, block=CAM0_DRAWS[f])


def _cam0_base(oracle, work, folder):
    if folder not in work["cache"]:
        od = oracle.load_folder(folder)
        work["cache"][folder] = (od, oracle.adjust(od))
    return work["cache"][folder]


@pytest.mark.parametrize("variant", ["stage3_noic_pinhole", "stage3_pinhole"])
@pytest.mark.parametrize("f", [3.0, 0.1])
def test_cam0_mix(fba, oracle, cam0_folders, work, variant, f):
    """control points (noic) and the inner-constraint border together with priors, loose (f = 3) and tight
    (f = 0.1); a k2 prior is among them, so a mis-scaled distortion row cannot pass"""
    od, base = _cam0_base(oracle, work, cam0_folders[variant])
    pri = cam0_mix(oracle, od, f, base)
    run_case(f"cam0 {variant} f={f}", fba, oracle, cam0_folders[variant], pri)


# ---- 3. shapes --------------------------------------------------------------------------------------------------
def test_control_leaf12_one_image_per_block(fba, oracle, work, monkeypatch):
    """4 blocks, 30 padding slots: all EOPs of the first image of every image block, and every camera unknown"""
    from test_gpu_block_shapes import CB, _scene, _set_leaf, assert_shape
    row = "control-leaf12"
    _set_leaf(monkeypatch, row)
    s = _scene(fba, work, row)
    assert_shape(fba, s["ds"], row)
    order = fba.capi.image_order(s["ds"].pack())
    first = {}
    for slot, e in enumerate(order):
        if e >= 0:
            first.setdefault(6 * slot // CB, int(e))
    assert len(first) >= 3
    od = oracle.load_folder(s["folder"])
    u_img, u_cam = oracle.counts(od.settings)
    idx = np.concatenate([np.arange(6 * e, 6 * e + 6) for e in sorted(first.values())]
                         + [np.arange(u_img * od.numImg, u_img * od.numImg + u_cam)])
    run_case(row, fba, oracle, s["folder"], from_covariance(oracle, od, idx, 3.0), s["ds"])


@pytest.mark.parametrize("name", ["rig2", "dup"])
def test_general_points_with_priors(fba, oracle, tmp_path, name):
    """priors on points that are general anyway (two cameras / measured twice in one image) and on both cameras' c"""
    from test_gpu_general import SCENES, _folder
    folder = _folder(tmp_path, name, **SCENES[name])
    od = oracle.load_folder(folder)
    names = oracle.buildxhat(od)[1]
    cams, imgs = {}, {}
    for t, k, e in zip(od.tie_index, od.cam_num, od.ext_index):
        cams.setdefault(int(t), set()).add(int(k))
        imgs.setdefault(int(t), []).append(int(e))
    general = sorted(t for t in cams if t >= 0 and (len(cams[t]) > 1 or len(set(imgs[t])) < len(imgs[t])))[:5]
    assert len(general) == 5
    u_img, u_cam = oracle.counts(od.settings)
    tie0 = u_img * od.numImg + u_cam * od.numCam
    idx = np.concatenate([np.array([i for i, nm in enumerate(names) if nm.startswith("c_")])]
                         + [np.arange(tie0 + 3 * t, tie0 + 3 * t + 3) for t in general])
    assert len(idx) == od.numCam + 15
    run_case(f"general {name}", fba, oracle, folder, from_covariance(oracle, od, idx, 3.0))


def test_partial_flag_set(fba, oracle, work):
    """flag_masks' mix_a (Omega, Zc, yp and the radial terms not estimated): reference-layout indices shift"""
    import flag_masks as fm
    folder = fm.synth_folder(work["root"], "control", "mix_a")
    od = oracle.load_folder(folder)
    names = oracle.buildxhat(od)[1]
    u_img, u_cam = oracle.counts(od.settings)
    assert (u_img, u_cam) == (4, 4)
    tie0 = u_img * od.numImg + u_cam * od.numCam
    idx = np.concatenate([np.arange(0, 4), np.arange(5 * u_img, 5 * u_img + 4),
                          np.array([i for i, nm in enumerate(names) if nm.split("_")[0] in ("xp", "c", "p1")]),
                          np.arange(tie0, tie0 + 15)])
    run_case("mask mix_a", fba, oracle, folder, from_covariance(oracle, od, idx, 3.0))


# ---- 4. every point general -------------------------------------------------------------------------------------
def test_every_point_general(fba, oracle, work, monkeypatch, capfd):
    """sigma = 1e30 on every tie coordinate of the u129 free network (inner constraints on): every point takes the
    general path (no k_lin_reduce chunk is left) and xhat, sigma0^2 and diag(Cx) are the no-prior oracle's"""
    from test_gpu_block_shapes import _errors, _fmt, _solve_lu
    monkeypatch.delenv("FBA_ND_LEAF", raising=False)
    s = gnss_scene(fba, work, ic="1")
    od = oracle.load_folder(s["folder"])
    ro, lu = oracle.adjust(od), oracle.adjust(od, solver=_solve_lu)
    assert lu.iterations == ro.iterations
    u_img, u_cam = oracle.counts(od.settings)
    tie0 = u_img * od.numImg + u_cam * od.numCam
    idx = np.arange(tie0, len(ro.xhat))
    pri = (idx, ro.xhat[idx], np.full(len(idx), 1e30))
    ctx = _ctx(fba, s["ds"], priors=pri, verbose=True)
    ctx.close()
    log = capfd.readouterr().err
    assert " chunks 0," in log and f"general points {len(idx) // 3}" in log, log
    res = fba.adjust(s["ds"], priors=pri)
    assert res.iterations == ro.iterations
    err, spread = _errors(res.xhat, ro.xhat, ro), _errors(lu.xhat, ro.xhat, ro)
    s_s02 = abs(lu.sigma02 - ro.sigma02) / ro.sigma02
    # the divisor counts the 900 priors; their v'Pv term is ~1e-60
    n, u = ro.A.shape
    e_s02 = abs(res.sigma02 * (n + len(idx) - u) / (n - u) - ro.sigma02) / ro.sigma02
    cdo = oracle.covariance(od, ro)[0] * (n - u) / (n + len(idx) - u)  # Cx carries the run's own sigma0^2
    e_c = float(np.max(np.abs(res.cx_diag - cdo) / cdo))
    print(f"priors all-general (error/oracle's own spread): sigma02={e_s02:.1e}/{s_s02:.1e} diag(Cx)={e_c:.1e} " + _fmt(err, spread))
    failed = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
    assert not failed, failed
    assert e_s02 <= max(1e-9, 20 * s_s02)
    assert e_c <= 1e-8  # test_gpu_parity._check_cov's bar


# ---- 6. two rank contexts ---------------------------------------------------------------------------------------
def test_two_ranks(fba, oracle, cam0_folders, work):
    """world = 2, replicated solve, cam0's mix: every rank takes the full list, rank 0 adds the camera-side priors
    and a tie point's owner that point's; xhat is the single context's at test_gpu_parity's two-rank bar (1e-10 per
    group), the ranks' get_priors residuals and v'Pv shares sum to the single context's"""
    from conftest import group_rel_err
    from test_gpu_reliability import _step_ranks
    folder = cam0_folders["stage3_pinhole"]
    od, base = _cam0_base(oracle, work, folder)
    pri = cam0_mix(oracle, od, 3.0, base)
    ds = fba.load_folder(folder)
    single = _ctx(fba, ds, priors=pri)
    ranks = [_ctx(fba, ds, rank=r, world=2, priors=pri) for r in range(2)]
    try:
        _step_ranks(single, ranks, 4)
        res = [c.residuals() for c in [single] + ranks]  # (ahead of build_awg, which drops the linearisation)
        st, vi = [r[2] for r in res], res[0][0]
        xs = single.get_xhat()
        xr = sum(c.get_xhat(owned_only=True) for c in ranks)
        _, _, _, dsc = single.build_awg(xs)
        err = group_rel_err(xr, xs, fba.xhat_names(ds), dsc)
        v1, p1 = single.get_priors()
        parts = [c.get_priors() for c in ranks]
        tie_owner, _ = fba.capi.partition(ds.pack(), 2)
        # the 16 camera-side priors on rank 0, the 15 tie priors (points 0..4) on their owner
        mine = [np.concatenate([np.full(16, r == 0), np.repeat(tie_owner[:5] == r, 3)]) for r in range(2)]
        for (v, _), m in zip(parts, mine):
            assert (v[~m] == 0).all() and (v[m] != 0).all()
        vs, ps = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
        print(f"priors two ranks: xhat {err}; summed prior residuals vs single {np.abs(vs - v1).max():.2e}, v'Pv "
              f"shares {abs(ps - p1) / p1:.2e}")
        assert max(err.values()) <= 1e-10, err
        assert (np.abs(vs - v1) <= unit_bars(fba.xhat_names(ds), dsc, xs, pri[0], lambda g: 1e-10)).all()
        # v'Pv's prior term: sum p v^2 with every v at that bar
        bar_p = 2 * np.sum(np.abs(v1) / pri[2] ** 2 * unit_bars(fba.xhat_names(ds), dsc, xs, pri[0], lambda g: 1e-10))
        assert abs(ps - p1) <= bar_p
        # stats[4] carries each rank's share (image rows at test_gpu_reliability's two-rank bar on v, 1e-9 of its
        # scale, propagated through v'Pv), stats[5] the full divisor
        assert st[1][5] == st[2][5] == st[0][5] == 2 * ds.n_pts + 31 - len(xs)
        bar_i = 2 * np.sum(oracle.weights(od) * np.abs(vi)) * 1e-9 * np.abs(vi).max()
        assert abs(st[1][4] + st[2][4] - st[0][4]) <= bar_i + bar_p
    finally:
        for c in [single] + ranks:
            c.close()


# ---- 7. contract ------------------------------------------------------------------------------------------------
def test_contract(fba, oracle, cam0_folders, work):
    """fba_create_priors(NULL) / n = 0 is fba_create, bit for bit; two contexts with the same priors give bitwise-
    equal xhat, cx_diag, r; a split request with priors is FBA_ERR_UNSUPPORTED; fba_build_awg returns what a context
    without priors returns"""
    import ctypes as C
    folder = cam0_folders["stage3_pinhole"]
    od, base = _cam0_base(oracle, work, folder)
    pri = cam0_mix(oracle, od, 3.0, base)
    ds = fba.load_folder(folder)
    ctxs = []

    def stepped(**kw):
        c = _ctx(fba, ds, **kw)
        ctxs.append(c)
        for _ in range(3):
            c.step()
        return c
    try:
        plain = stepped()
        empty = stepped(priors=(np.zeros(0, np.int64), np.zeros(0), np.zeros(0)))
        np.testing.assert_array_equal(empty.get_xhat(), plain.get_xhat())
        # the entry point itself with a NULL list and with n = 0
        pk, st = ds.pack(), fba.capi.make_settings(ds.settings)
        for prp in (None, C.byref(fba.capi.Priors(0, None, None, None))):
            h = C.c_void_p()
            opts = fba.capi.Options(0, 0, 1, 0, None, 0)
            fba.capi.check(fba.capi.lib.fba_create_priors(C.byref(pk.struct), C.byref(st), C.byref(opts), prp, C.byref(h)))
            x, d = np.zeros(plain.u), C.c_double()
            for _ in range(3):
                fba.capi.check(fba.capi.lib.fba_step(h, C.byref(d)))
            fba.capi.check(fba.capi.lib.fba_get_xhat(h, fba.capi.ptr(x), 0))
            n = C.c_int64(-1)
            fba.capi.check(fba.capi.lib.fba_get_priors(h, C.byref(n), None, None))
            fba.capi.lib.fba_destroy(h)
            np.testing.assert_array_equal(x, plain.get_xhat())
            assert n.value == 0
        a, b = stepped(priors=pri), stepped(priors=pri)
        np.testing.assert_array_equal(a.get_xhat(), b.get_xhat())
        assert not np.array_equal(a.get_xhat(), plain.get_xhat())
        for x, y in zip(a.get_priors(), b.get_priors()):
            np.testing.assert_array_equal(x, y)
        sa, sb = a.residuals()[2], b.residuals()[2]
        np.testing.assert_array_equal(sa, sb)
        assert sa[5] == 2 * ds.n_pts + 31 - a.u
        for x, y in zip(a.reliability(sa[3]), b.reliability(sb[3])):
            np.testing.assert_array_equal(x, y)
        with pytest.raises(fba.capi.FBAError) as ei:
            _ctx(fba, ds, rank=0, world=2, split=True, priors=pri)
        assert ei.value.code == 5 and "subtree split" in str(ei.value)  # FBA_ERR_UNSUPPORTED
        x0 = plain.buildxhat()
        for x, y in zip(_ctx_awg(fba, ds, x0, priors=pri), _ctx_awg(fba, ds, x0)):
            np.testing.assert_array_equal(x, y)
    finally:
        for c in ctxs:
            c.close()


def _ctx_awg(fba, ds, x0, **kw):
    c = _ctx(fba, ds, **kw)
    try:
        A, w, G, dsc = c.build_awg(x0)
    finally:
        c.close()
    return A, w, G, dsc


def test_huber_with_priors_three_irls_steps(fba, oracle, work):
    """test_gpu_weights' robust scene (cam0 with the planted blunder): L2 with priors to convergence, then exactly 3
    steps under Huber -- the loss re-weights the image measurements only, the priors keep their weight"""
    from test_gpu_block_shapes import _errors, _fmt
    from test_gpu_weights import HUBER_K, blunder_folder
    folder = blunder_folder(work["root"])
    od = oracle.load_folder(folder)
    pri = cam0_mix(oracle, od, 3.0)
    l2 = gn(oracle, od, pri)
    ref = reference(oracle, od, pri, rel=False, x0=l2.xhat, steps=3, loss="huber", k=HUBER_K)
    ro = ref["ro"]
    ds = fba.load_folder(folder)
    ctx = _ctx(fba, ds, priors=pri)
    try:
        it, _ = ctx.adjust()
        assert it == l2.iterations
        ctx.set_loss("huber", HUBER_K)
        for _ in range(3):
            ctx.step()
        xhat, (v, rsd, st), wts, (pv, pvtpv) = ctx.get_xhat(), ctx.residuals(), ctx.get_weights(), ctx.get_priors()
    finally:
        ctx.close()
    err, spread = _errors(xhat, ro.xhat, ro), ref["spread"][-1]
    e_s02 = abs(st[3] - ro.sigma02) / ro.sigma02
    e_v = float(np.abs(v - ro.v).max() / np.abs(ro.v).max())
    bar_p = prior_bar(ref)
    e_p = np.abs(pv - ro.vp)
    print(f"priors huber (error/oracle's own spread): sigma02={e_s02:.1e}/{ref['s_s02']:.1e} v={e_v:.1e} prior v'Pv "
          f"{abs(pvtpv - ro.vtpv_p) / ro.vtpv_p:.1e} down-weighted points {int((wts[0::2] < 0.999).sum())} " + _fmt(err, spread))
    failed = [(g, e, spread[g]) for g, e in err.items() if not e <= max(1e-9, 20 * spread[g])]
    assert not failed, failed
    assert e_s02 <= ref["vtol"] and e_v <= 10 * ref["vtol"]
    assert (e_p <= bar_p).all()
    assert (wts[0::2] < 0.999).any() and st[5] == ro.dof
