"""The MEX drop-ins with the reference's own signatures (mex/BuildAwG.c, mex/Buildxhat.c,
mex/BuildRSD.c), RUN without MATLAB: each is compiled against tests/mexstub (a stand-in for the MEX /
matrix API, test infrastructure) and libfba.so, and its mexFunction is called with the reference's
`data` struct (main.m:280-383) and cell arrays (main.m:196-258) built from the oracle's restatement
of the ingest.

* CPU: every drop-in (and the whole-loop gateway mex/fba_mex.c) compiles and links.
* GPU: the whole-loop gateway, the reference's main.m:386-602 in one call,
    [error, xhat, count, deltasum, v, RSD, stats, cx_diag, corr] = fba_mex(data, EXT, INT, TIE, CNT)
  on cam0 Stage-3 against the dense oracle (count, deltasum history, xhat per element, v, RSD, sigma0^2,
  diag(Cx), the EOP/IOP correlation blocks) and at config 3 (200 images x 5,000 tie points) against the
  C oracle's direct bordered solve (count, xhat per element, sigma0^2);
* GPU: on cam0 (shipped Stage-3 and a fish-eye variant, Stage-1) and a 2-camera rig --
    [error, xhat, xhatnames] = Buildxhat(data, EXT, INT, TIE, CNT)   bit-exact vs the oracle
    [error, A, misclosure, G, dist_scaling] = BuildAwG(data, xhat)   A per column <= 1e-12, w, G, ds
    RSD = BuildRSD(v, data, xhat)                                    <= 1e-12 (ids, x, y exact)
  and the reference's error behaviour: error = 1 for an invalid Type (BuildAwG.m:209-213), for a
  TIE target missing from CNT (Buildxhat.m:124-128); Num_Radial_Distortions = 0 accepted by Buildxhat
  and BuildRSD as the reference does (an empty K list, Buildxhat.m:71-72, BuildRSD.m:3).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import (ROOT, CAM0_VARIANTS, dist_scaling_of, elem_rel_err, group_rel_err, solver_spread,  # noqa: F401
                      variant_folder)
from flag_masks import REF_TEXT_VARIANTS

STUB = os.path.join(ROOT, "tests", "mexstub")
LIBDIR = os.path.join(ROOT, "fish-eye_bundle_adjustment_amd")
MASKED = REF_TEXT_VARIANTS  # cam0 under mix_a without inner constraints, and under stage2 with them
DROPINS = ("BuildAwG", "Buildxhat", "BuildRSD")


def _build(out):
    stub = os.path.join(out, "libmxstub.so")
    subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", STUB, "-o", stub,
                    os.path.join(STUB, "mxstub.c")], check=True, capture_output=True, text=True)
    libs = {}
    for name in DROPINS + ("fba_mex",):
        so = os.path.join(out, f"{name}_mex.so")
        r = subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", STUB, "-I",
                            os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "mex", f"{name}.c"),
                            "-L", out, "-lmxstub", "-L", LIBDIR, "-lfba", f"-Wl,-rpath,{out}:{LIBDIR}"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        libs[name] = so
    return stub, libs


def test_mex_dropins_build(tmp_path):
    """Source-level drop-ins (MATLAB is not in this image): each compiles with -Wall -Werror against
    the MEX API declarations and include/fba.h and links against libfba.so."""
    _build(str(tmp_path))


class Mx:
    """Builds / reads mxArrays through the stub's own API (ctypes)."""

    def __init__(self, stub):
        L = self.L = C.CDLL(stub, mode=C.RTLD_GLOBAL)
        P, S = C.c_void_p, C.c_size_t
        for n, a, r in [("mxCreateDoubleScalar", [C.c_double], P), ("mxCreateString", [C.c_char_p], P),
                        ("mxCreateDoubleMatrix", [S, S, C.c_int], P), ("mxCreateCellMatrix", [S, S], P),
                        ("mxCreateStructMatrix", [S, S, C.c_int, C.POINTER(C.c_char_p)], P),
                        ("mxSetCell", [P, S, P], None), ("mxSetField", [P, S, C.c_char_p, P], None),
                        ("mxGetDoubles", [P], C.POINTER(C.c_double)), ("mxGetM", [P], S), ("mxGetN", [P], S),
                        ("mxGetCell", [P, S], P), ("mxArrayToString", [P], C.c_void_p), ("mxFree", [P], None),
                        ("mxIsChar", [P], C.c_int), ("mxIsCell", [P], C.c_int), ("mxDestroyArray", [P], None),
                        ("mxstub_call", [P, C.c_int, P, C.c_int, P], C.c_int), ("mxstub_error", [], C.c_char_p),
                        ("mxstub_exit", [], None)]:
            f = getattr(L, n)
            f.argtypes, f.restype = a, r

    def num(self, v):
        return self.L.mxCreateDoubleScalar(float(v))

    def str(self, s):
        return self.L.mxCreateString(str(s).encode())

    def mat(self, a):
        a = np.atleast_2d(np.asarray(a, dtype=np.float64))
        m = self.L.mxCreateDoubleMatrix(a.shape[0], a.shape[1], 0)
        d = self.L.mxGetDoubles(m)
        for i, v in enumerate(a.reshape(-1, order="F")):
            d[i] = v
        return m

    def cell(self, rows, ncol=None):
        M = len(rows)
        N = ncol or max(len(r) for r in rows)
        c = self.L.mxCreateCellMatrix(M, N)
        for i, r in enumerate(rows):
            for j, v in enumerate(r):
                self.L.mxSetCell(c, j * M + i, self.str(v) if isinstance(v, str) else self.num(v))
        return c

    def struct(self, recs):
        """1 x len(recs) struct array; values already mxArrays"""
        names = list(recs[0])
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        s = self.L.mxCreateStructMatrix(1, len(recs), len(names), arr)
        for i, r in enumerate(recs):
            for k, v in r.items():
                self.L.mxSetField(s, i, k.encode(), v)
        return s

    def get(self, a):
        if self.L.mxIsChar(a):
            p = self.L.mxArrayToString(a)
            out = C.cast(p, C.c_char_p).value.decode()
            self.L.mxFree(p)
            return out
        m, n = self.L.mxGetM(a), self.L.mxGetN(a)
        if self.L.mxIsCell(a):
            return [[self.get(self.L.mxGetCell(a, j * m + i)) for j in range(n)] for i in range(m)]
        d = self.L.mxGetDoubles(a)
        return np.array([d[i] for i in range(m * n)]).reshape((m, n), order="F")

    def call(self, fn, nlhs, args):
        plhs = (C.c_void_p * max(nlhs, 1))()
        prhs = (C.c_void_p * len(args))(*args)
        rc = self.L.mxstub_call(C.cast(fn, C.c_void_p), nlhs, plhs, len(args), prhs)
        if rc:
            raise RuntimeError(self.L.mxstub_error().decode())
        return list(plhs)


def data_struct(mx, od):
    """main.m's `data` (settings, points, counts) and EXT / INT / TIE / CNT cells, from the oracle's
    restatement of main.m:60-384 -- the reference's 1-based indices and field names."""
    s = od.settings
    st = {k: (mx.str(v) if isinstance(v, str) else mx.num(v)) for k, v in s.items() if k != "Check_Points"}
    nk = s["Num_Radial_Distortions"]
    pts = []
    for i in range(len(od.x)):
        e, k, t = int(od.ext_index[i]), int(od.cam_num[i]), int(od.tie_index[i])
        io = od.iop_fixed[i]
        b = od.bounds[i]
        r = {"x": mx.num(od.x[i]), "y": mx.num(od.y[i]), "targetID": mx.str(od.target[i]),
             "imageID": mx.str(od.image[i]), "ext_index": mx.num(e + 1), "cameraID": mx.str(od.EXT[e][1])}
        for j, nm in enumerate(("Xc", "Yc", "Zc", "w", "p", "k")):
            r[nm] = mx.num(od.eop_fixed[i, j])
        r.update({"int_index": mx.num(2 * k + 1), "cam_num": mx.num(k + 1), "xp": mx.num(io[0]), "yp": mx.num(io[1]),
                  "c": mx.num(io[2]), "K": mx.mat(np.asarray(io[3:3 + nk]).reshape(-1, 1)),
                  "P": mx.mat(np.asarray(io[3 + nk:5 + nk]).reshape(-1, 1)), "xmin": mx.num(b[1]), "ymin": mx.num(b[2]),
                  "xmax": mx.num(b[3]), "ymax": mx.num(b[4]), "y_dir": mx.num(b[0]), "X": mx.num(od.xyz_fixed[i, 0]),
                  "Y": mx.num(od.xyz_fixed[i, 1]), "Z": mx.num(od.xyz_fixed[i, 2]),
                  "tieIndex": mx.num(t + 1 if t >= 0 else -1), "isTie": mx.num(1 if t >= 0 else 0)})
        pts.append(r)
    data = mx.struct([{"settings": mx.struct([st]), "points": mx.struct(pts), "numImg": mx.num(od.numImg),
                       "numCam": mx.num(od.numCam), "n": mx.num(od.n), "numGCP": mx.num(od.numGCP),
                       "numtie": mx.num(od.numtie)}])
    EXT = mx.cell(od.EXT)
    int_rows = []
    for r in od.INT:
        int_rows.append([r[0], r[1], r[2], r[3], r[4], r[5]])
        int_rows.append(list(r[6]))
    INT = mx.cell(int_rows, ncol=max(6, 5 + nk))
    TIE = mx.cell([[t] for t in od.TIE], ncol=1) if od.TIE else mx.L.mxCreateCellMatrix(0, 1)
    CNT = mx.cell(od.CNT)
    return data, EXT, INT, TIE, CNT


@pytest.fixture(scope="module")
def mexlibs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mex"))
    stub, libs = _build(out)
    mx = Mx(stub)
    fns = {n: getattr(C.CDLL(libs[n]), "mexFunction") for n in DROPINS + ("fba_mex",)}
    yield mx, fns
    mx.L.mxstub_exit()  # mexAtExit: the cached libfba context


def _rig_folder(tmp_path):
    from fba_amd import synth
    return synth.write_folder(synth.generate(14, 200, seed=61, n_cam=2), str(tmp_path / "rig"))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["stage3_pinhole", "stage3_fisheye", "stage1_pinhole", "rig2",
                                     "mix_a_noic_pinhole", "stage2_pinhole"])
def test_mex_dropins_match_oracle(fba, oracle, mexlibs, cam0_folders, tmp_path, variant):
    mx, fns = mexlibs
    if variant in MASKED:  # cam0 under a partial Estimate_* mask (tests/flag_masks.py)
        folder = variant_folder(str(tmp_path), variant, MASKED[variant])
    else:
        folder = _rig_folder(tmp_path) if variant == "rig2" else cam0_folders[variant]
    od = oracle.load_folder(folder)
    data, EXT, INT, TIE, CNT = data_struct(mx, od)
    # Buildxhat
    err, xhat, names = mx.call(fns["Buildxhat"], 3, [data, EXT, INT, TIE, CNT])
    assert mx.get(err)[0, 0] == 0
    x = mx.get(xhat)[:, 0]
    xo, no = oracle.buildxhat(od)
    np.testing.assert_array_equal(x, xo)
    assert [r[0] for r in mx.get(names)] == no
    if variant in MASKED:  # the partial layouts: 4 of 6 EOPs and xp, c, p1, p2 / all six EOPs and xp, yp, c
        assert oracle.counts(od.settings) == {"mix_a_noic_pinhole": (4, 4), "stage2_pinhole": (6, 3)}[variant]
    # BuildAwG at the start values and at a perturbed xhat
    rng = np.random.default_rng(3)
    for xv in (xo, xo * (1 + 1e-4 * rng.standard_normal(len(xo)))):
        out = mx.call(fns["BuildAwG"], 5, [data, mx.mat(xv.reshape(-1, 1))])
        e, A, w, G, ds = (mx.get(o) for o in out)
        assert e[0, 0] == 0
        Ao, wo, Go, dso = oracle.build_awg(od, xv)
        colmax = np.maximum(np.abs(Ao).max(axis=0), 1e-300)
        assert (np.abs(A - Ao).max(axis=0) / colmax).max() <= 1e-12
        assert np.abs(w[:, 0] - wo).max() <= 1e-12 * np.abs(od.x).max()
        if Go is None:
            assert G.shape == (1, 1) and G[0, 0] == 0  # BuildAwG.m:38: G = 0 without inner constraints
        else:
            np.testing.assert_allclose(G, Go, rtol=1e-14, atol=1e-14 * np.abs(Go).max())
        np.testing.assert_allclose(ds, dso, rtol=1e-14)
        if variant in MASKED:  # the compact n x u A; the index columns of dist_scaling exactly
            assert A.shape == Ao.shape and np.array_equal(ds[:, :2], dso[:, :2])
    # BuildRSD with the oracle's final v and xhat (main.m:569-571)
    ro = oracle.adjust(od)
    rsd = mx.get(mx.call(fns["BuildRSD"], 1, [mx.mat(ro.v.reshape(-1, 1)), data, mx.mat(ro.xhat.reshape(-1, 1))])[0])
    assert [r[0] for r in rsd] == od.target and [r[1] for r in rsd] == od.image
    assert np.array_equal(np.array([[r[2][0, 0], r[3][0, 0]] for r in rsd]), np.column_stack([od.x, od.y]))
    num = np.array([[v[0, 0] for v in r[4:]] for r in rsd])
    ref = oracle.build_rsd(od, ro.v, ro.xhat)
    assert np.abs(num - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.gpu
def test_mex_dropins_error_behaviour(fba, oracle, mexlibs, cam0_folders):
    """error = 1 and empty outputs where the reference sets error = 1: an invalid Type in BuildAwG
    (BuildAwG.m:209-213), a TIE target missing from CNT in Buildxhat (Buildxhat.m:124-128)."""
    mx, fns = mexlibs
    od = oracle.load_folder(cam0_folders["stage3_pinhole"])
    xo, _ = oracle.buildxhat(od)
    od.settings["type"] = "spherical"
    data, EXT, INT, TIE, CNT = data_struct(mx, od)
    out = [mx.get(o) for o in mx.call(fns["BuildAwG"], 5, [data, mx.mat(xo.reshape(-1, 1))])]
    assert out[0][0, 0] == 1 and out[1].size == 0
    od.settings["type"] = "pinhole"
    od.TIE = list(od.TIE[:-1]) + ["NOT_IN_CNT"]
    data, EXT, INT, TIE, CNT = data_struct(mx, od)
    err, xhat, names = (mx.get(o) for o in mx.call(fns["Buildxhat"], 3, [data, EXT, INT, TIE, CNT]))
    assert err[0, 0] == 1 and xhat.size == 0


def _mex_adjust(mx, fns, od, nlhs=9):
    data, EXT, INT, TIE, CNT = data_struct(mx, od)
    out = mx.call(fns["fba_mex"], nlhs, [data, EXT, INT, TIE, CNT])
    assert mx.get(out[0])[0, 0] == 0
    return out


@pytest.mark.gpu
def test_mex_whole_loop_matches_oracle_cam0(fba, oracle, mexlibs, cam0_folders):
    """fba_mex(data, EXT, INT, TIE, CNT) -- main.m:386-602 from what main.m holds at line 386 -- on the
    shipped cam0 Stage-3 (pinhole, inner constraints, tie points, 3 control points) against the dense
    oracle: same count, the deltasum history, xhat per element <= 1e-9, v, the RSD cell, RMS, sigma0^2
    <= 1e-9, diag(Cx) and the EOP/IOP correlation blocks (main.m:446-482, :602) <= 1e-7."""
    _whole_loop_cam0(fba, oracle, mexlibs, cam0_folders["stage3_pinhole"])


@pytest.mark.gpu
def test_mex_whole_loop_matches_oracle_cam0_mix_a(fba, oracle, mexlibs, tmp_path):
    """The same gateway and assertions on cam0 under the mixed mask mix_a (Omega, Zc, yp, radial off) without
    inner constraints: the gateway's xhat, cx_diag and corr have the compressed lengths u = 490 and
    u_img + u_cam = 4 + 4 (restatement spread on this variant <= 1.3e-11 per element, so 1e-9 holds)."""
    folder = variant_folder(str(tmp_path), "mix_a", MASKED["mix_a_noic_pinhole"])
    _whole_loop_cam0(fba, oracle, mexlibs, folder, u=490, mu=8)


def _whole_loop_cam0(fba, oracle, mexlibs, folder, u=None, mu=None):
    mx, fns = mexlibs
    od = oracle.load_folder(folder)
    ro = oracle.adjust(od)
    _, xhat, count, dsum, v, rsd, st, cxd, corr = _mex_adjust(mx, fns, od)
    if u is not None:
        assert mx.get(xhat).shape == (u, 1) == mx.get(cxd).shape and sum(oracle.counts(od.settings)) == mu
    assert mx.get(count)[0, 0] == ro.iterations
    # the deltasum history: the gateway runs the library's loop (fba_adjust), so the Python mirror's to
    # rounding; against the oracle the first pass at 1e-9 or 20x the restatements' own spread, the bound
    # test_gpu_parity.test_adjust_cam0 holds the library to (this scene's first Sigma|delta| moves by ~7e-9
    # between exact restatements: inner constraints + control points; the later passes are differences of
    # nearly equal iterates)
    d = mx.get(dsum)[0]
    lib = fba.adjust(fba.load_folder(folder), covariance=False).deltasum
    np.testing.assert_allclose(d, lib, rtol=0, atol=1e-12 * ro.deltasum[0])
    spread = solver_spread(oracle, od, ro)
    assert abs(d[0] - ro.deltasum[0]) <= max(1e-9, 20 * spread["deltasum0"]) * ro.deltasum[0], spread["deltasum0"]
    x = mx.get(xhat)[:, 0]
    for err in (group_rel_err(x, ro.xhat, ro.names, ro.dist_scaling), elem_rel_err(x, ro.xhat, ro.names, ro.dist_scaling)):
        assert max(err.values()) <= 1e-9, err
    st = mx.get(st)[:, 0]
    assert abs(st[3] - ro.sigma02) <= 1e-9 * ro.sigma02
    np.testing.assert_allclose(st[:3], ro.rms, rtol=1e-9)
    assert np.abs(mx.get(v)[:, 0] - ro.v).max() <= 1e-8 * np.abs(ro.v).max()
    cells = mx.get(rsd)
    assert [r[0] for r in cells] == od.target and [r[1] for r in cells] == od.image
    num = np.array([[c[0, 0] for c in r[4:]] for r in cells])
    assert np.abs(num - ro.rsd).max() <= 1e-8 * np.abs(ro.rsd).max()
    cdo, corro = oracle.covariance(od, ro)
    np.testing.assert_allclose(mx.get(cxd)[:, 0], cdo, rtol=1e-7)
    # corr: mu x mu x numImg (mxCreateNumericArray; the stub stores dims[0] x prod(dims[1:]))
    u_img, u_cam = oracle.counts(od.settings)
    mu = u_img + u_cam
    cr = mx.get(corr).reshape(mu, mu, od.numImg, order="F")
    for e in range(0, od.numImg, 7):
        idx = list(range(e * u_img, (e + 1) * u_img))
        k = int(od.cam_num[np.nonzero(od.ext_index == e)[0][0]])
        idx += list(range(u_img * od.numImg + k * u_cam, u_img * od.numImg + (k + 1) * u_cam))
        np.testing.assert_allclose(cr[:, :, e], corro[np.ix_(idx, idx)], rtol=0, atol=1e-7)


@pytest.mark.gpu
def test_mex_whole_loop_matches_oracle_config3(fba, oracle, mexlibs, tmp_path):
    """The same gateway at BASELINE.json config 3 (200 images x 5,000 tie points, 50k image points,
    fish-eye, free network) against oracle/fba_cpu.c solving the reference's bordered system [S G; G' 0]
    directly: count, xhat per element and per group <= 1e-9, sigma0^2 <= 1e-9."""
    import fba_cpu
    from fba_amd import synth
    mx, fns = mexlibs
    folder = synth.make_config(3, str(tmp_path / "c3"))
    od = oracle.load_folder(folder)
    ref = fba_cpu.CpuAdjustment(od, solver="kkt")
    it = ref.adjust()
    _, s02 = ref.residuals()
    ref.close()
    _, xhat, count, dsum, v, rsd, st = _mex_adjust(mx, fns, od, nlhs=7)
    assert mx.get(count)[0, 0] == it
    x = mx.get(xhat)[:, 0]
    dsc = dist_scaling_of(od)
    for err in (group_rel_err(x, ref.xhat, ref.names, dsc), elem_rel_err(x, ref.xhat, ref.names, dsc)):
        assert max(err.values()) <= 1e-9, err
    assert abs(mx.get(st)[3, 0] - s02) <= 1e-9 * s02


@pytest.mark.gpu
def test_mex_nk0_buildxhat_buildrsd(fba, oracle, mexlibs, tmp_path):
    """Num_Radial_Distortions = 0: the reference's Buildxhat lays out no K (an empty list,
    Buildxhat.m:71-72; INT row 2 is xp yp c P1 P2) and BuildRSD counts none (BuildRSD.m:3) -- both drop-ins
    follow it (only BuildAwG clamps its local copy to 1, BuildAwG.m:18-20); the whole-loop gateway
    rejects the combination with Estimate_Radial_Distortions = 1 (error = 1), where the reference's
    xhat + delta would not conform."""
    mx, fns = mexlibs
    folder = variant_folder(str(tmp_path), "nk0", {"Num_Radial_Distortions": "0"})
    od = oracle.load_folder(folder)
    assert od.settings["Num_Radial_Distortions"] == 0
    data, EXT, INT, TIE, CNT = data_struct(mx, od)
    err, xhat, names = mx.call(fns["Buildxhat"], 3, [data, EXT, INT, TIE, CNT])
    assert mx.get(err)[0, 0] == 0
    xo, no = oracle.buildxhat(od)
    np.testing.assert_array_equal(mx.get(xhat)[:, 0], xo)
    assert [r[0] for r in mx.get(names)] == no and not any(n.startswith("k1_") for n in no)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(2 * len(od.x))
    rsd = mx.get(mx.call(fns["BuildRSD"], 1, [mx.mat(v.reshape(-1, 1)), data, mx.mat(xo.reshape(-1, 1))])[0])
    num = np.array([[c[0, 0] for c in r[4:]] for r in rsd])
    ref = oracle.build_rsd(od, v, xo)
    assert np.abs(num - ref).max() <= 1e-12 * np.abs(ref).max()
    out = mx.call(fns["fba_mex"], 2, [data, EXT, INT, TIE, CNT])
    assert mx.get(out[0])[0, 0] == 1 and mx.get(out[1]).size == 0
