"""ctypes binding of libfba.so (include/fba.h).

The shared library is built in-tree (``make -C fish-eye_bundle_adjustment_amd/csrc`` or
``__graft_entry__.build()``).  There is no fallback: if the library is missing or fails to load,
importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfba.so")

TYPES = ("fisheye", "pinhole", "equisolid", "orthographic", "stereographic")
LOSSES = ("none", "huber", "cauchy")  # FBA_LOSS_*
# the usual 95 %-efficiency tuning constants (in units of sigma)
LOSS_K = {"huber": 1.345, "cauchy": 2.385}
NK_MAX = 8
RAY_STATUS = ("ok", "domain")                    # FBA_RAY_*
ISECT_STATUS = ("ok", "few", "weak", "refine")   # FBA_ISECT_*
RESECT_STATUS = ("ok", "few", "weak", "refine")  # FBA_RESECT_*
RESECT_USE = ("control", "all")                  # FBA_RESECT_USE_*
VCE_STATUS = ("ok", "empty", "weak", "clipped")  # FBA_VCE_*
SNOOP_STATE = ("active", "excluded", "readmitted")  # fba_snoop's excluded[] on exit
VCE_MAX_GROUPS = 256                             # FBA_VCE_MAX_GROUPS

# every symbol include/fba.h declares
EXPORTS = (
    "fba_last_error", "fba_abi_version", "fba_count_unknowns", "fba_partition", "fba_image_order", "fba_create",
    "fba_create_priors", "fba_get_priors", "fba_destroy", "fba_solve_mode", "fba_buildxhat", "fba_set_xhat", "fba_get_xhat", "fba_build_awg",
    "fba_accumulate", "fba_reduce_buffer", "fba_synchronize", "fba_solve_update", "fba_solve_update_async",
    "fba_deltasum_device", "fba_solve_finish", "fba_step", "fba_adjust",
    "fba_residuals", "fba_build_rsd", "fba_finish_stats", "fba_covariance", "fba_reliability",
    "fba_set_weights", "fba_set_loss", "fba_get_weights", "fba_last_timings", "fba_set_timing", "fba_set_probe",
    "fba_probe_stats", "fba_set_spin_bound", "fba_test_border_solve", "fba_test_live_allocations",
    "fba_set_damping", "fba_cost", "fba_adjust_lm",
    "fba_postfit_outputs",
    "fba_unproject_host", "fba_image_rays", "fba_intersect",
    "fba_resect", "fba_resect_host",
    "fba_vce", "fba_vce_host",
    "fba_snoop", "fba_snoop_host",
)
# ... but for the host-only helpers whose names carry a digit (tests/test_damping_host.py reads the header's
# declarations with a letters-only pattern and compares them with EXPORTS)
HOST_EXPORTS = ("fba_eig3_host",)


class FBAError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fba error {code}: {msg}")
        self.code = code


class Settings(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "est_Xc", "est_Yc", "est_Zc", "est_omega", "est_phi", "est_kappa", "est_xp", "est_yp", "est_c",
        "est_radial", "est_decent", "num_radial", "type", "inner_constraints", "iteration_cap", "reserved")] + [
        ("threshold", C.c_double), ("meas_std_x", C.c_double), ("meas_std_y", C.c_double)]


class Problem(C.Structure):
    _fields_ = [("n_pts", C.c_int64), ("n_img", C.c_int32), ("n_cam", C.c_int32), ("n_tie", C.c_int32),
                ("reserved", C.c_int32), ("xy", C.c_void_p), ("img", C.c_void_p), ("cam", C.c_void_p),
                ("tie", C.c_void_p), ("xyz_fixed", C.c_void_p), ("eop0", C.c_void_p), ("iop0", C.c_void_p),
                ("cam_info", C.c_void_p), ("tie0", C.c_void_p)]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("verbose", C.c_int32),
                ("stream", C.c_void_p), ("split", C.c_int32)]


class Priors(C.Structure):
    _fields_ = [("n", C.c_int64), ("index", C.c_void_p), ("value", C.c_void_p), ("sigma", C.c_void_p)]


class Postfit(C.Structure):
    """fba_postfit: the output pointers of fba_postfit_outputs, any of them NULL"""
    _fields_ = [(n, C.c_void_p) for n in ("cx_diag", "corr", "redundancy", "wstat", "cx_tie", "ellipsoid")]


class LMOptions(C.Structure):
    """fba_lm_options; the defaults are the library's (a NULL pointer)"""
    _fields_ = [(n, C.c_double) for n in ("lambda0", "up", "down", "lambda_min", "lambda_max", "ftol")]

    def __init__(self, lambda0=1e-3, up=10.0, down=10.0, lambda_min=1e-12, lambda_max=1e8, ftol=1e-9):
        super().__init__(lambda0, up, down, lambda_min, lambda_max, ftol)


class IntersectOptions(C.Structure):
    """fba_intersect_options; the defaults are the library's (a NULL pointer)"""
    _fields_ = [("refine_iters", C.c_int32), ("write_xhat", C.c_int32), ("min_ratio", C.c_double),
                ("refine_tol", C.c_double)]

    def __init__(self, refine_iters=10, write_xhat=False, min_ratio=0.5 * (1.0 - np.cos(np.pi / 180.0)),
                 refine_tol=1e-10):
        super().__init__(int(refine_iters), int(bool(write_xhat)), float(min_ratio), float(refine_tol))


class ResectOptions(C.Structure):
    """fba_resect_options; the defaults are the library's (a NULL pointer).  use: "control", "all" or the
    FBA_RESECT_USE_* number"""
    _fields_ = [("use", C.c_int32), ("refine_iters", C.c_int32), ("write_xhat", C.c_int32), ("reserved", C.c_int32),
                ("min_ratio", C.c_double), ("refine_tol", C.c_double)]

    def __init__(self, use="control", refine_iters=10, write_xhat=False, min_ratio=1e-6, refine_tol=1e-10):
        if isinstance(use, str):
            if use.lower() not in RESECT_USE:
                raise ValueError(f"resect: unknown use {use!r} (one of {', '.join(RESECT_USE)})")
            use = RESECT_USE.index(use.lower())
        super().__init__(int(use), int(refine_iters), int(bool(write_xhat)), 0, float(min_ratio), float(refine_tol))


class VceOptions(C.Structure):
    """fba_vce_options; the defaults are the library's (a NULL pointer)"""
    _fields_ = [("max_rounds", C.c_int32), ("reserved", C.c_int32), ("tol", C.c_double),
                ("min_redundancy", C.c_double), ("clip", C.c_double)]

    def __init__(self, max_rounds=10, tol=1e-3, min_redundancy=1.0, clip=100.0):
        super().__init__(int(max_rounds), 0, float(tol), float(min_redundancy), float(clip))


class SnoopOptions(C.Structure):
    """fba_snoop_options; the defaults are the library's (a NULL pointer)"""
    _fields_ = [("max_rounds", C.c_int32), ("min_rays", C.c_int32), ("min_img_points", C.c_int32), ("reserved", C.c_int32),
                ("crit", C.c_double), ("max_share", C.c_double)]

    def __init__(self, max_rounds=20, min_rays=2, min_img_points=6, crit=3.29, max_share=0.05):
        super().__init__(int(max_rounds), int(min_rays), int(min_img_points), 0, float(crit), float(max_share))


def _given(**kw):
    """the keywords a caller gave (not None): the *Options classes above hold the defaults of the others"""
    return {k: v for k, v in kw.items() if v is not None}


def pack_priors(priors):
    """(index, value, sigma) -> (fba_priors, the arrays it points into), or (None, None) for None / no rows.
    Shapes only: the values are checked by fba_create_priors, on the host, before it touches the GPU."""
    if priors is None:
        return None, None
    index, value, sigma = priors
    index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
    value = np.ascontiguousarray(value, dtype=np.float64).reshape(-1)
    sigma = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
    if not (index.size == value.size == sigma.size):
        raise ValueError("priors: index, value and sigma must have the same length")
    if index.size == 0:
        return None, None
    return Priors(index.size, ptr(index).value, ptr(value).value, ptr(sigma).value), (index, value, sigma)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is not built: run `make -C {os.path.join(_HERE, 'csrc')}` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    sig = {
        "fba_last_error": ([], C.c_char_p),
        "fba_abi_version": ([], C.c_int),
        "fba_count_unknowns": ([P, P, P], C.c_int),
        "fba_partition": ([P, I, P, P], C.c_int),
        "fba_image_order": ([P, P, P], C.c_int),
        "fba_create": ([P, P, P, P], C.c_int),
        "fba_create_priors": ([P, P, P, P, P], C.c_int),
        "fba_get_priors": ([P, P, P, P], C.c_int),
        "fba_destroy": ([P], None),
        "fba_solve_mode": ([P, P], C.c_int),
        "fba_buildxhat": ([P, P, P], C.c_int),
        "fba_set_xhat": ([P, P], C.c_int),
        "fba_get_xhat": ([P, P, I], C.c_int),
        "fba_build_awg": ([P, P, P, P, P, P], C.c_int),
        "fba_accumulate": ([P], C.c_int),
        "fba_reduce_buffer": ([P, P, P], C.c_int),
        "fba_synchronize": ([P], C.c_int),
        "fba_solve_update": ([P, P], C.c_int),
        "fba_solve_update_async": ([P], C.c_int),
        "fba_deltasum_device": ([P, P], C.c_int),
        "fba_solve_finish": ([P, P], C.c_int),
        "fba_step": ([P, P], C.c_int),
        "fba_build_rsd": ([P, P, P, P], C.c_int),
        "fba_adjust": ([P, P, P], C.c_int),
        "fba_residuals": ([P, P, P, P], C.c_int),
        "fba_finish_stats": ([P, P, P, D, P], C.c_int),
        "fba_covariance": ([P, D, P, P], C.c_int),
        "fba_reliability": ([P, D, P, P, P, P], C.c_int),
        "fba_set_weights": ([P, P], C.c_int),
        "fba_set_loss": ([P, I, D], C.c_int),
        "fba_get_weights": ([P, P], C.c_int),
        "fba_last_timings": ([P, P], C.c_int),
        "fba_set_timing": ([P, I], C.c_int),
        "fba_set_probe": ([P, I], C.c_int),
        "fba_probe_stats": ([P, P], C.c_int),
        "fba_set_spin_bound": ([P, C.c_int64], C.c_int),
        "fba_test_border_solve": ([I, P, P], C.c_int),
        "fba_test_live_allocations": ([P], C.c_int),
        "fba_set_damping": ([P, D], C.c_int),
        "fba_cost": ([P, P], C.c_int),
        "fba_adjust_lm": ([P, P, P, P, P], C.c_int),
        "fba_postfit_outputs": ([P, D, P], C.c_int),
        "fba_eig3_host": ([C.c_int64, P, P], C.c_int),
        "fba_unproject_host": ([I, I, C.c_int64, P, P, P, P], C.c_int),
        "fba_image_rays": ([P, P, P], C.c_int),
        "fba_intersect": ([P, P, P, P, P, P], C.c_int),
        "fba_resect": ([P, P, P, P, P, P], C.c_int),
        "fba_resect_host": ([I, C.c_int64, P, P, P, D, D, D, D, P, P, P, P], C.c_int),
        "fba_vce": ([P, I, P, P, P, P, P, P, P, P], C.c_int),
        "fba_vce_host": ([C.c_int64, I, P, P, P, P, P, P, P, P], C.c_int),
        "fba_snoop": ([P, P, P, P, P, P, P, P, P], C.c_int),
        "fba_snoop_host": ([C.c_int64, P, P, P, P, I, I, P, P, P, P], C.c_int),
    }
    for name, (args, res) in sig.items():
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    return lib


lib = _load()


def last_error() -> str:
    return lib.fba_last_error().decode(errors="replace")


def check(rc: int):
    if rc != 0:
        raise FBAError(rc, last_error())


def ptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"] or a.flags["F_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class PackedProblem:
    """Owns the numpy arrays a ``fba_problem`` points into."""

    def __init__(self, xy, img, cam, tie, xyz_fixed, eop0, iop0, cam_info, tie0, n_img, n_cam, n_tie):
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        self.img = np.ascontiguousarray(img, dtype=np.int32)
        self.cam = np.ascontiguousarray(cam, dtype=np.int32)
        self.tie = np.ascontiguousarray(tie, dtype=np.int32)
        self.xyz_fixed = np.ascontiguousarray(xyz_fixed, dtype=np.float64).reshape(-1)
        self.eop0 = np.ascontiguousarray(eop0, dtype=np.float64).reshape(-1)
        self.iop0 = np.ascontiguousarray(iop0, dtype=np.float64).reshape(-1)
        self.cam_info = np.ascontiguousarray(cam_info, dtype=np.float64).reshape(-1)
        self.tie0 = np.ascontiguousarray(tie0, dtype=np.float64).reshape(-1)
        self.n_pts = len(self.img)
        self.n_img, self.n_cam, self.n_tie = int(n_img), int(n_cam), int(n_tie)
        self.struct = Problem(self.n_pts, self.n_img, self.n_cam, self.n_tie, 0, ptr(self.xy).value,
                              ptr(self.img).value, ptr(self.cam).value, ptr(self.tie).value,
                              ptr(self.xyz_fixed).value, ptr(self.eop0).value, ptr(self.iop0).value,
                              ptr(self.cam_info).value, ptr(self.tie0).value)


def make_settings(s: dict) -> Settings:
    """From the reference's data.settings field names (main.m:112-171)."""
    nk = int(s["Num_Radial_Distortions"])
    if s["type"] not in TYPES:
        raise FBAError(2, "BuildAwG, invalid type in data.settings.type")
    return Settings(int(s["Estimate_Xc"]), int(s["Estimate_Yc"]), int(s["Estimate_Zc"]), int(s["Estimate_w"]),
                    int(s["Estimate_p"]), int(s["Estimate_k"]), int(s["Estimate_xp"]), int(s["Estimate_yp"]),
                    int(s["Estimate_c"]), int(s["Estimate_radial"]), int(s["Estimate_decent"]), nk,
                    TYPES.index(s["type"]), int(s["Inner_Constraints"]), int(s["Iteration_Cap"]), 0,
                    float(s["threshold"]), float(s["Meas_std"]), float(s["Meas_std_y"]))


class Context:
    """One device-resident adjustment (one GPU / one rank)."""

    def __init__(self, packed: PackedProblem, settings: Settings, device=0, rank=0, world=1, stream=None,
                 verbose=False, split=False, priors=None):
        """priors: (index, value, sigma) -- prior observations of unknowns, index into the reference-layout xhat
        (fba_create_priors); None, or no rows, is fba_create."""
        self.packed = packed
        self.settings = settings
        self.world = world
        opts = Options(device, rank, world, int(verbose), stream, int(bool(split)))
        h = C.c_void_p()
        pr, self.priors = pack_priors(priors)
        if pr is None:
            check(lib.fba_create(C.byref(packed.struct), C.byref(settings), C.byref(opts), C.byref(h)))
        else:
            check(lib.fba_create_priors(C.byref(packed.struct), C.byref(settings), C.byref(opts), C.byref(pr),
                                        C.byref(h)))
        self.h = h
        # the solve libfba runs: a split request falls back to the replicated solve when the block
        # pattern cannot be cut (fba_solve_mode)
        mode = C.c_int32()
        check(lib.fba_solve_mode(self.h, C.byref(mode)))
        self.split = bool(mode.value)
        u = C.c_int64()
        check(lib.fba_buildxhat(self.h, None, C.byref(u)))
        self.u = u.value

    def close(self):
        if getattr(self, "h", None):
            lib.fba_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def buildxhat(self):
        x = np.zeros(self.u)
        check(lib.fba_buildxhat(self.h, ptr(x), None))
        return x

    def set_xhat(self, xhat):
        x = np.ascontiguousarray(xhat, dtype=np.float64)
        check(lib.fba_set_xhat(self.h, ptr(x)))

    def get_xhat(self, owned_only=False):
        x = np.zeros(self.u)
        check(lib.fba_get_xhat(self.h, ptr(x), int(owned_only)))
        return x

    def build_awg(self, xhat=None, dense=True):
        n = 2 * self.packed.n_pts
        A = np.zeros((n, self.u), order="F") if dense else None
        w = np.zeros(n)
        G = np.zeros((self.u, 7), order="F") if self.settings.inner_constraints else None
        ds = np.zeros((self.packed.n_cam, 2 + self.settings.num_radial), order="F")
        x = None if xhat is None else np.ascontiguousarray(xhat, dtype=np.float64)
        check(lib.fba_build_awg(self.h, ptr(x), ptr(A), ptr(w), ptr(G), ptr(ds)))
        return A, w, G, ds

    def accumulate(self):
        check(lib.fba_accumulate(self.h))

    def reduce_buffer(self):
        p, n = C.c_void_p(), C.c_int64()
        check(lib.fba_reduce_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def synchronize(self):
        check(lib.fba_synchronize(self.h))

    def solve_update(self):
        d = C.c_double()
        check(lib.fba_solve_update(self.h, C.byref(d)))
        return d.value

    def solve_update_async(self):
        check(lib.fba_solve_update_async(self.h))

    def deltasum_device(self):
        p = C.c_void_p()
        check(lib.fba_deltasum_device(self.h, C.byref(p)))
        return p.value

    def solve_finish(self):
        d = C.c_double()
        check(lib.fba_solve_finish(self.h, C.byref(d)))
        return d.value

    def step(self):
        d = C.c_double()
        check(lib.fba_step(self.h, C.byref(d)))
        return d.value

    def adjust(self):
        cap = max(int(self.settings.iteration_cap), 1)
        hist = np.zeros(cap)
        it = C.c_int32()
        check(lib.fba_adjust(self.h, C.byref(it), ptr(hist)))
        return it.value, hist[: it.value].copy()

    def set_damping(self, lam=0.0):
        """fba_set_damping: Levenberg-Marquardt parameter of every following solve; 0 is Gauss-Newton"""
        check(lib.fba_set_damping(self.h, float(lam)))

    def cost(self):
        """fba_cost: (total, image part, prior part) of the objective at the device xhat"""
        out = np.zeros(3)
        check(lib.fba_cost(self.h, ptr(out)))
        return out

    def adjust_lm(self, options=None):
        """fba_adjust_lm: (trials, polish passes, history) -- history has one row per trial and pass:
        lambda, cost after it, deltasum, accepted.  options: an LMOptions, a dict of its fields, or None."""
        if isinstance(options, dict):
            options = LMOptions(**options)
        cap = max(int(self.settings.iteration_cap), 1)
        hist = np.full((cap, 4), np.nan)
        nt, npol = C.c_int32(), C.c_int32()
        check(lib.fba_adjust_lm(self.h, None if options is None else C.byref(options), C.byref(nt), C.byref(npol),
                                ptr(hist)))
        return nt.value, npol.value, hist[: nt.value + npol.value].copy()

    def residuals(self):
        n = self.packed.n_pts
        v = np.zeros(2 * n)
        rsd = np.zeros((n, 5))
        st = np.zeros(6)
        check(lib.fba_residuals(self.h, ptr(v), ptr(rsd), ptr(st)))
        return v, rsd, st

    def build_rsd(self, v, xhat):
        """fba_build_rsd: BuildRSD.m rows [r, vx, vy, vr, vt] for a given v (PHO order) and xhat."""
        n = self.packed.n_pts
        v = np.ascontiguousarray(v, dtype=np.float64)
        x = np.ascontiguousarray(xhat, dtype=np.float64)
        if v.size != 2 * n or x.size != int(self.u):
            raise ValueError("BuildRSD: v must have 2*n_pts entries and xhat u entries")
        rsd = np.zeros((n, 5))
        check(lib.fba_build_rsd(self.h, ptr(v), ptr(x), ptr(rsd)))
        return rsd

    def covariance(self, sigma02, corr=True):
        """fba_covariance: diag of the reference's final Cx (main.m:428-482, :602) in xhat order, and
        per EXT image the Correlation sub-matrix over [its estimated EOPs, its camera's estimated
        IOPs] (main.m:446-456, :831-840), shape (n_img, u_img + u_cam, u_img + u_cam)."""
        st = self.settings
        u_img = sum(int(x) for x in (st.est_Xc, st.est_Yc, st.est_Zc, st.est_omega, st.est_phi, st.est_kappa))
        u_cam = (int(st.est_xp) + int(st.est_yp) + int(st.est_c) + int(st.est_radial) * int(st.num_radial)
                 + 2 * int(st.est_decent))
        mu = u_img + u_cam
        d = np.zeros(max(int(self.u), 1))
        cr = np.zeros((max(self.packed.n_img, 1), mu, mu)) if corr else None
        check(lib.fba_covariance(self.h, float(sigma02), ptr(d), ptr(cr)))
        return d[: int(self.u)], (cr[: self.packed.n_img] if corr else None)

    def reliability(self, sigma02, corr=True):
        """fba_reliability: (cx_diag, corr, redundancy, wstat) -- covariance()'s two outputs, bit-identical, and
        per image measurement (PHO order, x y interleaved like v) Baarda's redundancy number r = 1 - p a Cx a'
        and the standardised residual w = v / (sigma sqrt(r)).  Consumes the factor like covariance(): call
        one of the two."""
        st = self.settings
        u_img = sum(int(x) for x in (st.est_Xc, st.est_Yc, st.est_Zc, st.est_omega, st.est_phi, st.est_kappa))
        u_cam = (int(st.est_xp) + int(st.est_yp) + int(st.est_c) + int(st.est_radial) * int(st.num_radial)
                 + 2 * int(st.est_decent))
        mu = u_img + u_cam
        n = self.packed.n_pts
        d = np.zeros(max(int(self.u), 1))
        cr = np.zeros((max(self.packed.n_img, 1), mu, mu)) if corr else None
        red, wst = np.zeros(max(2 * n, 1)), np.zeros(max(2 * n, 1))
        check(lib.fba_reliability(self.h, float(sigma02), ptr(d), ptr(cr), ptr(red), ptr(wst)))
        return d[: int(self.u)], (cr[: self.packed.n_img] if corr else None), red[: 2 * n], wst[: 2 * n]

    def postfit(self, sigma02, reliability=False, tie_cov=True, ellipsoids=True, corr=True):
        """fba_postfit_outputs: (cx_diag, corr, redundancy, wstat, cx_tie, ellipsoid) in one call on one selected
        inverse -- the first four exactly covariance()'s / reliability()'s (redundancy and wstat None without
        reliability=True), cx_tie (n_tie, 6): XX XY XZ YY YZ ZZ of every tie point's block of the final Cx, ellipsoid
        (n_tie, 12): the 1-sigma semi-axes a >= b >= c and the three unit axis vectors as rows, TIE order; None
        where not asked for.  Consumes the factor like covariance(): call one of the three."""
        st = self.settings
        u_img = sum(int(x) for x in (st.est_Xc, st.est_Yc, st.est_Zc, st.est_omega, st.est_phi, st.est_kappa))
        u_cam = (int(st.est_xp) + int(st.est_yp) + int(st.est_c) + int(st.est_radial) * int(st.num_radial)
                 + 2 * int(st.est_decent))
        mu = u_img + u_cam
        n, nt = self.packed.n_pts, self.packed.n_tie
        d = np.zeros(max(int(self.u), 1))
        cr = np.zeros((max(self.packed.n_img, 1), mu, mu)) if corr else None
        red = np.zeros(max(2 * n, 1)) if reliability else None
        wst = np.zeros(max(2 * n, 1)) if reliability else None
        blk = np.zeros((max(nt, 1), 6)) if tie_cov else None
        ell = np.zeros((max(nt, 1), 12)) if ellipsoids else None
        out = Postfit(*[None if a is None else ptr(a).value for a in (d, cr, red, wst, blk, ell)])
        check(lib.fba_postfit_outputs(self.h, float(sigma02), C.byref(out)))
        return (d[: int(self.u)], (cr[: self.packed.n_img] if corr else None),
                (red[: 2 * n] if reliability else None), (wst[: 2 * n] if reliability else None),
                (blk[:nt] if tie_cov else None), (ell[:nt] if ellipsoids else None))

    def set_weights(self, weights=None):
        """fba_set_weights: per-measurement multipliers of the a-priori weight, (2 n_pts) in PHO order, x y
        interleaved like v (or (n_pts, 2)); None restores all 1.  Entries must be finite and > 0."""
        if weights is None:
            check(lib.fba_set_weights(self.h, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != 2 * self.packed.n_pts:
            raise ValueError("set_weights: weights must have 2*n_pts entries")
        check(lib.fba_set_weights(self.h, ptr(w)))

    def set_loss(self, loss="none", k=None):
        """fba_set_loss: "none", "huber" or "cauchy" (or the FBA_LOSS_* number); k in units of sigma, by
        default the 95 %-efficiency constant of the loss (LOSS_K)."""
        if isinstance(loss, str):
            if loss.lower() not in LOSSES:
                raise ValueError(f"set_loss: unknown loss {loss!r} (one of {', '.join(LOSSES)})")
            loss = LOSSES.index(loss.lower())
        if k is None:
            k = LOSS_K.get(LOSSES[loss], 0.0) if 0 <= int(loss) < len(LOSSES) else 0.0
        check(lib.fba_set_loss(self.h, int(loss), float(k)))

    def get_weights(self):
        """fba_get_weights: the effective weights (user weight x loss factor) at the last linearisation point,
        (2 n_pts) in PHO order; other ranks' observations are 0."""
        w = np.zeros(max(2 * self.packed.n_pts, 1))
        check(lib.fba_get_weights(self.h, ptr(w)))
        return w[: 2 * self.packed.n_pts]

    def get_priors(self):
        """fba_get_priors: (resid, vtpv) -- the priors' residuals xhat[index] - value at the device xhat, in the
        order they were given (0 for the priors another rank adds), and this rank's sum of p v^2"""
        n = 0 if self.priors is None else self.priors[0].size
        resid, vtpv = np.zeros(max(n, 1)), C.c_double()
        check(lib.fba_get_priors(self.h, None, ptr(resid), C.byref(vtpv)))
        return resid[:n], vtpv.value

    def image_rays(self):
        """fba_image_rays: (ray, status) -- per PHO row the projection centre and the unit direction of the
        measurement's image ray in the object frame, (n_pts, 6), and FBA_RAY_* (n_pts), at the device xhat;
        other ranks' observations are 0."""
        n = self.packed.n_pts
        ray, st = np.zeros((max(n, 1), 6)), np.zeros(max(n, 1), dtype=np.int32)
        check(lib.fba_image_rays(self.h, ptr(ray), ptr(st)))
        return ray[:n], st[:n]

    def intersect(self, refine_iters=None, write_xhat=None, min_ratio=None, refine_tol=None):
        """fba_intersect: (xyz, quality, status, n_not_ok) -- every tie point intersected from its image rays at the
        device xhat, TIE order: xyz (n_tie, 3); quality (n_tie, 4): rays used, lambda_min / lambda_max of the
        intersection's normal matrix, RMS reprojection residual (px) of the linear and of the refined solution;
        status (n_tie) FBA_ISECT_* (capi.ISECT_STATUS); the number of points not OK.  write_xhat: the OK and REFINE
        points replace their entries of the device xhat.  Other ranks' tie points are 0."""
        nt = self.packed.n_tie
        op = IntersectOptions(**_given(refine_iters=refine_iters, write_xhat=write_xhat, min_ratio=min_ratio,
                                       refine_tol=refine_tol))
        xyz, q, st = np.zeros((max(nt, 1), 3)), np.zeros((max(nt, 1), 4)), np.zeros(max(nt, 1), dtype=np.int32)
        bad = C.c_int64()
        check(lib.fba_intersect(self.h, C.byref(op), ptr(xyz), ptr(q), ptr(st), C.byref(bad)))
        return xyz[:nt], q[:nt], st[:nt], bad.value

    def resect(self, use=None, refine_iters=None, write_xhat=None, min_ratio=None, refine_tol=None):
        """fba_resect: (eop, quality, status, n_not_ok) -- every image resected from object points and its measured
        image rays at the device xhat, EXT order: eop (n_img, 6) Xc Yc Zc omega phi kappa; quality (n_img, 5): points
        used, lambda_1 / lambda_11 of the linear solution's Gram matrix, RMS reprojection residual (px) of the linear
        and of the refined solution, the share of the used points in front (d . M (X - C) > 0); status (n_img)
        FBA_RESECT_* (capi.RESECT_STATUS); the number of images not OK.  use: "control" (control observations only)
        or "all" (also the tie observations at the device xhat's tie coordinates).  write_xhat: the OK and REFINE
        images replace their six entries of the device xhat.  One GPU only (world == 1)."""
        ni = self.packed.n_img
        op = ResectOptions(**_given(use=use, refine_iters=refine_iters, write_xhat=write_xhat, min_ratio=min_ratio,
                                    refine_tol=refine_tol))
        eop, q, st = np.zeros((max(ni, 1), 6)), np.zeros((max(ni, 1), 5)), np.zeros(max(ni, 1), dtype=np.int32)
        bad = C.c_int64()
        check(lib.fba_resect(self.h, C.byref(op), ptr(eop), ptr(q), ptr(st), C.byref(bad)))
        return eop[:ni], q[:ni], st[:ni], bad.value

    def vce(self, group, n_groups, max_rounds=None, tol=None, min_redundancy=None, clip=None):
        """fba_vce: variance components of groups of image measurements, estimated and applied on the device.
        group: (2 n_pts) ids in [0, n_groups) or -1 (no estimated group), PHO order, x y interleaved like v (or
        (n_pts, 2)).  Returns a dict: component (n_groups + 2) the cumulative variance factor of each group relative to
        its starting weights (the last two entries -- the rows with id -1, the priors -- are reported only and stay
        1); table (rounds, n_groups + 2, 4): R, T, n and sigma2 of every round; status (n_groups + 2) FBA_VCE_*
        (capi.VCE_STATUS) of the last round; rounds, iterations, converged.  Afterwards the context is as adjust()
        leaves one with these weights: residuals(), postfit() and get_weights() work unchanged.  One GPU, no robust
        loss, no damping."""
        g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        if g.size != 2 * self.packed.n_pts:
            raise ValueError("vce: group must have 2*n_pts entries")
        op = VceOptions(**_given(max_rounds=max_rounds, tol=tol, min_redundancy=min_redundancy, clip=clip))
        ng2 = max(int(n_groups), 0) + 2
        comp = np.zeros(ng2)
        table = np.zeros((max(op.max_rounds, 1), ng2, 4))
        st = np.zeros(ng2, dtype=np.int32)
        rounds, its, conv = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.fba_vce(self.h, int(n_groups), ptr(g), C.byref(op), ptr(comp), ptr(table), ptr(st), C.byref(rounds),
                          C.byref(its), C.byref(conv)))
        return {"component": comp, "table": table[: rounds.value].copy(), "status": st, "rounds": rounds.value,
                "iterations": its.value, "converged": bool(conv.value)}

    def snoop(self, excluded=None, max_rounds=None, min_rays=None, min_img_points=None, crit=None, max_share=None):
        """fba_snoop: Baarda data snooping over the image points on the device -- rounds of adjustment, w-test,
        elimination of the local maxima above crit (at most one per tie point and per image in a round) and, once a
        round eliminates nothing, re-admission of the excluded points whose predicted residual passes the test.
        excluded: (n_pts) nonzero = the point starts excluded (PHO order), or None.  Returns a dict: excluded (n_pts)
        uint8 0 active / 1 excluded / 2 re-admitted (capi.SNOOP_STATE); stat (n_pts) W or W~ of the last round; table
        (rounds, 4): picked, passed by the back-check, excluded after the round, largest active W; rounds, iterations,
        converged, status_bits (bit 1: the max_share stop).  Afterwards xhat, residuals() and get_weights() are those
        of adjust() with the final weights (1e-12 x the starting weight on the excluded points); the call consumed
        the last factor, so postfit() needs one step() first.  One GPU, no robust loss, no damping."""
        n = self.packed.n_pts
        ex = np.zeros(max(n, 1), dtype=np.uint8)
        if excluded is not None:
            e = np.asarray(excluded).reshape(-1)
            if e.size != n:
                raise ValueError("snoop: excluded must have n_pts entries")
            ex[:n] = e != 0
        op = SnoopOptions(**_given(max_rounds=max_rounds, min_rays=min_rays, min_img_points=min_img_points, crit=crit,
                                   max_share=max_share))
        stat = np.zeros(max(n, 1))
        table = np.zeros((max(op.max_rounds, 1), 4))
        rounds, its, conv, bits = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.fba_snoop(self.h, C.byref(op), ptr(ex), ptr(stat), ptr(table), C.byref(rounds), C.byref(its),
                            C.byref(conv), C.byref(bits)))
        return {"excluded": ex[:n], "stat": stat[:n], "table": table[: rounds.value].copy(), "rounds": rounds.value,
                "iterations": its.value, "converged": bool(conv.value), "status_bits": bits.value}

    def set_spin_bound(self, spins=0):
        """(tests) this context's hand-off poll bound in sleeps; 0 restores the default"""
        check(lib.fba_set_spin_bound(self.h, int(spins)))

    def set_timing(self, on=True):
        check(lib.fba_set_timing(self.h, int(on)))

    def set_probe(self, on=True):
        check(lib.fba_set_probe(self.h, int(on)))

    def probe_stats(self):
        out = np.zeros(4)
        check(lib.fba_probe_stats(self.h, ptr(out)))
        return {"launches": int(out[0]), "ms": float(out[1]), "flops": float(out[2])}

    def timings(self):
        ms = np.zeros(8)
        check(lib.fba_last_timings(self.h, ptr(ms)))
        return ms


def live_allocations() -> int:
    """(tests) fba_test_live_allocations: device and pinned allocations libfba holds in this process now"""
    n = C.c_int64()
    check(lib.fba_test_live_allocations(C.byref(n)))
    return n.value


def eig3_host(blocks):
    """fba_eig3_host: the device's symmetric 3 x 3 eigen routine (csrc/fba_eig3.h) run on the CPU, no GPU needed.
    blocks (n, 6): XX XY XZ YY YZ ZZ -> (n, 12): the semi-axes a >= b >= c = sqrt(max(lambda, 0)), then the three
    unit axis vectors as rows."""
    b = np.ascontiguousarray(blocks, dtype=np.float64).reshape(-1, 6)
    out = np.zeros((max(len(b), 1), 12))
    check(lib.fba_eig3_host(len(b), ptr(b) if len(b) else None, ptr(out)))
    return out[: len(b)]


def unproject_host(typ, xy, camtab):
    """fba_unproject_host: the device's inverse projection model (csrc/fba_ray.h) run on the CPU, no GPU needed.
    typ: a name of TYPES or the FBA_TYPE_* number; xy (n, 2) pixels; camtab: xp yp c ydir P1 P2 K1..Knk ->
    (out (n, 5): xu yu and the unit direction in the camera frame, status (n) FBA_RAY_*)."""
    t = TYPES.index(typ) if isinstance(typ, str) else int(typ)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    ct = np.ascontiguousarray(camtab, dtype=np.float64).reshape(-1)
    out, st = np.zeros((max(len(xy), 1), 5)), np.zeros(max(len(xy), 1), dtype=np.int32)
    check(lib.fba_unproject_host(t, ct.size - 6, len(xy), ptr(xy) if len(xy) else None, ptr(ct), ptr(out), ptr(st)))
    return out[: len(xy)], st[: len(xy)]


def resect_host(typ, xyz, ray, c, ydir, ray_status=None, std_x=0.3, std_y=0.3, refine_iters=None, min_ratio=None,
                refine_tol=None):
    """fba_resect_host: the device's per-image resection (csrc/fba_resect.h) run on the CPU for one image, no GPU
    needed.  typ: a name of TYPES or the FBA_TYPE_* number; xyz (n, 3) object points; ray (n, 5) unproject_host's
    rows of their measurements; ray_status (n) FBA_RAY_* or None; c, ydir of the camera -> (eop (6), quality (5),
    status): Context.resect's row of one image, eop zeros for FEW and WEAK."""
    t = TYPES.index(typ) if isinstance(typ, str) else int(typ)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    ray = np.ascontiguousarray(ray, dtype=np.float64).reshape(-1, 5)
    if len(xyz) != len(ray):
        raise ValueError("resect_host: one ray per object point expected")
    rs = None if ray_status is None else np.ascontiguousarray(ray_status, dtype=np.int32).reshape(-1)
    if rs is not None and len(rs) != len(xyz):
        raise ValueError("resect_host: one ray status per object point expected")
    op = ResectOptions(**_given(refine_iters=refine_iters, min_ratio=min_ratio, refine_tol=refine_tol))
    eop, q, st = np.zeros(6), np.zeros(5), C.c_int32()
    n = len(xyz)
    check(lib.fba_resect_host(t, n, ptr(xyz) if n else None, ptr(ray) if n else None, ptr(rs) if (rs is not None and n) else None,
                              float(c), float(ydir), float(std_x), float(std_y), C.byref(op), ptr(eop), ptr(q),
                              C.byref(st)))
    return eop, q, st.value


def vce_host(group, r, t, n_groups, max_rounds=None, tol=None, min_redundancy=None, clip=None):
    """fba_vce_host: the device's group arithmetic (csrc/fba_vce.h) run on the CPU, no GPU needed: the sums of r and t
    over the rows of each group in index order, then the estimate, the clamp, the factor and the status.  group (n)
    ids in [0, n_groups) or -1 -> (sums (n_groups + 1, 3): R T n, the last row the ids -1; sigma2, factor, status
    (n_groups))."""
    g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if not (g.size == r.size == t.size):
        raise ValueError("vce_host: group, r and t must have the same length")
    op = VceOptions(**_given(max_rounds=max_rounds, tol=tol, min_redundancy=min_redundancy, clip=clip))
    ng = max(int(n_groups), 0)
    sums, s2, f, st = np.zeros((ng + 1, 3)), np.zeros(max(ng, 1)), np.zeros(max(ng, 1)), np.zeros(max(ng, 1), dtype=np.int32)
    n = g.size
    check(lib.fba_vce_host(n, int(n_groups), ptr(g) if n else None, ptr(r) if n else None, ptr(t) if n else None,
                           C.byref(op), ptr(sums), ptr(s2), ptr(f), ptr(st)))
    return sums, s2[:ng], f[:ng], st[:ng]


def snoop_host(W, state, tie, img, n_tie=None, n_img=None, max_rounds=None, min_rays=None, min_img_points=None, crit=None,
               max_share=None):
    """fba_snoop_host: one round's selection of the data snooping (csrc/fba_snoop.h) run on the CPU in index order, no
    GPU needed.  W (n) the points' statistics, state (n) 0 active / 1 excluded / 2 re-admitted, tie (n) the tie point
    (< 0: a control observation), img (n) the image -> (pick, readmit (n) bool, status_bits)."""
    W = np.ascontiguousarray(W, dtype=np.float64).reshape(-1)
    state = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
    tie = np.ascontiguousarray(tie, dtype=np.int32).reshape(-1)
    img = np.ascontiguousarray(img, dtype=np.int32).reshape(-1)
    n = W.size
    if not (state.size == tie.size == img.size == n):
        raise ValueError("snoop_host: W, state, tie and img must have the same length")
    n_tie = int(tie.max(initial=-1)) + 1 if n_tie is None else int(n_tie)
    n_img = int(img.max(initial=-1)) + 1 if n_img is None else int(n_img)
    op = SnoopOptions(**_given(max_rounds=max_rounds, min_rays=min_rays, min_img_points=min_img_points, crit=crit,
                               max_share=max_share))
    pick, back = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    bits = C.c_int32()
    z = lambda a: ptr(a) if n else None
    check(lib.fba_snoop_host(n, z(W), z(state), z(tie), z(img), n_tie, n_img, C.byref(op), z(pick), z(back), C.byref(bits)))
    return pick[:n].astype(bool), back[:n].astype(bool), bits.value


def tie_blocks(cx_tie):
    """(n_tie, 6) XX XY XZ YY YZ ZZ -> (n_tie, 3, 3) full symmetric"""
    b = np.asarray(cx_tie, dtype=np.float64).reshape(-1, 6)
    return b[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def count_unknowns(packed: PackedProblem, settings: Settings) -> int:
    u = C.c_int64()
    check(lib.fba_count_unknowns(C.byref(packed.struct), C.byref(settings), C.byref(u)))
    return u.value


def partition(packed: PackedProblem, world: int):
    t = np.zeros(max(packed.n_tie, 1), dtype=np.int32)
    q = np.zeros(max(packed.n_pts, 1), dtype=np.int32)
    check(lib.fba_partition(C.byref(packed.struct), int(world), ptr(t), ptr(q)))
    return t[: packed.n_tie], q[: packed.n_pts]


def image_order(packed: PackedProblem):
    """fba_image_order: slot -> EXT row (-1: padding slot) of the reduced system's image part."""
    n = C.c_int32()
    check(lib.fba_image_order(C.byref(packed.struct), None, C.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=np.int32)
    check(lib.fba_image_order(C.byref(packed.struct), ptr(out), C.byref(n)))
    return out[: n.value]


def finish_stats(packed: PackedProblem, settings: Settings, sx2, sy2, vtpv):
    sums = np.array([sx2, sy2], dtype=np.float64)
    st = np.zeros(6)
    check(lib.fba_finish_stats(C.byref(packed.struct), C.byref(settings), ptr(sums), float(vtpv), ptr(st)))
    return st
