"""The C boundary's refusal of a NULL context, entry point by entry point (no GPU): the return code and the exact
fba_last_error() text of every exported function that takes a context, and the export list itself.

The expected texts are literals, recorded from the library as it was built before the C API file was split by
subsystem: they pin that the split and its shared entry check changed no message.
"""
import ctypes as C
import subprocess

import pytest

# entry point -> (return code, fba_last_error()) for a NULL context and otherwise valid arguments
NULL_CONTEXT = {
    "fba_get_priors": (1, "fba_get_priors: NULL context"),
    "fba_solve_mode": (1, "fba_solve_mode: null argument"),
    "fba_buildxhat": (1, "NULL context"),
    "fba_set_xhat": (1, "NULL argument"),
    "fba_get_xhat": (1, "NULL argument"),
    "fba_build_awg": (1, "NULL context"),
    "fba_accumulate": (1, "NULL context"),
    "fba_reduce_buffer": (1, "NULL argument"),
    "fba_synchronize": (1, "NULL context"),
    "fba_solve_update": (1, "NULL context"),
    "fba_solve_update_async": (1, "NULL context"),
    "fba_deltasum_device": (1, "NULL argument"),
    "fba_solve_finish": (1, "NULL context"),
    "fba_step": (1, "NULL context"),
    "fba_adjust": (1, "NULL context"),
    "fba_residuals": (1, "NULL context"),
    "fba_build_rsd": (1, "NULL argument"),
    "fba_covariance": (1, "NULL context"),
    "fba_reliability": (1, "NULL context"),
    "fba_set_weights": (1, "fba_set_weights: NULL context"),
    "fba_set_loss": (1, "fba_set_loss: NULL context"),
    "fba_get_weights": (1, "fba_get_weights: NULL argument"),
    "fba_last_timings": (1, "NULL argument"),
    "fba_set_timing": (1, "NULL context"),
    "fba_set_probe": (1, "NULL context"),
    "fba_probe_stats": (1, "NULL argument"),
    "fba_set_spin_bound": (1, "fba_set_spin_bound: bad argument"),
    "fba_set_damping": (1, "fba_set_damping: NULL context"),
    "fba_cost": (1, "fba_cost: NULL argument"),
    "fba_adjust_lm": (1, "fba_adjust_lm: NULL context"),
    "fba_postfit_outputs": (1, "NULL context"),
    "fba_image_rays": (1, "fba_image_rays: NULL context"),
    "fba_intersect": (1, "fba_intersect: NULL context"),
    "fba_resect": (1, "fba_resect: NULL context"),
    "fba_vce": (1, "fba_vce: NULL context"),
    "fba_snoop": (1, "fba_snoop: NULL context"),
}
# the exports that take no context (fba_destroy(NULL) is a no-op and returns nothing)
NO_CONTEXT = {"fba_last_error", "fba_abi_version", "fba_count_unknowns", "fba_partition", "fba_image_order", "fba_create",
              "fba_create_priors", "fba_destroy", "fba_finish_stats", "fba_test_border_solve", "fba_test_live_allocations",
              "fba_unproject_host", "fba_resect_host", "fba_vce_host", "fba_snoop_host", "fba_eig3_host"}


def null_context_call(lib, name):
    """name(NULL, ...): every other pointer a zeroed buffer of 64 doubles, every double 1, every integer 0"""
    f = getattr(lib, name)
    args, keep = [None], []
    for t in f.argtypes[1:]:
        if t is C.c_void_p:
            keep.append((C.c_double * 64)())
            args.append(C.cast(keep[-1], C.c_void_p))
        else:
            args.append(1.0 if t is C.c_double else 0)
    return f(*args)


@pytest.mark.parametrize("name", sorted(NULL_CONTEXT))
def test_null_context_is_refused(fba, name):
    rc, text = NULL_CONTEXT[name]
    assert null_context_call(fba.capi.lib, name) == rc
    assert fba.capi.last_error() == text


def test_every_context_entry_point_is_listed(fba):
    every = set(fba.capi.EXPORTS) | set(fba.capi.HOST_EXPORTS)
    assert set(NULL_CONTEXT) | NO_CONTEXT == every and not set(NULL_CONTEXT) & NO_CONTEXT
    fba.capi.lib.fba_destroy(None)


def test_exports_are_the_library_s_symbols(fba):
    out = subprocess.run(["nm", "-D", "--defined-only", fba.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("fba_")}
    assert defined == set(fba.capi.EXPORTS) | set(fba.capi.HOST_EXPORTS)
    assert fba.capi.lib.fba_abi_version() == 2
