"""Every device and pinned allocation of a context has one owner: after fba_destroy, and after an fba_create
that fails half way, the library holds as many allocations as before (fba_test_live_allocations).

The count is exact, so there is no tolerance: a buffer added to the context and not to its owner, a call-lifetime
buffer left behind by an early return, or a workspace slot that is not freed shows as a difference of one.
"""
import numpy as np
import pytest

from test_gpu_general import SCENES, _folder

pytestmark = pytest.mark.gpu


def _exercise(fba, folder):
    """every entry point that allocates: the context's buffers, the weights' on first use, every workspace slot
    (post-fit outputs with all six requested, weights staging, cost, rays, intersection) and the call-lifetime
    buffers of build_awg / build_rsd"""
    ds = fba.load_folder(folder)
    ctx = fba.capi.Context(ds.pack(), fba.capi.make_settings(ds.settings))
    try:
        assert fba.capi.live_allocations() > 0
        ctx.adjust()
        v, _, st = ctx.residuals()
        x = ctx.get_xhat()
        ctx.build_awg(x)
        ctx.build_rsd(v, x)
        ctx.set_weights(np.full(2 * ds.pack().n_pts, 0.5))
        ctx.set_loss("huber")
        ctx.step()  # the weighted, robust linearisation that get_weights and the post-fit outputs read
        ctx.get_weights()
        ctx.cost()
        out = ctx.postfit(st[3], reliability=True, tie_cov=True, ellipsoids=True, corr=True)
        assert all(o is not None for o in out)
        ctx.image_rays()
        ctx.intersect()
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", ["stage3_pinhole", "stage3_noic_pinhole"])
def test_cam0_context_frees_everything(fba, cam0_folders, variant):
    """cam0 (1029 observations) with the inner constraints' border and without"""
    n0 = fba.capi.live_allocations()
    _exercise(fba, cam0_folders[variant])
    assert fba.capi.live_allocations() == n0


def test_general_point_context_frees_everything(fba, tmp_path):
    """the smallest general-point scene of tests/test_gpu_general.py (the d_g* tables, k_rel_gen's workspace)"""
    folder = _folder(tmp_path, "dup", **SCENES["dup"])
    n0 = fba.capi.live_allocations()
    _exercise(fba, folder)
    assert fba.capi.live_allocations() == n0


def test_refused_create_frees_everything(fba, tmp_path, monkeypatch):
    """chol_setup refuses the subtree split on the per-level factorisation (FBA_ERR_UNSUPPORTED) after the plan is
    uploaded and most work buffers are allocated: nothing of the half-built context stays behind"""
    from fba_amd import synth
    folder = str(tmp_path / "c3")
    synth.make_config(3, folder)
    ds = fba.load_folder(folder)
    packed, settings = ds.pack(), fba.capi.make_settings(ds.settings)
    n0 = fba.capi.live_allocations()
    monkeypatch.setenv("FBA_CHOL_FLOW", "0")
    with pytest.raises(fba.capi.FBAError) as ei:
        fba.capi.Context(packed, settings, rank=0, world=2, split=True)
    assert ei.value.code == 5, ei.value
    assert fba.capi.live_allocations() == n0
