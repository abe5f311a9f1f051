"""CPU: the host planning of fba_create (fba_plan.cpp).

tests/plan_check.cpp builds small scenes, runs build_plan() for every rank and verifies what the kernels
later take on trust -- observation order, chunk cuts, pair keys / U-row terms / image keys per chunk, the
partial slot lists and their fixed (ascending) summation order, the general points' plan, the masks and
the multi-rank reduce-buffer layout -- against brute force from the problem arrays alone.  No GPU
involved; the kernels that run the plan are covered by tests/test_gpu_*.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fish-eye_bundle_adjustment_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "plan_check.cpp"),
                    os.path.join(CSRC, "fba_api_host.cpp"), os.path.join(CSRC, "fba_plan.cpp"), os.path.join(CSRC, "fba_order.cpp"),
                    "-o", exe], check=True)
    return exe


def run_scene(checker, scene):
    """The scene's "ok" lines as one dict of fields per checked plan (scene run, rank)."""
    env = dict(os.environ)
    for k in ("FBA_ND_LEAF", "FBA_FLOW_MERGE", "FBA_FLOW_BLOCK", "FBA_FLOW_SPLIT", "FBA_FLOW_MSPLIT"):
        env.pop(k, None)
    r = subprocess.run([checker, scene], capture_output=True, text=True, env=env, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and all(ln.startswith("ok ") for ln in lines), r.stdout + r.stderr
    plans = []
    for ln in lines:
        for rank in ln.split()[2:]:
            plans.append({k: int(v) for k, v in (f.split("=") for f in rank.split(":", 1)[1].split(","))})
    return plans


# what each scene is there for, pinned so that a scene cannot quietly stop exercising it
@pytest.mark.parametrize("scene,chunks", [
    ("points", 3),       # 150 points of one camera: cut by the point count, 64 + 64 + 22
    ("points_nk6", 5),   # nK = 6: 32-point chunks
    ("two_cameras", 4),  # 75 points per camera: 64 + 11, cut at the camera change, 64 + 11
    ("cut_obs", 2),      # 40 points of 12 images: 21 points fill the 256 observations of a chunk
    ("cut_terms", 3),    # 30 points of 20 images (190 terms each): 10 points fill the 2048 terms of a chunk
    ("control", 5)])     # 2 tie chunks, then control observations: 305 of camera 0 (256 + 49), 10 of camera 1
def test_chunk_cuts(checker, scene, chunks):
    (plan,) = run_scene(checker, scene)
    assert plan["chunks"] == chunks and plan["general"] == 0


def test_pair_terms_by_keys_or_u_rows(checker):
    """Every point seen by an image pair of its own: one term per key, so every chunk takes the U-row
    path at the default ratio 2 and none at ratio 0."""
    (urow,) = run_scene(checker, "own_pairs")
    assert urow["urow_chunks"] == urow["chunks"] == 5 and urow["urow_terms"] == 300 and urow["pair_keys"] == 0
    (keys,) = run_scene(checker, "own_pairs_ratio0")
    assert keys["urow_chunks"] == 0 and keys["urow_terms"] == 0 and keys["pair_keys"] == 300


def test_general_points(checker):
    """One scene with each kind: seen through two cameras, measured twice in one image, seen by 257 images
    of one camera, carrying a prior, and both twice in an image and through two cameras."""
    (plan,) = run_scene(checker, "general")
    assert plan["general"] == 5 and plan["points"] == 40
    ranks = run_scene(checker, "general_world2")  # the same on two ranks (priors: camera-side on rank 0, a point's on its owner)
    assert sum(p["general"] for p in ranks) == 5 and sum(p["obs"] for p in ranks) == plan["obs"]


def test_replicated_ranks(checker):
    plans = run_scene(checker, "replicated")  # world 2, then world 3: every rank
    assert len(plans) == 5
    assert sum(p["obs"] for p in plans[:2]) == sum(p["obs"] for p in plans[2:]) == 150 * 3 + 75 + 40


def test_subtree_split(checker):
    """World 2 with the subtree split on the 420-image scene of sched_check (leaves of 60)."""
    plans = run_scene(checker, "split")
    assert len(plans) == 2 and all(p["top"] > 0 for p in plans)
