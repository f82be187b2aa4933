"""The host side of the mask-free scene path, no device: tests/scene_poses_ref.py on hand-made cases, the proposal cap of the
perfect-head scenes of tests/test_gpu_scene_poses.py on the oracle's own vote, and the refusals of cppf_amd.scene_poses that are decided
before anything touches a device."""
import os
import sys

import numpy as np
import pytest

import cppf_amd.synthetic as syn
from cppf_amd import scene_poses
from cppf_amd.config import CATEGORIES
from cppf_amd.inference import _assemble, grid_shape
from cppf_amd.utils.util import fibonacci_sphere, num_sphere_bins

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_poses_ref as S  # noqa: E402
import zero_shot_ref as Z  # noqa: E402


def _is_rotation(R):
    """orthonormal and right-handed, up to the 1e-9 regulariser of the right axis' normalisation (nocs/inference.py:307: its length
    is 1 / (1 + 1e-9), so R^T R is off by 2e-9 in one entry and the determinant by 1e-9)"""
    return np.allclose(R.T @ R, np.eye(3), atol=1e-8) and abs(np.linalg.det(R) - 1) < 1e-8


def test_assemble_hand_made_cases():
    mug, bowl = CATEGORIES["mug"], CATEGORIES["bowl"]
    # a right axis that leans into up is orthogonalised against it; x = right, y = up, z = right x up
    p = S.assemble([0, 1, 0], [1, 0.2, 0], [0.1, 0.2, 0.2], mug)
    assert np.allclose(p["R"], np.eye(3), atol=1e-8) and _is_rotation(p["R"]) and abs(p["scale_norm"] - 0.3) < 1e-12
    # no right axis: the fixed vector (0, -up_z, up_y)
    up = np.array([0.0, 0.6, 0.8])
    p = S.assemble(up, None, [1, 1, 1], bowl)
    assert np.allclose(p["right"], [0, -0.8, 0.6], atol=1e-8) and _is_rotation(p["R"]) and np.allclose(p["R"][:, 1], up)
    # ... which vanishes for up = +-x: a random tangent, still a rotation
    p = S.assemble([1, 0, 0], None, [1, 1, 1], bowl)
    assert abs(np.linalg.norm(p["right"]) - 1) < 1e-12 and abs(p["right"] @ p["up"]) < 1e-12 and _is_rotation(p["R"])
    # the z_right frame: x = up x right, y = up, z = right
    class ZRight:
        regress_right, z_right = True, True
    p = S.assemble([0, 1, 0], [0, 0, 1], [1, 1, 1], ZRight)
    assert np.allclose(p["R"], np.eye(3), atol=1e-8)


@pytest.mark.parametrize("cat", ["mug", "bowl"])
def test_assemble_agrees_with_the_instance_paths_record_assembly(cat):
    """the same numbers through inference._assemble's 21-double record (T, best directions, sign sums, scale sums)"""
    cfg = CATEGORIES[cat]
    rng = np.random.default_rng(4)
    for _ in range(20):
        best = rng.standard_normal((2, 3))
        best /= np.linalg.norm(best, axis=-1, keepdims=True)
        sign = np.stack([rng.random(2) * 50, rng.random(2) * 50, [40.0, 40.0]], -1)        # {up loss sum, down loss sum, n} per axis
        logit_sums, n = rng.standard_normal(3) * 4, 40
        rec = np.concatenate([[0.1, 0.2, 0.9], best.reshape(-1), sign.reshape(-1), logit_sums, [n], [0, 0]])
        got = _assemble(rec, cfg)
        dirs = [-best[j] if sign[j, 1] < sign[j, 0] else best[j] for j in range(2)]
        scale = np.exp((logit_sums / n).astype(np.float32)).astype(np.float64) * np.asarray(cfg.scale_mean) * 2
        want = S.assemble(dirs[0], dirs[1], scale, cfg)
        for k in ("up", "right", "R", "scale"):
            assert np.allclose(got[k], want[k], atol=1e-12), k


def test_pose_ref_recovers_a_known_object(oracle):
    """one mug with the world's axes and perfect heads, every pair kept: the oracle composition finds its axes and its size"""
    cfg = CATEGORIES["mug"]
    ob = syn.make_posed_object("mug", 1024, 5, rotate=False)
    idx = np.random.default_rng(0).integers(0, 1024, (20000, 2))
    heads = syn.closed_form_heads(ob["pc"], ob["normals"], idx, cfg, quantise=False)
    sph = np.array(fibonacci_sphere(num_sphere_bins(1.5)))
    p = S.pose_ref(oracle, ob["pc"], ob["normals"], idx, heads, np.arange(20000), ob["center"], sph, cfg)
    ang = lambda a, b: np.degrees(np.arccos(np.clip(abs(a @ b), -1, 1)))
    assert ang(p["up"], np.array([0, 1.0, 0])) < 2.0 and ang(p["right"], np.array([1.0, 0, 0])) < 2.0 and _is_rotation(p["R"])
    assert np.abs(p["scale"] / (2 * np.asarray(cfg.scale_mean)) - 1).max() < 0.01                  # exp(mean of N(0, 0.05)) ~ 1
    assert np.allclose(p["RT"][:3, :3], p["R"] * p["scale_norm"]) and np.array_equal(p["RT"][:3, 3], ob["center"])
    # an empty list is defined: the first bin, no flip, the mean scale
    e = S.pose_ref(oracle, ob["pc"], ob["normals"], idx, heads, np.zeros(0, np.int64), ob["center"], sph, cfg)
    assert np.allclose(e["scale"], 2 * np.asarray(cfg.scale_mean)) and _is_rotation(e["R"])


@pytest.mark.parametrize("cat,n_obj,seed", S.PERFECT_SCENES)
def test_proposal_cap_holds_on_the_oracles_vote(oracle, cat, n_obj, seed):
    """the condition the GPU test puts on its scenes, checked without the code under test: on the oracle's vote grid, smoothed and
    searched by the numpy restatement, 2 n_obj proposals hold every object's centre within one cell, each by its own proposal"""
    sc = S.perfect_scene(cat, n_obj, seed)
    cfg = sc["cfg"]
    corners, dims = grid_shape(sc["pc"], cfg.res)
    grid = np.zeros(dims, np.float32)
    oracle.ppf_voting(sc["pc"], sc["outputs"], np.ones(sc["pc"].shape[0], np.float32), sc["idx"].astype(np.int32), grid, corners[0],
                      cfg.res, 72, True, threads=min(8, oracle.num_threads()))
    loc, val, diff, _ = Z.proposals(Z.smooth(grid), max_proposals=2 * n_obj)
    m = S.match_objects(loc, corners[0], cfg.res, [o["center"] for o in sc["obs"]])
    assert None not in m and len(set(m)) == n_obj, (m, loc, val)
    assert S.match_objects(loc[:1], corners[0], cfg.res, [o["center"] for o in sc["obs"]]).count(None) == n_obj - 1   # distinct means distinct


def test_refusals_before_any_device_work():
    from cppf_amd.models.model import PPFEncoder
    cfg = CATEGORIES["bowl"]
    enc9, enc141, wide = PPFEncoder([84, 32, 32, 16], 9), PPFEncoder([84, 32, 32, 16], 141), PPFEncoder([84, 64, 16], 141)
    x = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="out_dim"):
        scene_poses.scene_poses(enc9, x, x, x, np.zeros((2, 2), np.int64), None, None, cfg)
    with pytest.raises(ValueError, match="standard pair encoder"):
        scene_poses.scene_poses(wide, x, x, x, np.zeros((2, 2), np.int64), None, None, cfg)
    with pytest.raises(ValueError, match="max_proposals"):
        scene_poses.scene_poses(enc141, x, x, x, np.zeros((2, 2), np.int64), None, None, cfg, max_proposals=33)
    with pytest.raises(ValueError, match="both or neither"):
        scene_poses.scene_poses(None, x, x, None, np.zeros((2, 2), np.int64), None, None, cfg, outputs=np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="margin"):
        scene_poses.scene_poses(enc141, x, x, x, np.zeros((2, 2), np.int64), None, None, cfg, margin=0)
    with pytest.raises(ValueError, match="out_dim"):
        scene_poses.scene_frame(np.zeros((4, 4), np.uint16), np.eye(3), enc9, None, cfg)
    with pytest.raises(ValueError, match="max_proposals"):
        scene_poses.scene_frame(np.zeros((4, 4), np.uint16), np.eye(3), enc141, None, cfg, max_proposals=40)
    scene_poses.check_encoder(enc141, cfg)
    assert scene_poses.check_args(32) == 128 and scene_poses.check_args(3, max_iters=5) == 5
