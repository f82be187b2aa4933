"""The zero-shot scene path without a GPU: tests/zero_shot_ref.py (the restatement the device kernels are held to) against the
reference notebook's own cells (tests/golden/zero_shot.npz, made by exec'ing cells 9 and 11) and scipy, and the host-side
parameter handling of cppf_amd.zero_shot."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limits_cases as LC  # noqa: E402
import zero_shot_ref as Z  # noqa: E402

from cppf_amd import zero_shot  # noqa: E402


def _dedupe(loc, diff):
    """rows of the notebook's proposals with consecutive repeats removed (include/cppf.h: cppf_scene_proposals)"""
    return [k for k in range(len(diff)) if k == 0 or not (np.array_equal(loc[k], loc[k - 1]) and diff[k] == diff[k - 1])]


def test_restatement_equals_notebook_cell9(golden):
    g = golden("zero_shot.npz")
    for name in g["cases"]:
        grid = g[f"{name}.grid"]
        sm = Z.smooth(grid)
        assert hashlib.sha256(sm.tobytes()).digest() == g[f"{name}.smoothed_sha256"].tobytes(), name
        loc, val, diff, _ = Z.proposals(sm)
        if int(g[f"{name}.raises"]):                     # a size-1 axis: the notebook raises, the defined result is empty
            assert min(grid.shape) < 2 and loc.shape[0] == 0
            continue
        k = _dedupe(g[f"{name}.loc"], g[f"{name}.diff"])
        assert np.array_equal(loc, g[f"{name}.loc"][k]), name
        assert val.tobytes() == g[f"{name}.value"][k].tobytes() and diff.tobytes() == g[f"{name}.diff"][k].tobytes(), name
        assert np.array_equal(Z.world(loc, g["corner"], float(g["res"])), g[f"{name}.world"][k]), name


def test_last_plane_case_repeats_in_notebook(golden):
    g = golden("zero_shot.npz")
    assert len(g["last_plane.diff"]) == 64 and len(_dedupe(g["last_plane.loc"], g["last_plane.diff"])) < 64


def test_restatement_equals_notebook_segmentation(golden):
    g = golden("zero_shot.npz")
    for s in range(4):
        idx, surv = g[f"seg{s}.idx"], g[f"seg{s}.surv"]
        pm, pos = Z.segment(idx, surv, 200)
        assert np.array_equal(pm, g[f"seg{s}.point_mask"])
        assert np.array_equal(idx[pos], g[f"seg{s}.pairs"])


@pytest.mark.parametrize("sigma", [1.0, 2.0])
def test_smooth_equals_scipy(sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for shape in [(1, 1, 1), (1, 2, 3), (2, 9, 1), (3, 5, 9), (9, 9, 9), (17, 4, 6)]:
        g = (rng.random(shape) * 300).astype(np.float32)
        assert Z.smooth(g, sigma).tobytes() == ndi.gaussian_filter(g, sigma=sigma).tobytes(), shape


@pytest.mark.parametrize("sigma,truncate,radius", LC.SMOOTH_PARAMS)
def test_smooth_equals_scipy_at_the_radius_limits(sigma, truncate, radius):
    """radius 0, 31 and 32 (csrc/scene.hip SCN_MAX_RADIUS) on the grids of tests/test_gpu_limits.py: lines shorter than the radius
    included, where scipy's reflection repeats"""
    ndi = pytest.importorskip("scipy.ndimage")
    assert (Z.gaussian_weights(sigma, truncate).shape[0] - 1) // 2 == radius
    for shape in LC.SMOOTH_GRIDS:
        g = LC.smooth_grid_case(shape)
        assert Z.smooth(g, sigma, truncate).tobytes() == ndi.gaussian_filter(g, sigma=sigma, truncate=truncate).tobytes(), shape


def test_restatement_equals_notebook_cell9_at_margin_64_and_1(golden):
    """tests/golden/zero_shot_margins.npz: the notebook's cell 9 with its margin set to the documented limits, on the grids of
    tests/limits_cases.py (edge slices of 128 cells -- the whole of np.mean's base case -- and boxes clipped at both ends)"""
    g = golden("zero_shot_margins.npz")
    for name, sm in (("peaks", LC.margin_grid_smoothed()), ("thin", Z.smooth(LC.smooth_grid_case((33, 7, 70))))):
        for margin in (64, 1):
            key = f"{name}.m{margin}"
            loc, val, diff, _ = Z.proposals(sm, float(g[f"{key}.thresh"]), margin, max_proposals=64, max_iters=64)
            k = _dedupe(g[f"{key}.loc"], g[f"{key}.diff"])
            assert len(k) >= 2 and np.array_equal(loc, g[f"{key}.loc"][k]), key
            assert val.tobytes() == g[f"{key}.value"][k].tobytes() and diff.tobytes() == g[f"{key}.diff"][k].tobytes(), key


def test_np_mean_order():
    rng = np.random.default_rng(4)
    for _ in range(3000):
        n, st = int(rng.integers(1, 129)), int(rng.integers(1, 4))
        v = (rng.standard_normal(n * st) * 10.0 ** rng.uniform(-3, 4)).astype(np.float32)[::st]
        assert Z.np_mean_f32(v).tobytes() == np.mean(v).tobytes()


def test_distinct_mask_matches_cell6_formula():
    rng = np.random.default_rng(5)
    pc = rng.standard_normal((50, 3)).astype(np.float32)
    nrm = rng.standard_normal((50, 3)).astype(np.float32)
    nrm[:25] = [0, 0, 1]                                          # parallel normals, pairs in the plane: filtered
    pc[:25, 2] = 0
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    idx = rng.integers(0, 50, (4000, 2))
    keep = Z.distinct_mask(pc, nrm, idx)
    both_flat = (idx < 25).all(1) & (idx[:, 0] != idx[:, 1])
    assert not keep[both_flat].any() and keep[~(idx < 25).any(1)].mean() > 0.9


@pytest.mark.parametrize("sigma,truncate", [(1.0, 4.0), (2.0, 4.0), (0.5, 3.0), (1.3, 2.5)])
def test_weights_equal_scipy(sigma, truncate):
    filt = pytest.importorskip("scipy.ndimage._filters")
    r = int(truncate * sigma + 0.5)
    assert np.array_equal(zero_shot.gaussian_weights(sigma, truncate), filt._gaussian_kernel1d(sigma, 0, r)[::-1])
    assert np.array_equal(zero_shot.gaussian_weights(sigma, truncate), Z.gaussian_weights(sigma, truncate))


def test_parameter_validation():
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            zero_shot.gaussian_weights(bad)
    with pytest.raises(ValueError):
        zero_shot.gaussian_weights(10.0)                          # radius 40 > 32
    assert zero_shot._check_loop_args(50, 10, 32, None) == 128
    assert zero_shot._check_loop_args(50, 10, 5, 7) == 7
    for args in [(50, 0, 32, None), (50, 65, 32, None), (50, 10, -1, None), (50, 10, 4, -1), (float("nan"), 10, 4, None)]:
        with pytest.raises(ValueError):
            zero_shot._check_loop_args(*args)


def test_defined_behaviour_of_the_restatement():
    g = np.zeros((6, 1, 6), np.float32)
    assert Z.proposals(g)[0].shape == (0, 3)                      # an axis < 2
    g = np.zeros((12, 12, 12), np.float32)
    g[11, 5, 5] = 5000                                            # a peak on the last plane: repeats are emitted once
    loc, _, diff, it = Z.proposals(Z.smooth(g))
    assert loc.shape[0] >= 1 and np.array_equal(loc[0], [11, 5, 5]) and it < 128
    assert Z.proposals(Z.smooth(g), max_proposals=1)[0].shape[0] == 1
