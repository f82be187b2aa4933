"""The host's statements of the vote grid's dims and corners against the float64 reference of tests/grid_dims_cases.py, on every
case there (extents k * res +-3 ulp for every resolution in use, built to differ under a reciprocal-multiply or an unrounded double
quotient; three edges in one cloud; single point; all points equal; a denormal extent; both zeros as the minimum):
  inference.grid_shape through cppf_host_grid_shape (C-contiguous float32 clouds),
  inference.grid_shape through its numpy form (float64 and non-contiguous clouds),
  oracle.grid_setup (what the device kernels are held to elsewhere).
The host's dims choose the pipeline an object runs on and the device computes its own: all of them must give the reference's."""
import numpy as np
import pytest

import grid_dims_cases as G
from cppf_amd import _lib
from cppf_amd.inference import grid_shape


def test_the_case_set_bites_on_both_mistakes():
    """the generator's own assertions, restated on what it returned: exact extents, >= 20 cases per resolution that differ from the
    reference under each mistake, and the issue's two worked examples"""
    assert set(G.BITING) == {float(np.float32(r)) for r in (0.004, 0.01, 0.03, 0.002, 0.0016)}
    for r, b in G.BITING.items():
        assert b["recip"] >= G.MIN_BITING and b["double"] >= G.MIN_BITING, (r, b["recip"], b["double"])
    f32 = np.float32
    assert G.recip_dims_axis(f32(0.012000000104308128), f32(0.004)) != G.ref_dims_axis(f32(0.012000000104308128), f32(0.004))
    assert G.recip_dims_axis(f32(0.04999999701976776), f32(0.01)) != G.ref_dims_axis(f32(0.04999999701976776), f32(0.01))
    for c in G.CASES:
        lo, hi = c["pc"].min(0), c["pc"].max(0)
        assert tuple(int(f32(f32(hi[j] - lo[j]) / f32(c["res"]))) + 1 for j in range(3)) == c["dims"], c["name"]    # numpy's own f32 division
    assert all(c in G.DEVICE_CASES for c in G.CASES if c["biting"])


def _check(got, c, path):
    corners, dims = got
    assert tuple(int(v) for v in dims) == c["dims"], (path, c["name"], tuple(dims), c["dims"])
    assert G.corners_equal(corners, c["corners"], c["by_value"]), (path, c["name"], corners, c["corners"])


def test_grid_shape_c_form_equals_the_reference():
    L = _lib.lib()
    assert hasattr(L, "cppf_host_grid_shape")
    for c in G.CASES:
        pc = np.ascontiguousarray(c["pc"], np.float32)
        _check(grid_shape(pc, c["res"]), c, "C")


def test_grid_shape_numpy_form_equals_the_reference():
    for j, c in enumerate(G.CASES):
        if j % 2 or c["pc"].shape[0] == 1:                                     # (a one-row slice counts as contiguous)
            pc = c["pc"].astype(np.float64)                                    # not float32: the numpy form
        else:
            wide = np.zeros((c["pc"].shape[0], 5), np.float32)
            wide[:, 1:4] = c["pc"]
            pc = wide[:, 1:4]                                                  # float32 but not contiguous: the numpy form
            assert not pc.flags.c_contiguous
        _check(grid_shape(pc, c["res"]), c, "numpy")


def test_oracle_grid_setup_equals_the_reference(oracle):
    for c in G.CASES:
        corner, dims = oracle.grid_setup(c["pc"], c["res"])
        assert tuple(int(v) for v in dims) == c["dims"], (c["name"], tuple(dims), c["dims"])
        assert G.corners_equal(corner, c["corners"][0], c["by_value"]), (c["name"], corner, c["corners"][0])


@pytest.mark.parametrize("block", [256, 1024])
def test_placement_cases_hold_their_own_reference(block):
    """the device test's placement clouds, on the host forms: minimum and maximum wherever they sit"""
    for c in G.placement_cases(block):
        _check(grid_shape(c["pc"], c["res"]), c, "C")
