"""Training views on the host: the OBJ reader, the numpy restatement of the rasteriser (tests/mesh_ref.py) against an independent
fp64 ray caster and a closed form, and the pose draws of utils/dataset.py:143-159.  No GPU."""
import numpy as np
import pytest

import mesh_ref as R
from cppf_amd import meshes as M
from cppf_amd.config import CATEGORIES

W, H = 160, 120
FX, FY = M.FX / 4, M.FY / 4


def _model(t, R3=np.eye(3)):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R3, t
    return m


def test_parse_obj_every_record_form():
    text = """# a comment
mtllib model.mtl
o thing
g group1
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 5 5 5
vt 0 0
vt 1 0
vn 0 0 1
usemtl red
s off
f 1 2 3
f 1/1 3/2 4/1
f 1//1 2//1 3//1
f 1/1/1 3/2/1 4/1/1   # trailing comment
f -5 -4 -3 -2
v 0 0 2
f 1 2 3 4 -1
"""
    v, f, bmin, bmax = M.parse_obj(text)
    assert v.shape == (6, 3) and v.dtype == np.float64 and f.dtype == np.int32
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3],
                          [0, 1, 2], [0, 2, 3], [0, 3, 5]]
    # vertex 4 (5, 5, 5) is referenced by no face: the bounds leave it out
    assert bmin.tolist() == [0, 0, 0] and bmax.tolist() == [1, 1, 2]
    with pytest.raises(ValueError):
        M.parse_obj("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        M.parse_obj("v 0 0 0\n")


def test_load_obj_file_round_trip(tmp_path):
    v, f, quads = R.box(0.3, 0.2, 0.1)
    p = tmp_path / "box.obj"
    p.write_text(R.to_obj(v, f, quads))
    v2, f2 = M.load_obj(str(p))
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    bmin, bmax = M.mesh_bounds(v2, f2)
    assert np.allclose(bmax - bmin, [0.6, 0.4, 0.2])


@pytest.mark.parametrize("name", ["sphere", "bottle", "box"])
def test_restatement_matches_the_ray_caster(name):
    mesh = {"sphere": lambda: R.uv_sphere(0.3, 12, 24), "bottle": lambda: R.necked_cylinder(0.12, 0.36, n_lon=24),
            "box": lambda: R.box(0.3, 0.2, 0.15)[:2]}[name]()
    v, f = mesh
    rot = M.roty(0.7)[:3, :3] @ M.rotx(0.5)[:3, :3]
    model = _model([0.05, -0.03, -1.4], rot)
    d = R.raster_ref(v, f, model, FX, FY, W, H)
    rc = R.ray_cast(v, f, model, FX, FY, W, H)
    both = (d > 0) & (rc > 0)
    assert both.sum() > 500
    assert np.max(np.abs(d[both] - rc[both]) / rc[both]) < 1e-5
    mis = (d > 0) != (rc > 0)
    if mis.any():
        assert R.edge_distance(v, f, model, FX, FY, W, H)[mis].max() < 1e-3


def test_axis_aligned_quad_at_known_depth():
    # the quad x in [-0.2, 0.3], y in [-0.1, 0.15] at z = -2: the pixels whose centres project inside, at depth 2
    v = np.array([[-0.2, -0.1, -2.0], [0.3, -0.1, -2.0], [0.3, 0.15, -2.0], [-0.2, 0.15, -2.0]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    d = R.raster_ref(v, f, np.eye(4), FX, FY, W, H)
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    x = (cc / (W / 2) - 1) / (2 * FX / W) * 2.0
    y = ((H - rr) / (H / 2) - 1) / (2 * FY / H) * 2.0
    inside = (x > -0.2) & (x < 0.3) & (y > -0.1) & (y < 0.15)
    assert np.array_equal(d > 0, inside)
    assert np.all(np.abs(d[inside] - 2.0) <= 2.0 * 4e-7)
    # seen from behind it is culled, and drawn with culling off
    assert not (R.raster_ref(v, R.flipped(f), np.eye(4), FX, FY, W, H) > 0).any()
    assert np.array_equal(R.raster_ref(v, R.flipped(f), np.eye(4), FX, FY, W, H, cull=False), d)


def test_near_plane_is_clipped_not_dropped():
    # a floor strip from in front of the near plane to far away: the visible part renders, nothing beyond depth 0.05 .. 5
    v = np.array([[-1.0, -0.3, 1.0], [1.0, -0.3, 1.0], [1.0, -0.3, -5.0], [-1.0, -0.3, -5.0]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    d = R.raster_ref(v, f, np.eye(4), FX, FY, W, H)
    assert (d > 0).sum() > 1000
    assert d[d > 0].min() >= np.float32(0.05) * (1 - 1e-6) and d.max() <= 5.0 * (1 + 1e-6)
    rc = R.ray_cast(v, f, np.eye(4), FX, FY, W, H)
    both = (d > 0) & (rc > 0)
    # (a grazing plane whose clipped vertices project ~1e4 px off screen: fp32 window coordinates cost a decade here)
    assert np.max(np.abs(d[both] - rc[both]) / rc[both]) < 1e-4


@pytest.mark.parametrize("cat", ["bottle", "mug", "chair", "table"])
def test_pose_draws_stay_in_the_reference_ranges(cat):
    rng = np.random.default_rng(3)
    nocs = cat in ("bottle", "mug")
    for _ in range(300):
        Rm, t = M.draw_pose(rng, nocs)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(Rm), 1)
        lim, z = (0.3, (0.6, 2.0)) if nocs else (0.2, (1.0, 5.0))
        assert abs(t[0]) <= lim and abs(t[1]) <= lim and z[0] <= -t[2] <= z[1]
        # the tilt of the object's up axis towards the camera: x in [25, 65] deg (NOCS, +-15 for the yy turn) / [10, 70]
        up = Rm[:, 1]
        tilt = np.degrees(np.arccos(np.clip(up[1], -1, 1)))
        if nocs:
            assert 25 - 1e-9 <= tilt <= 65 + 1e-9
        else:
            assert 10 - 1e-9 <= tilt <= 70 + 1e-9
    lo, hi = CATEGORIES[cat].scale_range
    assert 0 < lo < hi and CATEGORIES[cat].npoint_max == 10000


def test_model_matrix_and_half_extents():
    bmin, bmax = np.array([-1.0, 0.0, 2.0]), np.array([3.0, 1.0, 4.0])
    m = M.model_matrix(np.eye(3), [0.1, 0.2, -1.0], 0.5, bmin, bmax)
    c = np.append((bmin + bmax) / 2, 1.0)
    assert np.allclose(m @ c, [0.1, 0.2, -1.0, 1.0])
    assert np.allclose(M.view_half_extents(bmin, bmax, 0.5), [0.5, 0.25, 1.0])     # x and z swapped
    assert np.allclose(M.roty(0.3)[:3, :3] @ [1, 0, 0], [np.cos(0.3), 0, np.sin(0.3)])   # the reference's sign convention
