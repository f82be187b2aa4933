"""TabletopFrameSampler's host draws without a device: the seeded-generator contract, every object upright on the table with its box's
bottom face in the plane, footprints kept min_gap apart (and in contact at min_gap = 0), the refusals, the table's rectangle against
the view frustum, and the restatement's render of a draw: the table is the last instance, keeps label -1 and loses ties."""
import numpy as np
import pytest

import mesh_frames_ref as FR
import mesh_ref as R
from cppf_amd import mesh_frames as MF
from cppf_amd import meshes as M

W, H, FX, FY = 96, 72, M.FX * 96 / 640, M.FY * 72 / 480            # the dataset's camera at 0.15 of its resolution


def _unit(m):
    """a mesh scaled to a unit box diagonal, as the datasets' meshes are (the configs' scale ranges are metres per diagonal)"""
    return m[0] / np.linalg.norm(m[0].max(0) - m[0].min(0)), m[1]


_MESHES = {"bottle": [_unit(R.necked_cylinder(0.15, 0.45, n_lon=12))], "bowl": [_unit(R.uv_sphere(0.3, 6, 8))],
           "camera": [_unit(R.box(0.3, 0.2, 0.15))], "can": [_unit(R.necked_cylinder(0.2, 0.3, neck=0.9, n_lon=10))],
           "laptop": [_unit(R.box(0.4, 0.05, 0.3)), _unit(R.box(0.35, 0.3, 0.04))], "mug": [_unit(R.box(0.25, 0.2, 0.2))]}
SEEDS = range(8)


def _sampler(seed, n=4, **kw):
    return MF.TabletopFrameSampler(_MESHES, n, seed=seed, fx=FX, fy=FY, width=W, height=H, **dict(dict(z_range=(0.6, 1.8)), **kw))


def test_the_same_seed_gives_the_same_spec():
    a, b, c = _sampler(7), _sampler(7), _sampler(8)
    for _ in range(3):
        sa, sb, sc = a.draw(), b.draw(), c.draw()
        assert sa["categories"] == sb["categories"] and sa["tilt"] == sb["tilt"]
        for key in ("inst_mesh", "scales", "Rs", "ts", "radii", "model_views", "centers", "gt_Rs", "half_extents", "up", "table_point", "feet",
                    "footprints"):
            assert np.array_equal(sa[key], sb[key]), key
        assert all(np.array_equal(x, y) for x, y in zip(sa["quad"], sb["quad"]))
        assert not np.array_equal(sa["ts"], sc["ts"]) and sa["tilt"] != sc["tilt"]
        assert sa["model_views"].shape == (5, 4, 4) and sa["inst_mesh"].tolist()[-1] == a.plane_mesh == len(a.meshes) - 1
        assert np.deg2rad(25) <= sa["tilt"][0] <= np.deg2rad(65) and abs(sa["tilt"][1]) <= np.deg2rad(15)


@pytest.mark.parametrize("min_gap", [0.0, 0.05])
def test_objects_stand_upright_on_the_plane_and_keep_their_distance(min_gap):
    contacts, closest = 0, np.inf
    for seed in SEEDS:
        s = _sampler(seed, min_gap=min_gap)
        sp = s.draw()
        up, o = sp["up"], sp["table_point"]
        assert abs(np.linalg.norm(up) - 1) < 1e-12 and up[1] > 0 and up[2] > 0 and up @ o < 0          # the camera looks down at the table
        for k in range(4):
            m = sp["inst_mesh"][k]
            v, f = s.meshes[m]
            bmin, bmax = s.bounds[m]
            mv = sp["model_views"][k]
            # the eight corners of the mesh's box, posed: the four of the bottom face lie in the plane, the others above it
            box = np.array([[x, y, z] for x in (bmin[0], bmax[0]) for y in (bmin[1], bmax[1]) for z in (bmin[2], bmax[2])])
            hgt = (box @ mv[:3, :3].T + mv[:3, 3] - o) @ up
            assert np.all(np.abs(hgt[[0, 1, 4, 5]]) <= 1e-9) and np.all(hgt[[2, 3, 6, 7]] > 1e-3), (seed, k, hgt)
            # the object's up axis (the mesh's +y) is parallel to the plane normal; the rotation is proper
            axis = mv[:3, 1] / np.linalg.norm(mv[:3, 1])
            assert np.linalg.norm(np.cross(axis, up)) <= 1e-12 and axis @ up > 0
            assert np.allclose(sp["Rs"][k].T @ sp["Rs"][k], np.eye(3), atol=1e-12) and np.linalg.det(sp["Rs"][k]) == pytest.approx(1.0)
            # every vertex is on or above the table and inside its footprint circle about the foot
            cam = v[np.unique(f)] @ mv[:3, :3].T + mv[:3, 3]
            assert np.all((cam - o) @ up >= -1e-9)
            flat = (cam - sp["feet"][k]) - np.outer((cam - sp["feet"][k]) @ up, up)
            assert np.all(np.linalg.norm(flat, axis=1) <= sp["footprints"][k] + 1e-9)
            assert abs((sp["feet"][k] - o) @ up) <= 1e-9 and s.z_range[0] <= -sp["ts"][k][2] <= s.z_range[1]
            for j in range(k):
                gap = np.linalg.norm(sp["feet"][k] - sp["feet"][j]) - sp["footprints"][k] - sp["footprints"][j]
                assert gap >= min_gap, (seed, k, j, gap)
                closest = min(closest, gap)
                contacts += gap <= min_gap + 1e-3
    print(f"min_gap {min_gap}: closest pair {closest:.3e} m beyond its footprints, {contacts} contacts within 1 mm over {len(SEEDS)} seeds")
    assert contacts >= 1                                                       # the placement rule moves a colliding draw INTO contact


def test_refusals():
    with pytest.raises(RuntimeError, match="placements in a row"):
        _sampler(0, n=40, z_range=(0.5, 0.6), max_attempts=5).draw()
    with pytest.raises(ValueError, match="instances"):
        _sampler(0, n=MF.MAX_INSTANCES)
    with pytest.raises(ValueError, match="min_gap"):
        _sampler(0, min_gap=-0.01)
    assert _sampler(0, n=1).n_objects == 1 and MF.MAX_INSTANCES == 65536


def _in_quad(p, quad, slack=1e-9):
    centre, e1, e2, half = quad
    q = p - centre
    return abs(q @ e1) <= half[0] + slack and abs(q @ e2) <= half[1] + slack


@pytest.mark.parametrize("seed", SEEDS)
def test_the_plane_quad_covers_the_frustum_at_the_far_range(seed):
    s = _sampler(seed)
    sp = s.draw()
    up, o, quad = sp["up"], sp["table_point"], sp["quad"]
    far, tx, ty = s.z_range[1], W / (2 * FX), H / (2 * FY)
    assert abs(up @ (quad[0] - o)) <= 1e-12 and abs(quad[1] @ up) <= 1e-12 and abs(quad[2] @ up) <= 1e-12
    # the four corner rays: where one reaches the table within the far range, the table is there
    hits = 0
    for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        ray = np.array([sx * tx, sy * ty, -1.0])
        lam = (up @ o) / (up @ ray)
        if 0 < lam <= far:
            hits += 1
            assert _in_quad(lam * ray, quad), (sx, sy)
    assert hits >= 2                                                           # the bottom corners see the table
    # every ray of the image (a grid over the full frame, corners included) that reaches the table within the far range hits the quad
    for a in np.linspace(-1, 1, 21):
        for b in np.linspace(-1, 1, 21):
            ray = np.array([a * tx, b * ty, -1.0])
            lam = (up @ o) / (up @ ray)
            if 0 < lam <= far:
                assert _in_quad(lam * ray, quad)
    # the posed PLANE_MESH is that rectangle, facing the camera
    mv = sp["model_views"][-1]
    v = MF.PLANE_MESH[0] @ mv[:3, :3].T + mv[:3, 3]
    assert all(abs((p - o) @ up) <= 1e-9 for p in v)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    assert n @ up > 0 and np.linalg.det(mv[:3, :3] / np.array([quad[3][0], 1.0, quad[3][1]])) == pytest.approx(1.0)
    span = [(v - quad[0]) @ quad[1], (v - quad[0]) @ quad[2]]
    assert np.allclose(np.abs(span[0]), quad[3][0]) and np.allclose(np.abs(span[1]), quad[3][1])


def test_the_restatements_render_of_a_draw():
    """tests/mesh_frames_ref.py's render of one draw: the table is instance K, shows between the objects, and where an object's bottom
    meets it the object wins; frame() of the relabelled images is a MeshFrame of the K objects"""
    s = _sampler(2, n=3, z_range=(0.6, 1.0))
    sp = s.draw()
    depth, labels = FR.raster_instances_ref(s.meshes, sp["inst_mesh"], sp["model_views"], FX, FY, W, H)
    K = 3
    assert set(np.unique(labels)) <= {-1, 0, 1, 2, K} and (labels == K).sum() > 0.3 * W * H and sum((labels == k).sum() > 20 for k in range(K)) >= 2
    alone, _ = FR.raster_instances_ref(s.meshes, sp["inst_mesh"][-1:], sp["model_views"][-1:], FX, FY, W, H)
    objs, olab = FR.raster_instances_ref(s.meshes, sp["inst_mesh"][:-1], sp["model_views"][:-1], FX, FY, W, H)
    # the composition rule: the nearer of (objects, table), the objects on a tie
    want = np.where((olab >= 0) & ((alone == 0) | (objs <= alone)), olab, np.where(alone > 0, K, -1))
    assert np.array_equal(labels, want)
    assert np.all(depth[labels == K] == alone[labels == K]) and np.all(depth[labels == K] > 0)
    fr = s.frame(sp, depth, np.where(labels == K, -1, labels).astype(np.int32))
    assert len(fr.categories) == K and fr.visible_pixels.sum() == (olab >= 0).sum() - ((olab >= 0) & (labels == K)).sum()
    assert (fr.depth_mm > 0).sum() == (labels >= 0).sum() and len(fr.gt_poses(1)) == len(fr.instances(1)) == len(fr.visible(1))
    rec = fr.record(fr.gt_poses(1), min_pixels=1)
    assert len(rec["gt_RTs"]) == K
