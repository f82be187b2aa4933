"""Mesh frames without a device: the numpy restatement of cppf_raster_instances against an independent ray caster, the frame
convention (intrinsics and axis flips) on a slanted plane, the ground-truth records through the host evaluation, and the sampler's
host draws."""
import numpy as np
import pytest

import mesh_frames_ref as FR
import mesh_ref as R
from cppf_amd import evaluation as E
from cppf_amd import mesh_frames as MF
from cppf_amd import meshes as M

W, H, FX, FY = 96, 72, M.FX * 96 / 640, M.FY * 72 / 480            # the dataset's camera at 0.15 of its resolution


def _scene():
    """three objects, the second partly hidden behind the first, none intersecting"""
    meshes = [R.box(0.3, 0.2, 0.15)[:2], R.uv_sphere(0.25, 6, 8), R.necked_cylinder(0.12, 0.35, n_lon=12)]
    inst = [0, 1, 2, 1]
    mvs = [FR.model([-0.15, 0.0, -1.0], FR.rot(0.5, 0.4)), FR.model([0.1, 0.05, -1.6], FR.rot(0.2, 0.1)),
           FR.model([0.45, -0.1, -1.2], FR.rot(1.0, 0.6)), FR.model([-0.3, 0.2, -2.2], FR.rot(0.3, 0.9), 1.5)]
    return meshes, inst, mvs


def test_restatement_agrees_with_the_ray_caster():
    meshes, inst, mvs = _scene()
    depth, labels = FR.raster_instances_ref(meshes, inst, mvs, FX, FY, W, H)
    rdepth, rlabels = FR.ray_cast_instances(meshes, inst, mvs, FX, FY, W, H)
    covered = (labels >= 0) | (rlabels >= 0)
    assert covered.sum() > 800 and set(np.unique(labels)) == {-1, 0, 1, 2, 3}
    assert ((labels == 1) & (depth > 0)).sum() < ((FR.raster_instances_ref(meshes, [1], [mvs[1]], FX, FY, W, H)[1]) == 0).sum()  # occluded
    near_edge = FR.edge_distance_instances(meshes, inst, mvs, FX, FY, W, H) < 1e-3
    # the pixels where the ray caster itself is undecided (a centre on an edge to 1e-3 px) stay inside the cap
    assert (near_edge & covered).sum() <= 0.01 * covered.sum()
    differ = labels != rlabels
    assert not (differ & ~near_edge).any(), int((differ & ~near_edge).sum())
    assert differ.sum() <= 0.01 * covered.sum()
    same = (labels >= 0) & ~differ
    assert np.max(np.abs(depth[same] - rdepth[same]) / rdepth[same]) < 1e-5


def test_single_instance_restatement_is_the_single_render():
    meshes, inst, mvs = _scene()
    depth, labels = FR.raster_instances_ref(meshes, [2], [mvs[2]], FX, FY, W, H)
    one = R.raster_ref(*meshes[2], mvs[2], FX, FY, W, H)
    assert np.array_equal(depth.view(np.uint32), one.view(np.uint32)) and np.array_equal(labels, np.where(one > 0, 0, -1))


def _plane_residual(depth, K, flip, n_gl, c):
    """largest distance (metres) of the back-projected points from the plane n_gl . p = c given in the render's camera frame,
    when frame coordinates are taken to be flip . (camera coordinates)"""
    p = FR.frame_points_ref(depth, K)
    n_f = flip @ n_gl                                       # (flip is orthogonal and symmetric)
    return float(np.max(np.abs(p @ n_f - c)) / np.linalg.norm(n_gl))


def test_frame_convention_on_a_slanted_plane():
    # the plane z = -1.2 + 0.3 x - 0.2 y in the render's camera frame, as one quad that covers the whole image
    zc = lambda x, y: -1.2 + 0.3 * x - 0.2 * y
    v = np.array([[x, y, zc(x, y)] for x, y in ((-1.5, -1.2), (1.5, -1.2), (1.5, 1.2), (-1.5, 1.2))])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    depth, labels = FR.raster_instances_ref([(v, f)], [0], [np.eye(4)])
    assert (labels == 0).all() and depth.min() > 0.5
    n_gl, c = np.array([0.3, -0.2, -1.0]), 1.2              # 0.3 x - 0.2 y - z = 1.2
    K = MF.frame_intrinsics()
    assert np.array_equal(K, [[M.FX, 0, M.WIDTH / 2 - 0.5], [0, M.FY, M.HEIGHT / 2 - 0.5], [0, 0, 1]])
    res = _plane_residual(depth, K, MF.FRAME_FROM_GL, n_gl, c)
    print("plane residual", res)
    assert res <= 1e-5
    # the test decides: neither a principal point at the image centre nor another pair of flips passes
    K_centre = np.array([[M.FX, 0, M.WIDTH / 2], [0, M.FY, M.HEIGHT / 2], [0, 0, 1]])
    assert _plane_residual(depth, K_centre, MF.FRAME_FROM_GL, n_gl, c) > 1e-4
    for other in (np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, 1.0, -1.0])):
        assert _plane_residual(depth, K, other, n_gl, c) > 1e-2


_NOCS_MESHES = {"bottle": [R.necked_cylinder(0.15, 0.45, n_lon=12)], "bowl": [R.uv_sphere(0.3, 6, 8)],
                "camera": [R.box(0.3, 0.2, 0.15)[:2]], "can": [R.necked_cylinder(0.2, 0.3, neck=0.9, n_lon=10)],
                "laptop": [R.box(0.4, 0.05, 0.3)[:2], R.box(0.35, 0.3, 0.04)[:2]], "mug": [R.box(0.25, 0.2, 0.2)[:2]]}


def _sampler(seed, n=5, **kw):
    return MF.MeshFrameSampler(_NOCS_MESHES, n, seed=seed, fx=FX, fy=FY, width=W, height=H, **kw)


@pytest.fixture(scope="module")
def cpu_frame():
    s = _sampler(3, z_range=(0.5, 1.0))
    spec = s.draw()
    meshes = s.meshes
    depth, labels = FR.raster_instances_ref(meshes, spec["inst_mesh"], spec["model_views"], FX, FY, W, H)
    return s, spec, s.frame(spec, depth, labels)


def test_ground_truth_boxes_hold_the_posed_meshes(cpu_frame):
    s, spec, fr = cpu_frame
    assert np.array_equal(fr.intrinsics, MF.frame_intrinsics(FX, FY, W, H))
    for k, m in enumerate(spec["inst_mesh"]):
        v, f = s.meshes[m]
        used = v[np.unique(f)]
        cam = used @ spec["model_views"][k][:3, :3].T + spec["model_views"][k][:3, 3]
        q = (cam @ MF.FRAME_FROM_GL.T - fr.centers[k]) @ fr.Rs[k]                  # R^T (p - centre), row-wise
        assert np.all(np.abs(q) <= fr.half_extents[k] + 1e-9), (k, fr.categories[k])
        assert np.abs(q).max(0) == pytest.approx(fr.half_extents[k], abs=1e-9)     # and the box is tight
        assert np.linalg.det(fr.gt_RTs[k][:3, :3]) > 0
        assert np.allclose(fr.Rs[k].T @ fr.Rs[k], np.eye(3), atol=1e-12) and np.linalg.det(fr.Rs[k]) == pytest.approx(1.0)
        size = 2 * fr.half_extents[k]
        assert np.allclose(fr.gt_RTs[k][:3, :3], fr.Rs[k] * np.linalg.norm(size)) and np.allclose(fr.gt_scales[k] * np.linalg.norm(size), size)
        assert np.array_equal(fr.gt_RTs[k][3], [0, 0, 0, 1]) and np.array_equal(fr.gt_RTs[k][:3, 3], fr.centers[k])
        # the rendered surface of the instance, back-projected the frame path's way, lies in its box too (pixel-centre depth: exact
        # to rounding)
        p = FR.frame_points_ref(fr.depth.numpy(), fr.intrinsics, fr.labels.numpy() == k)
        if len(p):
            assert np.all(np.abs((p - fr.centers[k]) @ fr.Rs[k]) <= fr.half_extents[k] + 1e-5), k


def test_record_of_the_ground_truth_scores_ap_one_on_the_host(cpu_frame):
    s, spec, fr = cpu_frame
    vis = fr.visible(1)
    assert len(vis) >= 3 and fr.visible_pixels.sum() == int((fr.labels >= 0).sum())
    assert [c for c, _ in fr.instances(1)] == [fr.categories[k] for k in vis]
    assert all(np.array_equal(m, fr.labels.numpy() == k) for (_, m), k in zip(fr.instances(1), vis))
    assert np.array_equal(fr.depth_mm, np.minimum(65535, np.rint(1000.0 * fr.depth.numpy().astype(np.float64))).astype(np.uint16))
    rec = fr.record(fr.gt_poses(1), min_pixels=1)
    deg, sh, iou = [5, 10, 15], [5, 10, 15], [0.25, 0.5, 0.75, 0.9]
    iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP([rec], fr.synset_names, None, deg, sh, iou, 0.1, False)
    seen = sorted({int(c) for c in rec["gt_class_ids"][vis]})
    hidden = [k for k in range(len(fr.categories)) if k not in vis]
    full = [c for c in seen if not any(rec["gt_class_ids"][k] == c for k in hidden)]
    assert full
    for c in full:                                                                 # classes whose every instance was predicted
        assert np.all(iou_aps[c] == 1.0) and np.all(pose_aps[c] == 1.0), (c, iou_aps[c], pose_aps[c])
    # an instance without a prediction stays as unmatched ground truth: its class loses recall
    rec2 = fr.record([None] + fr.gt_poses(1)[1:], min_pixels=1)
    assert len(rec2["pred_RTs"]) == len(vis) - 1 and len(rec2["gt_RTs"]) == len(fr.categories)
    iou2, _, _, _ = E.compute_degree_cm_mAP([rec2], fr.synset_names, None, deg, sh, iou, 0.1, False)
    assert np.all(iou2[rec["gt_class_ids"][vis[0]]] < 1.0)
    with pytest.raises(ValueError, match="poses for"):
        fr.record(fr.gt_poses(1)[:-1], min_pixels=1)


def test_sampler_is_deterministic_and_places_disjoint_spheres():
    a, b, c = _sampler(7, n=6), _sampler(7, n=6), _sampler(8, n=6)
    for _ in range(3):
        sa, sb, sc = a.draw(), b.draw(), c.draw()
        assert sa["categories"] == sb["categories"]
        for key in ("inst_mesh", "scales", "Rs", "ts", "radii", "model_views", "centers", "gt_Rs", "half_extents"):
            assert np.array_equal(sa[key], sb[key]), key
        assert not np.array_equal(sa["ts"], sc["ts"])
        ts, rr = sa["ts"], sa["radii"]
        for i in range(6):
            v, f = a.meshes[sa["inst_mesh"][i]]
            cam = v[np.unique(f)] @ sa["model_views"][i][:3, :3].T + sa["model_views"][i][:3, 3]
            assert np.all(np.linalg.norm(cam - ts[i], axis=1) <= rr[i] + 1e-12)    # the sphere holds the posed mesh
            assert a.z_range[0] <= -ts[i][2] <= a.z_range[1]
            for j in range(i):
                assert np.linalg.norm(ts[i] - ts[j]) > rr[i] + rr[j]
    with pytest.raises(RuntimeError, match="placements in a row"):
        _sampler(0, n=40, z_range=(0.5, 0.6), max_attempts=5).draw()
