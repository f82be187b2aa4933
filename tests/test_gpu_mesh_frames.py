"""Mesh frames on the MI355X: cppf_raster_instances against its numpy restatement (tests/mesh_frames_ref.py) bit for bit, against
the composition of single renders, with one instance against render_depth, the item-to-instance mapping across workgroups, the
error codes, and a sampled frame through the frame path's clouds and the device evaluation."""
import numpy as np
import pytest
import torch

import mesh_frames_ref as FR
import mesh_ref as R
from cppf_amd import _lib, frames
from cppf_amd import evaluation as E
from cppf_amd import mesh_frames as MF
from cppf_amd import meshes as M
from cppf_amd.config import CATEGORIES

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _scene():
    """three boxes (12 faces each) and one 80-face sphere drawn twice; the boxes overlap in the image, the spheres intersect a box"""
    meshes = [R.box(0.3, 0.2, 0.15)[:2], R.box(0.1, 0.4, 0.1)[:2], R.box(0.25, 0.25, 0.25)[:2], R.uv_sphere(0.25, 6, 8)]
    inst = [0, 3, 1, 2, 3]
    mvs = [FR.model([-0.2, 0.0, -1.0], FR.rot(0.5, 0.4)), FR.model([-0.05, 0.05, -0.95], FR.rot(0.2, 0.1)),
           FR.model([0.1, 0.0, -0.8], FR.rot(1.0, 0.6)), FR.model([0.3, -0.1, -1.4], FR.rot(0.3, 0.9)),
           FR.model([0.35, 0.2, -1.2], FR.rot(2.0, 0.3), 0.7)]
    return meshes, inst, mvs


@pytest.mark.parametrize("cull", [True, False], ids=["cull", "nocull"])
@pytest.mark.parametrize("size", [(40, 24), (640, 480)], ids=["40x24", "640x480"])
def test_instances_are_bit_exact_against_the_restatement(dev, size, cull):
    W, H = size                                                     # 40 x 24: 3 x 2 tiles, partial in both directions
    fx, fy = M.FX * W / 640, M.FY * H / 480
    meshes, inst, mvs = _scene()
    depth, labels = M.render_instances(meshes, inst, mvs, cull=cull, fx=fx, fy=fy, width=W, height=H, device=dev)
    rd, rl = FR.raster_instances_ref(meshes, inst, mvs, fx, fy, W, H, cull=cull)
    assert set(np.unique(rl)) == {-1, 0, 1, 2, 3, 4}
    assert depth.dtype == torch.float32 and labels.dtype == torch.int32 and depth.shape == labels.shape == (H, W)
    d, l = depth.cpu().numpy(), labels.cpu().numpy()
    assert np.array_equal(l, rl), int((l != rl).sum())
    assert _bits_equal(d, rd), float(np.abs(d - rd).max())


def test_composition_identity_against_the_single_render(dev):
    W, H = 200, 152                                                 # 12.5 x 9.5 tiles
    fx, fy = M.FX * W / 640, M.FY * H / 480
    v0, f0 = R.box(0.2, 0.2, 0.2)[:2]
    v_deg = np.vstack([v0, [[0.0, 0.0, 0.3], [0.1, 0.1, 0.3], [0.2, 0.2, 0.3]]])          # zero-area faces beside real ones
    f_deg = np.vstack([f0, [[0, 0, 1], [8, 9, 10], [3, 3, 3]]]).astype(np.int32)
    meshes = [R.box(0.35, 0.3, 0.1)[:2], R.uv_sphere(0.1, 6, 8), R.box(0.1, 0.1, 0.1)[:2], (v_deg, f_deg)]
    inst = [0, 1, 2, 2, 2, 3, 1, 1]
    mvs = [FR.model([0.0, 0.0, -1.0], FR.rot(0.1, 0.1)),           # 0: the occluder
           FR.model([0.0, 0.0, -2.0]),                              # 1: entirely hidden behind 0
           FR.model([0.12, -0.08, -0.12], FR.rot(0.5, 0.3)),        # 2: crosses the near plane
           FR.model([0.0, 0.0, 1.0]),                               # 3: behind the camera
           FR.model([40.0, 0.0, -1.0]),                             # 4: off screen
           FR.model([-0.55, 0.3, -1.3], FR.rot(0.4, 0.2)),          # 5: the mesh with zero-area faces
           FR.model([0.6, 0.42, -1.3]), FR.model([0.6, 0.42, -1.3])]   # 6, 7: the same mesh and matrix twice
    for cull in (True, False):
        depth, labels = M.render_instances(meshes, inst, mvs, cull=cull, fx=fx, fy=fy, width=W, height=H, device=dev)
        singles = [M.render_depth(*meshes[m], mv, cull=cull, fx=fx, fy=fy, width=W, height=H, device=dev).cpu().numpy()
                   for m, mv in zip(inst, mvs)]
        stack = np.stack([np.where(s > 0, s, np.inf) for s in singles])
        want_d = stack.min(0)
        want_l = np.where(np.isinf(want_d), -1, stack.argmin(0)).astype(np.int32)      # argmin: the first of equal minima
        want_d = np.where(np.isinf(want_d), 0, want_d).astype(np.float32)
        d, l = depth.cpu().numpy(), labels.cpu().numpy()
        assert np.array_equal(l, want_l) and _bits_equal(d, want_d), cull
        seen = set(np.unique(l))
        assert seen == {-1, 0, 2, 5, 6}, seen                       # 1 hidden, 3 behind, 4 off screen, 7 loses every tie to 6
        assert (singles[1] > 0).sum() > 20 and (singles[2] > 0).sum() > 200 and not (singles[3] > 0).any() and not (singles[4] > 0).any()
        assert np.array_equal(singles[6], singles[7]) and (l == 6).sum() > 500      # the lower index owns every shared pixel


def test_one_instance_is_the_single_render(dev):
    v, f = R.necked_cylinder(0.15, 0.45, n_lon=32)
    mv = FR.model([-0.1, 0.05, -1.6], FR.rot(1.1, 0.7))
    depth, labels = M.render_instances([(v, f)], [0], [mv], device=dev)
    one = M.render_depth(v, f, mv, device=dev)
    assert (one > 0).sum() > 1000 and torch.equal(depth.view(torch.int32), one.view(torch.int32))
    assert torch.equal(labels, torch.where(one > 0, 0, -1).to(torch.int32))


def test_item_to_instance_mapping_across_workgroups(dev):
    # meshes of 12, 250 and 7 faces: the 256-item blocks of the set-up kernel span two instances (items 0..255: 12 + 244) and three
    # (256..511: 6 + 7 + 243), and instance boundaries fall anywhere in a block
    box = R.box(0.1, 0.08, 0.06)[:2]
    sph = R.uv_sphere(0.1, 6, 25)
    seven = (box[0], box[1][:7].copy())
    assert [m[1].shape[0] for m in (box, sph, seven)] == [12, 250, 7]
    meshes = [box, sph, seven]
    inst = [0, 1, 2, 1, 0, 2, 2, 1, 0]
    W, H = 320, 240
    fx, fy = M.FX / 2, M.FY / 2
    mvs = [FR.model([-0.4 + 0.27 * (k % 3), -0.3 + 0.3 * (k // 3), -1.2], FR.rot(0.3 * k, 0.2 + 0.1 * k)) for k in range(9)]
    depth, labels = M.render_instances(meshes, inst, mvs, cull=False, fx=fx, fy=fy, width=W, height=H, device=dev)
    rd, rl = FR.raster_instances_ref(meshes, inst, mvs, fx, fy, W, H, cull=False)
    assert set(np.unique(rl)) == set(range(-1, 9))
    assert np.array_equal(labels.cpu().numpy(), rl) and _bits_equal(depth.cpu().numpy(), rd)
    # 300 two-triangle quads on a 20 x 15 grid of 32-pixel cells: every index owns pixels, and only inside its own cell
    quad = (np.array([[-0.01, -0.01, 0.0], [0.01, -0.01, 0.0], [0.01, 0.01, 0.0], [-0.01, 0.01, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    K = 300
    mvs = [FR.model([((k % 20) * 32 + 16 - 320) / M.FX, -((k // 20) * 32 + 16 - 240) / M.FY, -1.0]) for k in range(K)]
    depth, labels = M.render_instances([quad], np.zeros(K, np.int32), mvs, device=dev)
    l = labels.cpu().numpy()
    counts = np.bincount(l[l >= 0], minlength=K)
    assert counts.shape[0] == K and counts.min() >= 100 and counts.max() <= 12 * 12 + 24, (counts.min(), counts.max())
    rows, cols = np.nonzero(l >= 0)
    assert np.array_equal(l[rows, cols], (rows // 32) * 20 + cols // 32)
    rd, rl = FR.raster_instances_ref([quad], np.zeros(K, np.int32), mvs)
    assert np.array_equal(l, rl) and _bits_equal(depth.cpu().numpy(), rd)


def test_errors_are_codes_and_fill_both_images(dev):
    meshes, inst, mvs = _scene()
    W, H = 40, 24
    kw = dict(fx=M.FX * W / 640, fy=M.FY * H / 480, width=W, height=H, device=dev)
    out = (torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.int32, device=dev))
    with pytest.raises(_lib.CppfError, match=r"cppf_raster_instances failed \(-5\)"):        # CPPF_ECAPACITY
        M.render_instances(meshes, inst, mvs, max_bin_entries=1, out=out, **kw)
    assert torch.isnan(out[0]).all() and (out[1] == -1).all()
    # a face of the FIRST mesh names vertex 8: inside the concatenated array, outside its own mesh's 8 vertices
    bad = [(meshes[0][0], np.vstack([meshes[0][1], [[0, 1, 8]]]).astype(np.int32))] + meshes[1:]
    out[0].zero_(), out[1].zero_()
    with pytest.raises(_lib.CppfError, match=r"cppf_raster_instances failed \(-1\)"):        # CPPF_EINVAL, through the status words
        M.render_instances(bad, inst, mvs, out=out, **kw)
    assert torch.isnan(out[0]).all() and (out[1] == -1).all()
    # an instance that names no mesh: refused on the host, nothing launched, nothing written
    out[0].fill_(7.0), out[1].fill_(7)
    for wrong in (4, -1):
        with pytest.raises(_lib.CppfError, match=r"cppf_raster_instances failed \(-1\)"):
            M.render_instances(meshes, [0, wrong, 1], mvs[:3], out=out, **kw)
    torch.cuda.synchronize(dev)
    assert (out[0] == 7.0).all() and (out[1] == 7).all()
    with pytest.raises(ValueError, match="one matrix per instance"):
        M.render_instances(meshes, inst, mvs[:3], **kw)
    # and the device is in order afterwards
    depth, labels = M.render_instances(meshes, inst, mvs, out=out, **kw)
    assert np.array_equal(labels.cpu().numpy(), FR.raster_instances_ref(meshes, inst, mvs, kw["fx"], kw["fy"], W, H)[1])


def test_bin_list_grows_and_the_render_repeats(dev):
    # 100 frame-filling triangles: 100 x 1200 (primitive, tile) entries, more than the starting capacity of 4 per face + 64 per tile
    tri = R.big_triangle(-1.0)
    K = 100
    mvs = [FR.model([0.0, 0.0, -0.01 * k]) for k in range(K)]
    assert M.default_bin_entries(K) < K * 1200
    ms = M.mesh_set([tri], dev)
    depth, labels = M.render_instances(ms, np.zeros(K, np.int32), mvs, device=dev)
    assert ms.bins[(M.WIDTH, M.HEIGHT)] >= K * 1200                 # grown to what the render reported
    assert (labels == 0).all() and torch.equal(depth, M.render_depth(*tri, mvs[0], device=dev))
    with pytest.raises(_lib.CppfError, match=r"\(-5\)"):           # a fixed capacity does not grow
        M.render_instances(ms, np.zeros(K, np.int32), mvs, device=dev, max_bin_entries=M.default_bin_entries(K))


_NOCS_MESHES = {"bottle": [R.necked_cylinder(0.15, 0.45, n_lon=24)], "camera": [R.box(0.3, 0.2, 0.15)[:2]],
                "laptop": [R.box(0.4, 0.05, 0.3)[:2]], "mug": [R.box(0.25, 0.2, 0.2)[:2]], "bowl": [R.uv_sphere(0.3, 8, 16)]}


def test_sampled_frame_through_the_frame_path_and_the_device_evaluation(dev):
    fr = MF.MeshFrameSampler(_NOCS_MESHES, 3, device=dev, seed=5, z_range=(0.6, 1.2)).sample()
    again = MF.MeshFrameSampler(_NOCS_MESHES, 3, device=dev, seed=5, z_range=(0.6, 1.2)).sample()
    assert torch.equal(fr.depth.view(torch.int32), again.depth.view(torch.int32)) and torch.equal(fr.labels, again.labels)
    assert fr.categories == again.categories and np.array_equal(fr.gt_RTs, again.gt_RTs)
    assert fr.depth.shape == (480, 640) and fr.depth_mm.dtype == np.uint16 and fr.depth_mm.shape == (480, 640)
    assert np.array_equal(fr.visible_pixels, np.bincount(fr.labels.cpu().numpy()[fr.labels.cpu().numpy() >= 0], minlength=3))
    vis = fr.visible(200)
    assert len(vis) >= 2
    for (cat, mask), k in zip(fr.instances(200), vis):
        assert cat == fr.categories[k] and mask.sum() == fr.visible_pixels[k]
        pc, nrm = frames.instance_cloud(fr.depth_mm, fr.intrinsics, mask, CATEGORIES[cat])       # no jitter
        assert pc.shape[0] > 50
        q = (pc.double().cpu().numpy() - fr.centers[k]) @ fr.Rs[k]                              # R^T (p - centre)
        over = np.abs(q) - fr.half_extents[k]
        print(cat, "points", pc.shape[0], "largest excess over the box (m)", float(over.max()))
        assert over.max() <= 1e-3, (k, cat, float(over.max()))    # the millimetre rounding along the ray
    rec = fr.record(fr.gt_poses(200), min_pixels=200)
    deg, sh, iou = [5, 10, 15], [5, 10, 15], [0.25, 0.5, 0.75, 0.9]
    iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP([rec], fr.synset_names, None, deg, sh, iou, 0.1, False, device=dev)
    hidden_classes = {int(rec["gt_class_ids"][k]) for k in range(3) if k not in vis}
    full = sorted({int(rec["gt_class_ids"][k]) for k in vis} - hidden_classes)
    assert full
    for c in full:
        assert np.all(iou_aps[c] == 1.0) and np.all(pose_aps[c] == 1.0), (c, iou_aps[c], pose_aps[c])
    host = E.compute_degree_cm_mAP([rec], fr.synset_names, None, deg, sh, iou, 0.1, False)
    assert np.array_equal(host[0], iou_aps) and np.array_equal(host[1], pose_aps)
