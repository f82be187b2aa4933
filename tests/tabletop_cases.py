"""What the tabletop tests share (cppf_amd/mesh_frames.py: TabletopFrameSampler; tests/test_gpu_tabletop.py): the small camera, the
meshes, the sampler, the bounds a segmentation of such a frame is held to, and `qualify`: those bounds through the restatements alone
(tests/mesh_frames_ref.py's render, tests/concave_ref.py, tests/segments_ref.py) -- how the sampler seeds of the device test were
chosen."""
import numpy as np

import concave_ref as C
import mesh_frames_ref as FR
import mesh_ref as MR
import segments_ref as R
from cppf_amd import mesh_frames as MF
from cppf_amd import meshes as M

W, H = 320, 240
FX, FY = M.FX * W / 640, M.FY * H / 480                                       # the dataset's camera at half its resolution
N_OBJECTS, Z_RANGE = 3, (0.6, 1.2)
CONCAVE = dict(radius=3, step=4, tol_mm=10, slope_permille=10, min_count=16, cos_max=float(np.cos(np.deg2rad(30.0))), span_max=0.08)
MIN_PIXELS = 200


def _unit(v):
    return v / np.linalg.norm(v.max(0) - v.min(0))


def meshes():
    """CONVEX objects only -- a plain cylinder and a box.  They are filed under "bottle" and "camera" only because the sampler takes an
    object's size from a category's config; they are not bottles or cameras.  The bounds of tests/test_gpu_tabletop.py hold for such
    objects and are NOT claimed for others: a real bottle's shoulder is a concave crease of its own, the rule cuts it, and with 3.7j's
    necked bottle 1 sampler seed of 12 met the bounds (where the AP of the necked bottles is measured)."""
    b, c = MR.lathe([(0, -0.45), (0.15, -0.45), (0.15, 0.45), (0, 0.45)], 32), MR.box(0.3, 0.2, 0.15)[:2]
    return {"bottle": [(_unit(b[0]), b[1])], "camera": [(_unit(c[0]), c[1])]}


def sampler(seed, dev=None, min_gap=0.0):
    return MF.TabletopFrameSampler(meshes(), N_OBJECTS, device=dev, seed=seed, z_range=Z_RANGE, min_gap=min_gap, fx=FX, fy=FY, width=W, height=H)


def bounds(seg_labels, gt):
    """gt: the ground-truth label image with the table as label N_OBJECTS (-1: nothing).  Returns (the smallest share of a kept
    segment's pixels under one ground-truth label, the smallest share of an object of >= 500 pixels held by one segment, the number
    of kept segments that hold both table and object pixels)"""
    pur, own, mixed = [], [], 0
    for s in range(int(seg_labels.max()) + 1):
        g = gt[seg_labels == s]
        cnt = np.bincount(g[g >= 0], minlength=N_OBJECTS + 1)
        pur.append(cnt.max() / g.size)
        mixed += bool(cnt[N_OBJECTS] and cnt[:N_OBJECTS].sum())
    for k in range(N_OBJECTS):
        m = gt == k
        if m.sum() >= 500:
            segs = seg_labels[m]
            segs = segs[segs >= 0]
            own.append(np.bincount(segs).max() / m.sum() if segs.size else 0.0)
    return (min(pur) if pur else 0.0), (min(own) if own else 0.0), mixed


def ref_frame(seed, min_gap=0.0):
    """(sampler, spec, depth f32[H,W], labels i32[H,W] with the table as N_OBJECTS) of the restatement's render of sampler(seed)'s
    first draw"""
    s = sampler(seed, min_gap=min_gap)
    spec = s.draw()
    depth, labels = FR.raster_instances_ref(s.meshes, spec["inst_mesh"], spec["model_views"], FX, FY, W, H)
    return s, spec, depth, labels


def cut_and_plain(depth_mm, intrinsics):
    """the restatements' label images of a frame with the concave cut and without it"""
    K = np.asarray(intrinsics, np.float64)
    edge = C.concave_ref(depth_mm, None, K[0, 0], K[1, 1], K[0, 2], K[1, 2], **CONCAVE)["edge"]
    return (R.segments_ref(depth_mm, edge == 0, min_pixels=MIN_PIXELS)["labels"], R.segments_ref(depth_mm, None, min_pixels=MIN_PIXELS)["labels"])


def qualify(seed):
    """dict(purity, held, objects of >= 500 pixels, mixed segments without the cut, contact: the smallest footprint gap in metres, ok)"""
    _, spec, depth, labels = ref_frame(seed)
    cut, plain = cut_and_plain(MF.depth_to_mm(depth), MF.frame_intrinsics(FX, FY, W, H))
    pur, own, _ = bounds(cut, labels)
    _, _, mixed = bounds(plain, labels)
    big = int(sum((labels == k).sum() >= 500 for k in range(N_OBJECTS)))
    gaps = [np.linalg.norm(spec["feet"][i] - spec["feet"][j]) - spec["footprints"][i] - spec["footprints"][j]
            for i in range(N_OBJECTS) for j in range(i)]
    return dict(purity=float(pur), held=float(own), big=big, mixed_plain=int(mixed), contact=float(min(gaps)),
                ok=bool(pur >= 0.99 and own >= 0.80 and big >= 1 and mixed >= 1))
