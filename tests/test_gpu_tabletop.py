"""Tabletop frames on the device (cppf_amd/mesh_frames.py: TabletopFrameSampler): the render against tests/mesh_frames_ref.py bit for
bit with the table as the last instance, the MeshFrame it becomes, and what the concave cut does on frames whose objects stand on a
support and touch: frame_segments(n_planes=0, concave=...) separates table and objects, concave=None does not; scene_frame takes the
dict unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concave_ref as C  # noqa: E402
import mesh_frames_ref as FR  # noqa: E402
import segments_ref as R  # noqa: E402
import tabletop_cases as TC  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from cppf_amd import mesh_frames as MF  # noqa: E402
from cppf_amd import _lib, scene_poses, training  # noqa: E402
from cppf_amd import segments as SG  # noqa: E402
from cppf_amd.config import CATEGORIES  # noqa: E402

pytestmark = pytest.mark.gpu

# Sampler seeds (3 CONVEX objects -- tabletop_cases.meshes: a plain cylinder and a box --, min_gap = 0, 320 x 240).  Chosen on the CPU with the restatements alone (tabletop_cases.qualify:
# mesh_frames_ref's render, concave_ref, segments_ref): seeds 0..11 were tried and 8 qualified -- with the cut every kept segment >=
# 0.99 under one ground-truth label (an object or the table), every object of >= 500 pixels >= 0.80 inside one segment (0.81 .. 0.95
# held), and without the cut a segment that mixes table and objects.  Seeds 0, 1, 4 and 7 did not: a segment leaks between the table
# and an object (purity 0.92 .. 0.98).  In 8 and 9 two objects touch (their footprints a nanometre apart).
FRAME_SEEDS = [8, 9, 2]


@pytest.fixture(scope="module", params=FRAME_SEEDS)
def frame(request, dev):
    s = TC.sampler(request.param, dev)
    return request.param, s, s.sample()


def test_render_equals_the_restatement(frame):
    seed, s, fr = frame
    _, spec, depth, labels = TC.ref_frame(seed)
    K = TC.N_OBJECTS
    assert np.array_equal(fr.depth.cpu().numpy().view(np.uint32), depth.view(np.uint32))
    support = fr.spec["support"].cpu().numpy()
    got = fr.labels.cpu().numpy()
    assert np.array_equal(support, labels == K) and np.array_equal(got, np.where(labels == K, -1, labels))
    assert support.sum() > 0.3 * TC.W * TC.H and (depth[support] > 0).all() and (got[support] == -1).all()
    assert sorted(set(np.unique(labels).tolist()) - {-1}) == list(range(K + 1))
    for key in ("model_views", "inst_mesh", "feet", "up"):
        assert np.array_equal(fr.spec[key], spec[key]), key
    # the objects win ties: where the objects' own render and the table's are equally deep the pixel is the object's
    alone, _ = FR.raster_instances_ref(s.meshes, spec["inst_mesh"][-1:], spec["model_views"][-1:], TC.FX, TC.FY, TC.W, TC.H)
    objs, olab = FR.raster_instances_ref(s.meshes, spec["inst_mesh"][:-1], spec["model_views"][:-1], TC.FX, TC.FY, TC.W, TC.H)
    assert np.array_equal(labels, np.where((olab >= 0) & ((alone == 0) | (objs <= alone)), olab, np.where(alone > 0, K, -1)))
    # the same frame through MeshFrame
    assert np.array_equal(fr.depth_mm, MF.depth_to_mm(depth)) and np.array_equal(fr.intrinsics, MF.frame_intrinsics(TC.FX, TC.FY, TC.W, TC.H))
    assert np.array_equal(fr.visible_pixels, np.bincount(labels[(labels >= 0) & (labels < K)], minlength=K))
    inst = fr.instances(100)
    assert len(inst) == len(fr.visible(100)) == len(fr.gt_poses(100)) >= 2
    for (cat, mask), k in zip(inst, fr.visible(100)):
        assert cat == fr.categories[k] and np.array_equal(mask, labels == k)
    assert len(fr.record(fr.gt_poses(100))["gt_RTs"]) == K


def test_the_cut_separates_table_and_objects(frame):
    seed, s, fr = frame
    gt = np.where(fr.spec["support"].cpu().numpy(), TC.N_OBJECTS, fr.labels.cpu().numpy())
    cut = SG.frame_segments(fr.depth_mm, fr.intrinsics, n_planes=0, min_pixels=TC.MIN_PIXELS, concave=TC.CONCAVE)
    plain = SG.frame_segments(fr.depth_mm, fr.intrinsics, n_planes=0, min_pixels=TC.MIN_PIXELS, concave=None)
    want_cut, want_plain = TC.cut_and_plain(fr.depth_mm, fr.intrinsics)
    assert np.array_equal(cut["labels"].cpu().numpy(), want_cut) and np.array_equal(plain["labels"].cpu().numpy(), want_plain)
    pur, held, _ = TC.bounds(want_cut, gt)
    p0, h0, mixed = TC.bounds(want_plain, gt)
    print(f"seed {seed}: with the cut purity {pur:.4f}, held {held:.3f}, {cut['n_segments']} segments; without it purity {p0:.3f}, "
          f"{mixed} mixed of {plain['n_segments']} segments")
    assert pur >= 0.99 and held >= 0.80, (pur, held)
    assert mixed >= 1 and p0 < 0.99                                           # without the cut the table swallows the objects
    assert sum((gt == k).sum() >= 500 for k in range(TC.N_OBJECTS)) >= 2
    # what the CPU pipeline alone said of this seed (how it was chosen)
    q = TC.qualify(seed)
    assert q["ok"] and q["purity"] == pur and q["held"] == held


def test_scene_frame_takes_the_dict_unchanged(dev):
    """scene_frame(segments=) on frame_segments(concave=...)'s dict equals its hand composition (segment_inputs, then scene_poses):
    the extra keys change nothing downstream"""
    from test_gpu_segment_scene import KW, P, _same_out
    cfg = CATEGORIES["bottle"]
    penc, enc = training.load_weights(os.path.join(GOLDEN, "trained_bottle.npz"), cfg, dev)
    fr = TC.sampler(8, dev).sample()
    # A window of the frame with two objects and the table between them.  The whole table spans 1.4 m: a vote grid of more LDS tiles
    # than the exact tiled path serves, and the fall-back's fp32 atomics do not give the same grid twice (include/cppf.h, the vote).
    depth = np.zeros_like(fr.depth_mm)
    depth[95:205, 85:180] = fr.depth_mm[95:205, 85:180]
    seg = SG.frame_segments(depth, fr.intrinsics, n_planes=0, concave=TC.CONCAVE)
    assert seg["n_segments"] >= 3 and int(seg["edge"].sum()) > 100
    out = scene_poses.scene_frame(depth, fr.intrinsics, enc, penc, cfg, n_pairs=P, seed=2, segments=seg, **KW)
    assert _lib.lib().cppf_vote_tiles(*(int(g) for g in out["dims"])) > 0
    hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot), inst = SG.segment_inputs(depth, fr.intrinsics, penc, cfg, P, 2, seg)
    hand = scene_poses.scene_poses(enc, pc, nrm, feat, idx, u_tr, u_rot, cfg, **KW)
    hand.update(hi_pc=hi, hi_normals=hi_nrm, indices=ind, pc=pc, normals=nrm, feat=feat, idx=idx, n_pairs=int(idx.shape[0]), segment_ids=inst)
    _same_out(out, hand)
    assert torch.equal(out["segment_ids"], inst) and int(inst.max()) + 1 <= seg["n_segments"]
    # a dict without the extra keys gives the same frame: nothing downstream reads them
    bare = {k: v for k, v in seg.items() if k not in ("edge", "concave")}
    again = scene_poses.scene_frame(depth, fr.intrinsics, enc, penc, cfg, n_pairs=P, seed=2, segments=bare, **KW)
    _same_out(out, again)
