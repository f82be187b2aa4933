"""Segments fed into the mask-free paths (cppf_amd/segments.py: segment_inputs; scene_frame / frame_detections segments=): the
labelled cloud and the draw against frame_inputs and the restatement of the scene draw, the hand compositions, rendered frames with a
known answer, and a perfect-head scene whose pairs are all drawn inside the true objects."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_frames_ref as FR  # noqa: E402
import scene_cloud_ref as C  # noqa: E402
import scene_poses_ref as S  # noqa: E402
import scene_training_ref as TR  # noqa: E402
import segments_ref as R  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from cppf_amd import detections, scene_poses, scene_stage, training  # noqa: E402
from cppf_amd import mesh_frames as MF  # noqa: E402
from cppf_amd import segments as SG  # noqa: E402
from cppf_amd.config import CATEGORIES  # noqa: E402
from cppf_amd.frames import draw_pairs  # noqa: E402
from test_gpu_scene_training import _meshes  # noqa: E402

pytestmark = pytest.mark.gpu

# Sampler seeds of the rendered frames (3 objects for an even seed, 4 for an odd one, z_range 0.6..1.2 m, no background, n_planes = 0).
# Chosen on the CPU with tests/mesh_frames_ref.py's render and tests/segments_ref.py: seeds 0..11 were tried, all 12 met both bounds
# (every kept segment >= 99 % under one ground-truth label; every instance of >= 500 pixels >= 90 % inside one segment); the first
# four are used.
FRAME_SEEDS = [0, 1, 2, 3]
P = 100000


def _sampler(seed, dev=None):
    return MF.MeshFrameSampler(_meshes(), 3 + seed % 2, device=dev, seed=seed, z_range=(0.6, 1.2))


def segment_bounds(seg_labels, gt_labels):
    """(the smallest share of a kept segment's pixels under one ground-truth label, the smallest share of an instance of >= 500 pixels
    held by one segment)"""
    pur, own = [], []
    for s in range(int(seg_labels.max()) + 1):
        gt = gt_labels[seg_labels == s]
        pur.append(np.bincount(gt[gt >= 0], minlength=1).max() / gt.size)
    for k in range(int(gt_labels.max()) + 1):
        m = gt_labels == k
        if m.sum() >= 500:
            segs = seg_labels[m]
            segs = segs[segs >= 0]
            own.append(np.bincount(segs).max() / m.sum() if segs.size else 0.0)
    return min(pur), min(own)


@pytest.fixture(scope="module")
def frame(dev):
    fr = _sampler(1, dev).sample()
    return fr, SG.frame_segments(fr.depth_mm, fr.intrinsics, n_planes=0)


@pytest.fixture(scope="module")
def bottle(dev):
    cfg = CATEGORIES["bottle"]
    penc, enc = training.load_weights(os.path.join(GOLDEN, "trained_bottle.npz"), cfg, dev)
    return cfg, penc, enc


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("seed", FRAME_SEEDS)
def test_rendered_frames_segment_into_their_objects(dev, seed):
    s = _sampler(seed, dev)
    fr = s.sample()
    seg = SG.frame_segments(fr.depth_mm, fr.intrinsics, n_planes=0)
    want = R.segments_ref(fr.depth_mm, None, min_pixels=200, capacity=256)
    assert np.array_equal(seg["labels"].cpu().numpy(), want["labels"]) and seg["n_segments"] == want["counts"][0] >= 2
    gt = fr.labels.cpu().numpy()
    pur, own = segment_bounds(want["labels"], gt)
    assert pur >= 0.99 and own >= 0.90, (pur, own)
    # the restatement's render of the same draw meets them too (how the seeds were chosen)
    spec = _sampler(seed).draw()
    depth, labels = FR.raster_instances_ref(s.meshes, spec["inst_mesh"], spec["model_views"])
    pur, own = segment_bounds(R.segments_ref(MF.depth_to_mm(depth), None, min_pixels=200)["labels"], labels)
    assert pur >= 0.99 and own >= 0.90, (pur, own)


def test_segment_inputs_clouds_labels_and_draw(dev, frame, bottle):
    fr, seg = frame
    cfg, penc, _ = bottle
    seed = 5
    got = SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed, seg)
    ref = scene_stage.frame_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed)
    hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot), inst = got
    for name, a, b in zip(("hi", "hi_nrm", "ind", "pc", "nrm", "feat"), got[:6], ref[:6]):
        assert _eq(a, b), name
    # the independent side (segment_inputs and frame_inputs share code): the single public calls composed in tests/scene_cloud_ref.py
    hand = C.hand_scene_cloud(fr.depth_mm, fr.intrinsics, cfg, labels=seg["labels"])
    C.assert_same_cloud((hi, hi_nrm, None, ind, pc, nrm, inst), hand, ("hi", "hi_nrm", "ind", "pc", "nrm", "labels"))
    with torch.no_grad():
        assert _eq(feat, penc(hand[0][None], hand[1][None])[0][hand[3]])
    # labels: the label image at each point's own pixel (the point projects back into it), inst = hi_inst[ind]
    cloud = SG.labelled_frame_cloud(fr.depth_mm, fr.intrinsics, cfg, seg)
    C.assert_same_cloud(cloud, hand)
    K_ = fr.intrinsics
    p = hi.double().cpu().numpy()
    col = np.rint(p[:, 0] / p[:, 2] * K_[0, 0] + K_[0, 2]).astype(np.int64)
    row = np.rint(p[:, 1] / p[:, 2] * K_[1, 1] + K_[1, 2]).astype(np.int64)
    assert np.array_equal(seg["labels"].cpu().numpy()[row, col], cloud[2].cpu().numpy()) and torch.equal(inst, cloud[2][ind])
    inst_h = inst.cpu().numpy()
    N = inst_h.shape[0]
    n_seg = seg["n_segments"]
    sizes = np.bincount(inst_h[inst_h >= 0], minlength=n_seg)
    ok8 = (sizes >= 8).astype(np.int32)                                         # min_points' default
    assert n_seg >= 3 and ok8.sum() >= 3
    # the pair list: the restatement of the scene draw on the same members, behind the same filter; the uniforms: draw_pairs(seed, 0)'s
    _, u_full = draw_pairs(seed, 0, P, dev, N)

    def expect(flags, n_pos):
        members, seg_off = TR.members_ref(inst_h, flags)
        full = TR.draw_ref(members, seg_off, inst_h, N, P, n_pos, seed)
        pos = scene_stage.kept_positions(pc, nrm, torch.from_numpy(full).to(dev)).cpu().numpy()
        return full, pos

    full, pos = expect(ok8, P)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), full[pos])
    assert torch.equal(u_tr, u_full[0][torch.from_numpy(pos).to(dev)]) and torch.equal(u_rot, u_full[1][torch.from_numpy(pos).to(dev)])
    a, b = idx[:, 0].cpu().numpy(), idx[:, 1].cpu().numpy()
    assert 0 < pos.size <= P and np.all(inst_h[a] == inst_h[b]) and np.all(inst_h[a] >= 0)        # EVERY pair inside one segment
    assert set(inst_h[a].tolist()) == set(np.nonzero(ok8)[0].tolist())
    # a segment below min_points never appears
    cut = int(np.sort(sizes[sizes >= 8])[0]) + 1
    assert 1 <= (sizes >= cut).sum() < ok8.sum()
    got2 = SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed, seg, min_points=cut, cloud=cloud)
    full2, pos2 = expect((sizes >= cut).astype(np.int32), P)
    i2 = got2[6].cpu().numpy()
    assert np.array_equal(i2, full2[pos2]) and not np.isin(inst_h[i2], np.nonzero(sizes < cut)[0]).any()
    assert np.all(inst_h[i2[:, 0]] == inst_h[i2[:, 1]])
    # intra_frac = 0: the scene draw's uniform rule -- words x, y of Philox stream 4, NOT draw_pairs' pairs (stream 0)
    got0 = SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed, seg, intra_frac=0.0, cloud=cloud)
    full0, pos0 = expect(ok8, 0)
    assert np.array_equal(got0[6].cpu().numpy(), full0[pos0])
    assert not np.array_equal(full0, draw_pairs(seed, 0, P, dev, N)[0].cpu().numpy())
    assert (inst_h[full0[:, 0]] != inst_h[full0[:, 1]]).mean() > 0.3           # most uniform pairs join two objects
    # no qualifying segment: the kernel's rule at M = 0 is the uniform draw
    none = SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed, seg, min_points=N + 1, cloud=cloud)
    assert torch.equal(none[6], got0[6])
    # half and half
    half = SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed, seg, intra_frac=0.5, cloud=cloud)
    fullh, posh = expect(ok8, P // 2)
    assert np.array_equal(half[6].cpu().numpy(), fullh[posh])
    with pytest.raises(ValueError):
        SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, seed, seg, intra_frac=1.5, cloud=cloud)


POSE_KEYS = ("T", "R", "scale", "RT", "point_mask")
KW = dict(thresh=5.0, max_proposals=4)


def _same_out(a, b):
    assert sorted(a) == sorted(b)
    for k in ("outputs", "heads", "grid", "surv_bits", "pairs", "idx", "pc", "feat", "hi_pc", "indices", "normals", "hi_normals"):
        assert _eq(a[k], b[k]), k
    for x, y in zip(a["proposals"], b["proposals"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["offsets"], b["offsets"]) and a["n_pairs"] == b["n_pairs"] and len(a["poses"]) == len(b["poses"])
    for p, q in zip(a["poses"], b["poses"]):
        for k in POSE_KEYS:
            assert np.array_equal(p[k], q[k]), k
        assert p["n_pairs"] == q["n_pairs"] and p["cnt"] == q["cnt"]
        if "verify" in p or "verify" in q:
            assert p["verify"] == q["verify"]


def test_scene_frame_equals_the_hand_composition(dev, frame, bottle):
    fr, seg = frame
    cfg, penc, enc = bottle
    out = scene_poses.scene_frame(fr.depth_mm, fr.intrinsics, enc, penc, cfg, n_pairs=P, seed=2, segments=seg, **KW)
    hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot), inst = SG.segment_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, 2, seg)
    hand = scene_poses.scene_poses(enc, pc, nrm, feat, idx, u_tr, u_rot, cfg, **KW)
    hand.update(hi_pc=hi, hi_normals=hi_nrm, indices=ind, pc=pc, normals=nrm, feat=feat, idx=idx, n_pairs=int(idx.shape[0]), segment_ids=inst)
    _same_out(out, hand)
    assert torch.equal(out["segment_ids"], inst) and len(out["poses"]) >= 1
    # verify= works unchanged on top
    ver = scene_poses.scene_frame(fr.depth_mm, fr.intrinsics, enc, penc, cfg, n_pairs=P, seed=2, segments=seg, verify=True, **KW)
    assert all("verify" in p for p in ver["poses"]) and len(ver["poses"]) == len(out["poses"])
    # segments=None: the parent commit's code path -- frame_inputs, then scene_poses; the same keys and arrays
    plain = scene_poses.scene_frame(fr.depth_mm, fr.intrinsics, enc, penc, cfg, n_pairs=P, seed=2, **KW)
    hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot) = scene_stage.frame_inputs(fr.depth_mm, fr.intrinsics, penc, cfg, P, 2)
    hand = scene_poses.scene_poses(enc, pc, nrm, feat, idx, u_tr, u_rot, cfg, **KW)
    hand.update(hi_pc=hi, hi_normals=hi_nrm, indices=ind, pc=pc, normals=nrm, feat=feat, idx=idx, n_pairs=int(idx.shape[0]))
    _same_out(plain, hand)
    assert "segment_ids" not in plain and sorted(plain) == sorted(
        ["poses", "outputs", "heads", "grid", "proposals", "surv_bits", "offsets", "pairs", "corner", "dims", "hi_pc", "hi_normals", "indices",
         "pc", "normals", "feat", "idx", "n_pairs"])


def test_frame_detections_equals_the_per_category_loop(dev, frame, bottle):
    fr, seg = frame
    cfg, penc, enc = bottle
    mug = CATEGORIES["mug"]
    penc_m, enc_m = training.load_weights(os.path.join(GOLDEN, "trained_mug.npz"), mug, dev)
    nets = {"bottle": (penc, enc, cfg), "mug": (penc_m, enc_m, mug)}
    res = detections.frame_detections(fr.depth_mm, fr.intrinsics, nets, n_pairs=P, seed=4, segments=seg, intra_frac=0.75, **KW)
    outs = [scene_poses.scene_frame(fr.depth_mm, fr.intrinsics, e, pe, c, n_pairs=P, seed=4, segments=seg, intra_frac=0.75, **KW)
            for pe, e, c in nets.values()]
    want = detections.pool_detections(outs, list(nets), [c for _, _, c in nets.values()], device=dev)
    for a, b in zip(res["outs"], outs):
        _same_out(a, b)
    for k in ("pred_class_ids", "pred_RTs", "pred_scales", "pred_scores"):
        assert np.array_equal(res["result"][k], want["result"][k]), k
    assert res["kept_per_category"] == want["kept_per_category"] and len(res["detections"]) == len(want["detections"])
    # segments=None: what it returned before -- the per-category loop without segments
    plain = detections.frame_detections(fr.depth_mm, fr.intrinsics, nets, n_pairs=P, seed=4, **KW)
    outs0 = [scene_poses.scene_frame(fr.depth_mm, fr.intrinsics, e, pe, c, n_pairs=P, seed=4, **KW) for pe, e, c in nets.values()]
    want0 = detections.pool_detections(outs0, list(nets), [c for _, _, c in nets.values()], device=dev)
    for a, b in zip(plain["outs"], outs0):
        _same_out(a, b)
        assert "segment_ids" not in a
    for k in ("pred_class_ids", "pred_RTs", "pred_scales", "pred_scores"):
        assert np.array_equal(plain["result"][k], want0["result"][k]), k
    assert sorted(plain) == sorted(list(want0) + ["outs"])


# ------------------------------------------------------------------------------------------------------------------- perfect heads
def test_perfect_heads_with_pairs_inside_the_true_objects(dev):
    from cppf_amd.scene_training import sample_scene_pairs
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    on_dev = lambda m, o, i, n, p, s: sample_scene_pairs(d(m), d(o), d(i), p, p, s).cpu().numpy()
    sc, idx, outputs, heads = R.perfect_segment_scene(on_dev)
    assert np.array_equal(idx, R.perfect_segment_scene()[1])                  # the device's draw is the restatement's
    cfg, n_obj = sc["cfg"], R.PERFECT[1]
    out = scene_poses.scene_poses(None, d(sc["pc"]), d(sc["nrm"]), None, d(idx), None, None, cfg, outputs=d(outputs), heads=d(heads),
                                  max_proposals=2 * n_obj)
    m = S.match_objects(out["proposals"][0], out["corner"], cfg.res, [o["center"] for o in sc["obs"]])
    assert None not in m and len(set(m)) == n_obj, m
    for j, k in enumerate(m):                                                 # and each proposal's mask is its object
        truth = sc["owner"] == j
        pm = out["poses"][k]["point_mask"]
        assert (pm & truth).sum() / (pm | truth).sum() > 0.9
