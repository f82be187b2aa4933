"""cppf_amd.detections on the device: pooling and the two NMS passes on a perfect-head scene (tests/scene_poses_ref.py), and
frame_detections on a real depth frame with two committed networks against the hand-written loop (scene_frame per category, then
evaluation.nms_3d's host path), with and without the shared cloud."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cppf_amd import detections, scene_poses, training
from cppf_amd import evaluation as E
from cppf_amd.config import CATEGORIES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_poses_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
FRAME_KW = dict(n_pairs=200_000, seed=3, thresh=5.0, max_proposals=4)


def _d(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def perfect(dev):
    sc = S.perfect_scene("mug", 3, 2)
    d = _d(dev)
    out = scene_poses.scene_poses(None, d(sc["pc"]), d(sc["nrm"]), None, d(sc["idx"]), None, None, sc["cfg"], outputs=d(sc["outputs"]),
                                  heads=d(sc["heads"]), max_proposals=6)
    return sc, out


def _near(det, centre, cfg):
    return float(np.abs(det["RT"][:3, 3] - centre).max()) <= 1.5 * cfg.res


def test_pooling_per_category_and_cross_category(perfect, dev):
    sc, out = perfect
    cfg, centres = sc["cfg"], [o["center"] for o in sc["obs"]]
    n_prop = len(out["poses"])
    # the same output under two names, the second with other scores: object k's detection is the higher-scored in category k % 2
    other = dict(out, poses=[dict(p) for p in out["poses"]])
    for p in other["poses"]:
        k = int(np.argmin([np.abs(p["T"] - c).max() for c in centres]))
        p["diff"] = p["diff"] * (1.25 if k % 2 else 0.8)
    for device in (dev, None):
        res = detections.pool_detections([out, other], ["mug", "cup"], [cfg, cfg], nms_thresh=0.3, device=device)
        dets = res["detections"]
        assert res["proposals_per_category"] == {"mug": n_prop, "cup": n_prop}
        assert [d["score"] for d in dets] == sorted((d["score"] for d in dets), reverse=True)
        for c in (0, 1):                                                      # per category, every object is kept
            for ctr in centres:
                assert sum(d["category"] == c and _near(d, ctr, cfg) for d in dets) == 1
        for d in dets:
            p = ([out, other][d["category"]])["poses"][d["proposal"]]
            assert d["pose"] is p and d["class_name"] == ["mug", "cup"][d["category"]] and d["score"] == p["diff"]
            assert np.array_equal(d["RT"][:3, :3], p["R"] * p["scale_norm"]) and np.array_equal(d["scales"], p["scale"] / p["scale_norm"])
        assert all(res["kept_per_category"][nm] + res["suppressed"][nm] == n_prop for nm in ("mug", "cup"))
        r = res["result"]
        assert r["pred_class_ids"].tolist() == [d["category"] + 1 for d in dets] and r["pred_RTs"].shape == (len(dets), 4, 4)
        assert np.array_equal(r["pred_scores"], [d["score"] for d in dets])

        cross = detections.pool_detections([out, other], ["mug", "cup"], [cfg, cfg], nms_thresh=0.3, cross_category=True, device=device)
        for k, ctr in enumerate(centres):                                     # one detection per object: the higher-scored of the pair
            here = [d for d in cross["detections"] if _near(d, ctr, cfg)]
            assert len(here) == 1 and here[0]["category"] == k % 2, (k, [(d["category"], d["score"]) for d in here])
        assert sum(cross["kept_per_category"].values()) <= sum(res["kept_per_category"].values()) - len(centres)
        # the result record feeds the metric
        gt = dict(gt_class_ids=np.array([1] * len(centres)), gt_RTs=np.stack([_gt_rt(o) for o in sc["obs"]]),
                  gt_scales=np.ones((len(centres), 3)), gt_up_syms=np.zeros(len(centres), bool), gt_handle_visibility=np.ones(len(centres)))
        E.compute_degree_cm_mAP([dict(gt, **cross["result"])], ["BG", "mug", "cup"], None)
    # the same output twice: equal scores, the tie rule keeps the later category's
    tie = detections.pool_detections([out, out], ["a", "b"], None, cross_category=True, device=dev)
    assert tie["kept_per_category"]["a"] == 0 and tie["kept_per_category"]["b"] >= len(centres)
    none = detections.pool_detections([out, out], ["a", "b"], None, nms_thresh=None)
    assert len(none["detections"]) == 2 * n_prop and sum(none["suppressed"].values()) == 0


def _gt_rt(ob):
    RT = np.eye(4)
    RT[:3, 3] = ob["center"]
    return RT


@pytest.fixture(scope="module")
def frame(dev):
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))
    nets = {}
    for cat in ("bottle", "mug"):
        cfg = CATEGORIES[cat]
        penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
        nets[cat] = (penc, enc, cfg)
    outs = [scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, **FRAME_KW) for penc, enc, cfg in nets.values()]
    return depth, NOCS_INTRINSICS, nets, outs


def test_frame_detections_equal_the_hand_written_loop(frame, dev):
    depth, K, nets, outs = frame
    got = detections.frame_detections(depth, K, nets, **FRAME_KW)
    # the loop: every finite proposal of every category, nms_3d's host path per category, descending score
    rows = []
    for c, out in enumerate(outs):
        ps = [(k, p) for k, p in enumerate(out["poses"]) if detections._finite(p)]
        if not ps:
            continue
        RT = np.stack([p["RT"] for _, p in ps])
        (pick,) = E.nms_3d(RT, np.stack([p["scale"] for _, p in ps]), [p["diff"] for _, p in ps], 0.3)
        rows += [(ps[i][1]["diff"], c, ps[i][0]) for i in pick]
    pooled = {(c, k): n for n, (c, k) in enumerate((c, k) for c, out in enumerate(outs) for k, p in enumerate(out["poses"])
                                                  if detections._finite(p))}
    rows.sort(key=lambda r: (-r[0], -pooled[(r[1], r[2])]))
    assert sum(len(o["poses"]) for o in outs) > 0
    assert [(d["category"], d["proposal"]) for d in got["detections"]] == [(c, k) for _, c, k in rows]
    for d in got["detections"]:
        p = outs[d["category"]]["poses"][d["proposal"]]
        for key in ("T", "R", "scale", "RT"):
            assert np.array_equal(d["pose"][key], p[key]), key                # bit for bit
        assert d["pose"]["scale_norm"] == p["scale_norm"] and np.array_equal(d["pose"]["point_mask"], p["point_mask"])
        assert np.array_equal(d["RT"], p["RT"])
    assert list(got["kept_per_category"]) == ["bottle", "mug"] and len(got["outs"]) == 2


def test_a_shared_cloud_gives_the_same_bits(frame, dev):
    depth, K, nets, outs = frame
    cfgs = [cfg for _, _, cfg in nets.values()]
    assert (cfgs[0].res, cfgs[0].knn) == (cfgs[1].res, cfgs[1].knn)
    cloud = scene_poses.frame_cloud(depth, K, cfgs[0])
    for (penc, enc, cfg), want in zip(nets.values(), outs):
        got = scene_poses.scene_frame(depth, K, enc, penc, cfg, cloud=cloud, **FRAME_KW)
        assert got["hi_pc"] is cloud[0] and torch.equal(got["pc"], want["pc"]) and torch.equal(got["feat"], want["feat"])
        assert torch.equal(got["outputs"], want["outputs"]) and len(got["poses"]) == len(want["poses"])
        for a, b in zip(got["poses"], want["poses"]):
            for key in ("T", "R", "scale", "RT", "point_mask"):
                assert np.array_equal(a[key], b[key]), key
            # (the scores are heights of the smoothed scene vote, a sum of fp32 atomic adds whose order differs from run to run of
            # the SAME inputs: they agree to rounding, far inside 1e-4, and are not part of the pose)
            assert a["scale_norm"] == b["scale_norm"] and np.isclose(a["cnt"], b["cnt"], rtol=1e-4) and np.isclose(a["diff"], b["diff"], rtol=1e-4)
