"""detections.segment_detections on the device: one rendered frame of three floating procedural objects (no background, n_planes = 0),
the committed trained networks.  This pins the PLUMBING, not accuracy: the function equals the composition written by hand --
frame_segments -> labelled_frame_cloud -> hi[hi_labels == s] by torch -> runner.put / run per category -> refined_pose -- bit for
bit; the candidates are the qualifying segments x the categories; select="best" returns at most one detection per segment, the one
select_per_segment picks from `candidates`; max_segments, min_points and max_extent_ratio drop exactly what their rules say; a cloud
without labels raises; frame_detections with its defaults never reaches the new code and returns the same bits."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cppf_amd import detections, scene_poses, scene_stage, training
from cppf_amd import evaluation as E
from cppf_amd import mesh_frames as MF
from cppf_amd import segments as SG
from cppf_amd.batch import BatchPoseRunner
from cppf_amd.config import CATEGORIES
from test_gpu_scene_training import _meshes

pytestmark = pytest.mark.gpu
N_PAIRS = 20_000
SEED = 4
CATS = ("bottle", "mug")
POSE_KEYS = ("T", "R", "up", "right", "scale", "scale_norm", "RT", "n_points", "peak", "argmax")


@pytest.fixture(scope="module")
def setup(dev):
    fr = MF.MeshFrameSampler(_meshes(), 3, device=dev, seed=0, z_range=(0.6, 1.2)).sample()
    seg = SG.frame_segments(fr.depth_mm, fr.intrinsics, n_planes=0)
    nets = {}
    for cat in CATS:
        cfg = CATEGORIES[cat]
        penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
        nets[cat] = (penc, enc, cfg)
    runner = BatchPoseRunner({c: n[1] for c, n in nets.items()}, dev, point_encoders={c: n[0] for c, n in nets.items()})
    return fr, seg, nets, runner


def hand(fr, seg, nets, runner, seed=SEED, n_pairs=N_PAIRS, only=None, min_points=None):
    """the composition by hand -> [(segment, category index, record f64[20], n_points)] and the segments' point counts per category;
    only: the segments that may be candidates (None: all)"""
    S = seg["n_segments"]
    rows, counts = [], {}
    for c, (name, (penc, enc, cfg)) in enumerate(nets.items()):
        cloud = SG.labelled_frame_cloud(fr.depth_mm, fr.intrinsics, cfg, seg)
        parts = [(cloud.hi[cloud.hi_labels == s].contiguous(), cloud.hi_nrm[cloud.hi_labels == s].contiguous()) for s in range(S)]
        counts[name] = [int(p.shape[0]) for p, _ in parts]
        need = int(penc.k) if min_points is None else int(min_points)
        take = [s for s in range(S) if parts[s][0].shape[0] >= need and (only is None or s in only)]
        if not take:
            continue
        recs = runner.run(runner.put([dict(pc=parts[s][0], normals=parts[s][1], cfg=cfg, n_pairs=n_pairs) for s in take]), seed=seed)
        recs = recs.cpu().numpy()
        runner.check()
        rows += [(s, c, recs[j], parts[s][0].shape[0]) for j, s in enumerate(take)]
    return rows, counts


def assert_candidates(cands, rows, nets, n_pairs=N_PAIRS):
    cfgs = [n[2] for n in nets.values()]
    assert [(p["segment"], p["category"]) for p in cands] == [(s, c) for s, c, _, _ in rows]
    for p, (s, c, rec, n) in zip(cands, rows):
        assert rec[12] >= 0
        want = scene_poses.refined_pose(rec, cfgs[c], n)
        for key in POSE_KEYS:
            if want[key] is None:
                assert p[key] is None, key
            else:
                assert np.array_equal(np.asarray(p[key]), np.asarray(want[key])), (s, c, key)      # bit for bit
        assert p["n_surv"] == int(rec[14]) and p["n_pairs"] == n_pairs and p["class_name"] == list(nets)[c]
        assert isinstance(p["agreement"], np.float64) and p["agreement"] == np.float64(int(rec[14])) / np.float64(n_pairs)
        assert 0.0 <= p["agreement"] <= 1.0


@pytest.fixture(scope="module")
def best(setup):
    fr, seg, nets, runner = setup
    return detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED)


def test_the_frame_is_what_the_test_needs(setup):
    fr, seg, nets, runner = setup
    assert len(fr.visible(200)) == 3 and seg["n_segments"] >= 3
    k = {c: int(n[0].k) for c, n in nets.items()}
    rows, counts = hand(fr, seg, nets, runner)
    big = [s for s in range(seg["n_segments"]) if counts["bottle"][s] >= k["bottle"]]
    assert len(big) >= 3, counts                                              # three objects' worth of qualifying segments


def test_equals_the_hand_composition(setup, best):
    fr, seg, nets, runner = setup
    rows, counts = hand(fr, seg, nets, runner)
    assert best["segments"] is seg and not best["refused"] and all(r[2][12] >= 0 for r in rows)
    assert_candidates(best["candidates"], rows, nets)
    # qualifying segments x categories
    S = seg["n_segments"]
    qualifying = sum(counts[name][s] >= int(nets[name][0].k) for name in nets for s in range(S))
    assert len(best["candidates"]) == qualifying >= 2 * 3
    assert sorted(best["skipped"]["min_points"]) == sorted((s, name) for name in nets for s in range(S) if counts[name][s] < int(nets[name][0].k))
    assert best["skipped"]["max_segments"] == [] and best["skipped"]["extent"] == []
    # segments=None computes the same segments from segment_kw
    again = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, n_pairs=N_PAIRS, seed=SEED, segment_kw=dict(n_planes=0))
    assert torch.equal(again["segments"]["labels"], seg["labels"])
    assert_candidates(again["candidates"], rows, nets)


def test_best_keeps_one_detection_per_segment(setup, best):
    fr, seg, nets, runner = setup
    cands = best["candidates"]
    picked = detections.select_per_segment(cands, "best")
    unsup = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, nms_thresh=None)
    assert sorted(d["segment"] for d in unsup["detections"]) == [p["segment"] for p in picked]
    for d in unsup["detections"]:
        p = next(q for q in picked if q["segment"] == d["segment"])
        assert d["category"] == p["category"] and d["score"] == p["agreement"] and np.array_equal(d["RT"], p["RT"])
        assert np.array_equal(d["scales"], p["scale"] / p["scale_norm"]) and d["class_name"] == list(nets)[p["category"]]
    scores = [d["score"] for d in unsup["detections"]]
    assert scores == sorted(scores, reverse=True)
    # with the NMS: one pooled pass over the picked candidates, whatever their categories
    segs = [d["segment"] for d in best["detections"]]
    assert len(set(segs)) == len(segs) <= len(picked)
    use = [p for p in picked if detections._finite(p)]
    (keep,) = E.nms_3d(np.stack([p["RT"] for p in use]), np.stack([p["scale"] for p in use]), [p["agreement"] for p in use], 0.3)
    assert sorted(segs) == sorted(use[i]["segment"] for i in keep)
    for d in best["detections"]:
        assert d["pose"] is cands[d["proposal"]] and d["pose"]["segment"] == d["segment"]
    r = best["result"]
    assert r["pred_RTs"].shape == (len(segs), 4, 4) and r["pred_class_ids"].tolist() == [d["category"] + 1 for d in best["detections"]]
    assert sum(best["kept_per_category"].values()) == len(segs) and sum(best["proposals_per_category"].values()) == len(use)
    assert sum(best["suppressed"].values()) == len(use) - len(segs)


def test_all_keeps_every_candidate_and_peak_ranks_by_the_vote_peak(setup, best):
    fr, seg, nets, runner = setup
    every = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, select="all",
                                          nms_thresh=None)
    assert len(every["detections"]) == len(every["candidates"]) == len(best["candidates"])
    assert sorted((d["segment"], d["category"]) for d in every["detections"]) == sorted((p["segment"], p["category"]) for p in best["candidates"])
    # select="all" with the NMS: pool_detections' rule, a pass per category
    nms = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, select="all")
    want = []
    for c in range(len(nets)):
        use = [p for p in every["candidates"] if p["category"] == c]
        (keep,) = E.nms_3d(np.stack([p["RT"] for p in use]), np.stack([p["scale"] for p in use]), [p["agreement"] for p in use], 0.3)
        want += [(use[i]["segment"], c) for i in keep]
    assert sorted((d["segment"], d["category"]) for d in nms["detections"]) == sorted(want)
    peak = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, score="peak",
                                         nms_thresh=None)
    for p in peak["candidates"]:
        assert p["score"] == p["peak"]
    by_peak = detections.select_per_segment(peak["candidates"], "best")
    assert sorted((d["segment"], d["category"], d["score"]) for d in peak["detections"]) == [(p["segment"], p["category"], p["peak"]) for p in by_peak]
    with pytest.raises(ValueError, match="select"):
        detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, select="first")
    with pytest.raises(ValueError, match="score"):
        detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, score="diff")


def test_max_segments_min_points_and_max_extent_ratio_drop_what_their_rules_say(setup, best):
    fr, seg, nets, runner = setup
    S = seg["n_segments"]
    sizes = seg["sizes"].cpu().numpy()
    # max_segments = 2: the two largest by sizes, ties to the lower label
    order = sorted(range(S), key=lambda s: (-int(sizes[s]), s))
    two = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, max_segments=2)
    assert two["skipped"]["max_segments"] == sorted(order[2:]) and {p["segment"] for p in two["candidates"]} <= set(order[:2])
    rows, counts = hand(fr, seg, nets, runner, only=set(order[:2]))
    assert_candidates(two["candidates"], rows, nets)                          # objects 0, 1 of each batch: other draws than in `best`
    # min_points: one above the second largest cloud leaves the largest segment alone
    _, counts = hand(fr, seg, nets, runner, min_points=10 ** 7)
    bound = max(sorted(counts[name], reverse=True)[1] for name in nets) + 1
    one = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, min_points=bound)
    rows1, _ = hand(fr, seg, nets, runner, min_points=bound)
    assert_candidates(one["candidates"], rows1, nets)
    assert [(p["segment"], p["class_name"]) for p in one["candidates"]] == [(s, name) for name in nets for s in range(S)
                                                                           if counts[name][s] >= bound]
    assert 1 <= len(one["candidates"]) <= len(nets)                           # at most the largest segment of each cloud
    assert len(one["skipped"]["min_points"]) == len(nets) * S - len(one["candidates"])
    none = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, min_points=10 ** 7)
    assert none["candidates"] == [] and none["detections"] == [] and none["result"]["pred_RTs"].shape == (0, 4, 4)
    # max_extent_ratio: the diagonal of hi[hi_labels == s]'s box against r |2 scale_mean|, per (segment, category)
    diag = {}
    for name, (penc, enc, cfg) in nets.items():
        cloud = SG.labelled_frame_cloud(fr.depth_mm, fr.intrinsics, cfg, seg)
        for s in range(S):
            p = cloud.hi[cloud.hi_labels == s].double().cpu().numpy()
            diag[s, name] = float(np.linalg.norm(p.max(0) - p.min(0))) if len(p) else np.inf
    qualifying = [(p["segment"], p["class_name"]) for p in best["candidates"]]
    ratios = sorted(diag[s, n] / np.linalg.norm(2 * np.asarray(nets[n][2].scale_mean, np.float64)) for s, n in qualifying)
    r = 0.5 * (ratios[0] + ratios[1]) if ratios[1] > ratios[0] else ratios[0]  # between the smallest and the next: keeps one pair (or ties)
    ext = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, max_extent_ratio=r)
    keep = [(s, n) for s, n in qualifying if diag[s, n] <= r * np.linalg.norm(2 * np.asarray(nets[n][2].scale_mean, np.float64))]
    assert [(p["segment"], p["class_name"]) for p in ext["candidates"]] == keep and 1 <= len(keep) < len(qualifying)
    assert sorted(ext["skipped"]["extent"]) == sorted(set(qualifying) - set(keep))
    loose = detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, segments=seg, n_pairs=N_PAIRS, seed=SEED, max_extent_ratio=1e6)
    assert_candidates(loose["candidates"], hand(fr, seg, nets, runner)[0], nets)
    assert loose["skipped"]["extent"] == []


def test_refusals(setup, dev):
    fr, seg, nets, runner = setup
    cfg = nets["bottle"][2]
    bare = scene_poses.frame_cloud(fr.depth_mm, fr.intrinsics, cfg)
    assert isinstance(bare, scene_stage.SceneCloud) and bare.hi_labels is None
    with pytest.raises(ValueError, match="labels"):
        SG.segment_clouds(bare, seg["n_segments"])
    with pytest.raises(ValueError, match="at least one"):
        detections.segment_detections(fr.depth_mm, fr.intrinsics, {}, runner, segments=seg)
    with pytest.raises(ValueError, match="point encoder"):
        detections.segment_detections(fr.depth_mm, fr.intrinsics, nets, BatchPoseRunner({c: n[1] for c, n in nets.items()}, dev), segments=seg)


def test_frame_detections_defaults_never_reach_the_new_code(setup, monkeypatch):
    fr, seg, nets, runner = setup
    kw = dict(n_pairs=200_000, seed=3, thresh=5.0, max_proposals=4)
    want = detections.frame_detections(fr.depth_mm, fr.intrinsics, nets, **kw)

    def boom(*a, **k):
        raise AssertionError("a default path reached the segment-instance stage")
    for mod, names in ((SG, ("segment_clouds", "segment_clouds_device", "check_segment_cloud_args")),
                       (detections, ("segment_detections", "select_per_segment"))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
    got = detections.frame_detections(fr.depth_mm, fr.intrinsics, nets, **kw)
    assert list(got) == list(want) == ["detections", "kept_per_category", "suppressed", "proposals_per_category", "result", "cfgs", "outs"]
    assert len(got["detections"]) == len(want["detections"]) > 0
    for a, b in zip(got["detections"], want["detections"]):
        assert set(a) == set(b) == {"class_name", "category", "RT", "scales", "score", "pose", "proposal"}
        assert (a["category"], a["proposal"]) == (b["category"], b["proposal"])
        assert np.array_equal(a["RT"], b["RT"]) and np.array_equal(a["scales"], b["scales"]) and np.array_equal(a["RT"], a["pose"]["RT"])
    assert got["kept_per_category"] == want["kept_per_category"] and got["suppressed"] == want["suppressed"]
    for key in ("pred_class_ids", "pred_RTs", "pred_scales"):
        assert np.array_equal(got["result"][key], want["result"][key]), key
