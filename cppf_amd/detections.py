"""Mask-free frame detections: one depth frame in, ONE list of detections of all categories out.

cppf_amd.scene_poses returns, per category network, every proposal of a scene; each network also votes on every other category's
points, and nothing filters what it proposes.  This module pools the categories' proposals and runs the
reference's scene-level post-processing on them -- the greedy 3D non-maximum suppression of sunrgbd/eval.py:13-35,116-145 per class,
on the device (evaluation.nms_3d -> cppf_box_nms_batch, all categories in one call):

  frame_detections   depth frame -> scene_frame per category (the dense cloud and its normals computed once per distinct
                     (res, knn)) -> pool_detections
  pool_detections    scene_poses / scene_frame dicts, one per category -> detections, per-category NMS, optionally a second,
                     cross-category pass over the survivors
  segment_detections depth frame -> its depth segments taken as instance masks -> the instance path of every category on every
                     segment (one resident batch per category) -> select_per_segment -> NMS.  No scene stage
  select_per_segment the choice among a segment's candidates, a pure host function
"""
from collections import OrderedDict

import numpy as np

from . import evaluation as E


def _finite(p):
    return all(np.all(np.isfinite(np.asarray(p[k], np.float64))) for k in ("T", "R", "scale")) and np.isfinite(p["scale_norm"]) \
        and p["scale_norm"] > 0


def _box(p):
    """RT (rotation * scale_norm, translation), scales (scale / scale_norm) and extents (scale) of a pose dict"""
    RT = np.eye(4)
    RT[:3, :3] = np.asarray(p["R"], np.float64) * float(p["scale_norm"])
    RT[:3, 3] = np.asarray(p["T"], np.float64)
    scale = np.asarray(p["scale"], np.float64)
    return dict(RT=RT, scales=scale / float(p["scale_norm"]), extents=scale)


def _needs_verify(score, min_agreement, min_fill, min_within):
    return score == "agreement" or any(m is not None for m in (min_agreement, min_fill, min_within))


def pool_detections(outs, names, cfgs=None, nms_thresh=0.3, cross_category=False, score="diff", device=None, min_agreement=None,
                    min_fill=None, min_within=None, use_refined=False):
    """outs: scene_poses / scene_frame dicts, one per category, in the order of `names` (the categories' names); cfgs: their configs
    (kept beside the detections for callers; nothing here reads them).
    Every finite proposal with scale_norm > 0 becomes a detection dict:
      class_name, category (index into names), RT f64[4,4] (rotation * scale_norm, translation) and scales f64[3] (scale /
      scale_norm) -- the pair inference.nocs_result writes --, score (p["diff"], the smoothed peak's height above its box edge, which
      scripts/eval_mesh_frames.py ranks by; score="cnt": the smoothed peak itself), pose (the pose dict, its point_mask over THAT
      category's cloud) and proposal (its index in that category's list).
    NMS (evaluation.nms_3d, thresh = nms_thresh, boxes = (RT, extents p["scale"])) runs per category, all categories in one call: the
    reference's rule.  nms_thresh=None: no suppression.  device: where it runs (None: the host path).
    cross_category=True: a second pass over the survivors of all categories pooled as ONE group.  Scores of different networks are
    vote-peak heights of different networks on different clouds; they are NOT calibrated against each other, so which of two
    coincident detections of different categories survives says which network voted harder, not which is right.
    Returns dict(detections=[...] in descending score order (equal scores: the higher pooled index first, NMS' tie rule),
    kept_per_category {name: n}, suppressed {name: n} (both passes), proposals_per_category {name: n}, result=dict(pred_class_ids
    i32[n] = category + 1 (0 is the background of a synset list ["BG"] + names), pred_RTs, pred_scales, pred_scores) as
    evaluation.compute_degree_cm_mAP reads them, cfgs).
    Proposal verification (poses computed with verify=True, else ValueError): score="agreement" ranks by
    pose["verify"]["agreement"], a ratio in [0, 1] that means the same for every network.  min_agreement / min_fill / min_within (None:
    no filter) drop, BEFORE the NMS, every detection whose verify agreement / fill / within is below the bound.  When any of these is
    used the dict gains filtered {name: n}, the detections the filters dropped per category; they count in proposals_per_category and
    not in suppressed.  With all four at their defaults nothing here changes.
    use_refined=True (scene_poses.refine_poses has run on the poses): where pose["refined"] is a finite pose, the detection's RT, scales
    and the box the NMS sees come from it, and the detection gains coarse = dict(RT, scales, scale), the first pass's values.  The score,
    the verify counts and the filters stay the FIRST pass's: nothing is re-scored or re-verified from the refined pose.  A proposal
    without a refined pose (skipped, refused, not finite) stays a detection with its first-pass box."""
    names = list(names)
    if len(outs) != len(names):
        raise ValueError(f"{len(outs)} outputs for {len(names)} category names")
    if score not in ("diff", "cnt", "agreement"):
        raise ValueError(f"score must be 'diff', 'cnt' or 'agreement', got {score!r}")
    verified = _needs_verify(score, min_agreement, min_fill, min_within)
    bounds = [(key, float(m)) for key, m in (("agreement", min_agreement), ("fill", min_fill), ("within", min_within)) if m is not None]
    dets, dropped = [], [0] * len(names)
    for c, out in enumerate(outs):
        for k, p in enumerate(out["poses"]):
            if verified and p is not None and "verify" not in p:
                raise ValueError(f"score='agreement' and the min_agreement / min_fill / min_within filters read pose['verify']: proposal "
                                 f"{k} of {names[c]!r} has none -- compute the poses with verify=True")
            value = None if p is None else (p["verify"]["agreement"] if score == "agreement" else p[score])
            if p is None or not _finite(p) or not np.isfinite(value):
                continue
            if any(p["verify"][key] < m for key, m in bounds):
                dropped[c] += 1
                continue
            det = dict(class_name=names[c], category=c, score=float(value), pose=p, proposal=k, **_box(p))
            r = p.get("refined") if use_refined else None
            if r is not None and _finite(r):
                det.update(coarse=dict(RT=det["RT"], scales=det["scales"], scale=det["extents"]), **_box(r))
            dets.append(det)
    extra = {}
    if verified:
        extra["filtered"] = OrderedDict(zip(names, dropped))
    return _suppress(dets, names, cfgs, nms_thresh, cross_category, device, dropped if verified else None, **extra)


def _suppress(dets, names, cfgs, nms_thresh, cross_category, device, dropped=None, per_category=True, **extra):
    """pool_detections' second half: the NMS over detection dicts (each with RT, extents, score, category) and the dict it returns.
    per_category=False: ONE pass over all detections as one group instead of a pass per category (cross_category then adds nothing)."""
    n = len(dets)
    cat = np.array([d["category"] for d in dets], np.int64).reshape(n)
    scores = np.array([d["score"] for d in dets], np.float64).reshape(n)
    RTs = np.stack([d["RT"] for d in dets]) if n else np.zeros((0, 4, 4))
    extents = np.stack([d.pop("extents") for d in dets]) if n else np.zeros((0, 3))
    keep = np.arange(n)
    if nms_thresh is not None and n:
        keep = np.concatenate(E.nms_3d(RTs, extents, scores, nms_thresh, groups=cat if per_category else None, device=device)
                              + [np.zeros(0, np.int64)])
        if per_category and cross_category and len(keep):
            keep = np.sort(keep)
            (again,) = E.nms_3d(RTs[keep], extents[keep], scores[keep], nms_thresh, device=device)
            keep = keep[again]
    keep = np.sort(keep.astype(np.int64))
    keep = keep[np.argsort(scores[keep], kind="stable")[::-1]]
    kept = [dets[i] for i in keep]
    per_cat = lambda idx: OrderedDict((nm, int((cat[idx] == c).sum())) for c, nm in enumerate(names))
    total, left = per_cat(np.arange(n)), per_cat(keep)
    suppressed = OrderedDict((nm, total[nm] - left[nm]) for nm in names)
    if dropped is not None:
        total = OrderedDict((nm, total[nm] + dropped[c]) for c, nm in enumerate(names))
    result = dict(pred_class_ids=(cat[keep] + 1).astype(np.int32), pred_RTs=RTs[keep].reshape(-1, 4, 4),
                  pred_scales=(np.stack([d["scales"] for d in kept]) if kept else np.zeros((0, 3))), pred_scores=scores[keep])
    return dict(detections=kept, kept_per_category=left, suppressed=suppressed, proposals_per_category=total, result=result, cfgs=cfgs,
                **extra)


def frame_detections(depth, intrinsics, networks, n_pairs=5_000_000, seed=0, jitter=None, nms_thresh=0.3, cross_category=False,
                     score="diff", min_agreement=None, min_fill=None, min_within=None, refine=None, refine_kw=None, segments=None,
                     intra_frac=1.0, **scene_kw):
    """One depth frame with no instance masks -> the detections of all categories (pool_detections' dict, plus outs: the categories'
    scene_frame dicts).
    networks: an ordered mapping name -> (point_encoder, encoder, cfg), modules on one HIP device, in either precision (what the
    encoders are set to is what runs).  scene_frame runs once per category with the same `seed` (and jitter); the frame's SceneCloud
    is computed once per distinct (cfg.res, cfg.knn) and shared (scene_frame's cloud=: the same bits as without sharing).
    The NMS runs on the networks' device.  score="agreement" / min_agreement / min_fill / min_within: pool_detections'; scene_frame
    then runs with verify=True (only then).  scene_kw: scene_poses' options (thresh, max_proposals, ...).
    refine (opt-in, default None: the same launches and the same bits as ever): a BatchPoseRunner that holds every category's two
    encoders, or a dict name -> runner.  Every category's proposals are then refined as instances (scene_frame(refine=...): the
    voxel-owner map is computed once per shared cloud) and pooled with use_refined=True: box, RT and scales from `refined` where it
    exists, the first pass's under `coarse`; score, verification and filters stay the first pass's.  refine_kw: refine_poses' options.
    segments (opt-in, default None: the same launches and the same bits as ever): segments.frame_segments' dict for this frame, handed
    to every category's scene_frame with intra_frac -- each network's pairs are drawn inside the same segments.  The shared cloud
    is then the labelled one (segments.labelled_frame_cloud)."""
    from .scene_poses import frame_cloud, scene_frame
    if not networks:
        raise ValueError("frame_detections needs at least one category network")
    from .segments import labelled_frame_cloud
    names, outs, cfgs, clouds, owners, dev = [], [], [], {}, {}, None
    if _needs_verify(score, min_agreement, min_fill, min_within):
        scene_kw = dict(scene_kw, verify=True)
    for name, (point_encoder, encoder, cfg) in networks.items():
        key = (float(cfg.res), int(cfg.knn))
        if key not in clouds:
            clouds[key] = (frame_cloud(depth, intrinsics, cfg, jitter) if segments is None else
                           labelled_frame_cloud(depth, intrinsics, cfg, segments, jitter))
        extra = {}
        if segments is not None:
            extra = dict(segments=segments, intra_frac=intra_frac)
        if refine is not None:
            extra.update(refine=refine[name] if isinstance(refine, dict) else refine, refine_kw=dict(refine_kw or {}, owner=owners.get(key)))
        out = scene_frame(depth, intrinsics, encoder, point_encoder, cfg, n_pairs=n_pairs, seed=seed, jitter=jitter, cloud=clouds[key],
                          **extra, **scene_kw)
        if refine is not None:
            owners[key] = out["owner"]
        dev = out["pc"].device
        names.append(name); outs.append(out); cfgs.append(cfg)
    res = pool_detections(outs, names, cfgs, nms_thresh, cross_category, score, device=dev, min_agreement=min_agreement,
                          min_fill=min_fill, min_within=min_within, **({} if refine is None else dict(use_refined=True)))
    res["outs"] = outs
    return res


def select_per_segment(cands, rule="best"):
    """The choice among the candidates of segment_detections, on the host: cands is a list of dicts with `segment`, `category` (the
    index of the network) and `score`.  rule="best": per segment the candidate with the highest score, an equal score going to the
    lower category index (then to the earlier candidate); a candidate whose score is NaN is never chosen, and a segment with no
    candidate has no entry.  The chosen candidates come back in ascending segment order.  rule="all": every candidate, in the order
    given.  The dicts themselves are returned, not copies."""
    if rule == "all":
        return list(cands)
    if rule != "best":
        raise ValueError(f"select must be 'best' or 'all', got {rule!r}")
    best = {}
    for c in cands:
        score = float(c["score"])
        if np.isnan(score):
            continue
        have = best.get(c["segment"])
        if have is None or score > float(have["score"]) or (score == float(have["score"]) and c["category"] < have["category"]):
            best[c["segment"]] = c
    return [best[s] for s in sorted(best)]


def segment_detections(depth, intrinsics, networks, runner, segments=None, n_pairs=100_000, seed=0, jitter=None, select="best",
                       score="agreement", nms_thresh=0.3, min_points=None, max_segments=None, max_extent_ratio=None, segment_kw=None):
    """One depth frame -> detections, taking the frame's depth SEGMENTS as the instance masks: no scene vote, no
    proposals, no back-vote -- every segment's dense points go through the instance path of every category network, each (segment,
    category) candidate gets a score that means the same for every network, and per segment the best candidate is kept.
    networks: as for frame_detections; runner: a BatchPoseRunner that holds every category's two encoders (what refine= takes);
    segments: segments.frame_segments' dict for this frame (None: frame_segments(depth, intrinsics, **segment_kw)).
    Per distinct (cfg.res, cfg.knn) one labelled_frame_cloud and one segments.segment_clouds call (cppf_gather_segments: one read-back
    of the offsets, one of the bounds when max_extent_ratio is set).  Per category the segments with at least min_points points
    (default: the point encoder's k) go through runner.put / run as ONE resident batch, n_pairs pairs each, object j of the batch
    drawing its pairs from (seed, j) -- the way scene_poses.refine_poses feeds the runner.
    max_segments: only the largest segments by segments["sizes"] (pixels) are candidates, ties to the lower label.
    max_extent_ratio=r: a (segment, category) pair is skipped when the diagonal of the segment's bounds exceeds r * |2 cfg.scale_mean|.
    A candidate is scene_poses.refined_pose's dict plus segment, n_points, n_surv, n_pairs, agreement = n_surv / n_pairs (fp64; column
    14 of the runner's record over the pairs drawn: a ratio in [0, 1], this project's definition), class_name, category and score
    (score="agreement", or "peak": the vote peak, which is NOT comparable between networks).  A record the runner marks refused
    (record[:, 12] < 0) yields no candidate; the runner's late check of that batch is settled here, as refine_poses does.
    select="best": select_per_segment's choice, then ONE pooled NMS pass over all categories; select="all": every candidate, then
    pool_detections' per-category NMS.  nms_thresh=None: no suppression.
    Returns pool_detections' dict (detections -- each with class_name, category, RT, scales, score, pose (the candidate), proposal
    (its index in candidates) and segment --, result, kept_per_category, proposals_per_category, suppressed, cfgs) plus segments,
    candidates, refused [(segment, class_name)] and skipped = dict(max_segments=[segment], min_points=[(segment, class_name)],
    extent=[(segment, class_name)])."""
    import torch
    from ._lib import CppfError
    from .scene_poses import refined_pose
    from .segments import frame_segments, labelled_frame_cloud, segment_clouds
    if not networks:
        raise ValueError("segment_detections needs at least one category network")
    if select not in ("best", "all"):
        raise ValueError(f"select must be 'best' or 'all', got {select!r}")
    if score not in ("agreement", "peak"):
        raise ValueError(f"score must be 'agreement' or 'peak', got {score!r}")
    for name, (_, _, cfg) in networks.items():
        if cfg.category not in runner.encoders or cfg.category not in runner.point_encoders:
            raise ValueError(f"segment_detections: the runner needs the pair encoder and the point encoder of {cfg.category!r}")
    if segments is None:
        segments = frame_segments(depth, intrinsics, **(segment_kw or {}))
    S = int(segments["n_segments"])
    allowed = np.ones(S, bool)
    skipped = dict(max_segments=[], min_points=[], extent=[])
    if max_segments is not None and S > int(max_segments):
        sizes = np.asarray(segments["sizes"].cpu().numpy() if torch.is_tensor(segments["sizes"]) else segments["sizes"], np.int64)[:S]
        order = np.argsort(-sizes, kind="stable")                             # descending size, ties to the lower label
        allowed[order[max(int(max_segments), 0):]] = False
        skipped["max_segments"] = [int(s) for s in np.nonzero(~allowed)[0]]
    names, cfgs, packed, cands, refused, dev = [], [], {}, [], [], None
    for c, (name, (point_encoder, encoder, cfg)) in enumerate(networks.items()):
        names.append(name); cfgs.append(cfg)
        key = (float(cfg.res), int(cfg.knn))
        if key not in packed:
            g = segment_clouds(labelled_frame_cloud(depth, intrinsics, cfg, segments, jitter), S)
            g["bounds_host"] = g["bounds"].cpu().numpy().astype(np.float64) if max_extent_ratio is not None else None
            packed[key] = g
        g = packed[key]
        dev = g["pts"].device
        need = max(int(runner.point_encoders[cfg.category].k) if min_points is None else int(min_points), 1)
        limit = None if max_extent_ratio is None else float(max_extent_ratio) * float(np.linalg.norm(2.0 * np.asarray(cfg.scale_mean, np.float64)))
        take = []
        for s in np.nonzero(allowed)[0]:
            s = int(s)
            if g["clouds"][s][0].shape[0] < need:
                skipped["min_points"].append((s, name))
            elif limit is not None and not np.linalg.norm(g["bounds_host"][s, 3:] - g["bounds_host"][s, :3]) <= limit:
                skipped["extent"].append((s, name))
            else:
                take.append(s)
        if not take:
            continue
        objs = runner.put([dict(pc=g["clouds"][s][0], normals=g["clouds"][s][1], cfg=cfg, n_pairs=int(n_pairs)) for s in take])
        recs = runner.run(objs, seed=seed)
        batch = runner._batch_no - 1
        recs = recs.cpu().numpy() if torch.is_tensor(recs) else np.asarray(recs)
        try:
            runner.check()
        except CppfError as e:
            if getattr(e, "batch", None) != batch:
                raise
        for j, s in enumerate(take):
            if recs[j, 12] < 0:
                refused.append((s, name))
                continue
            p = refined_pose(recs[j], cfg, g["clouds"][s][0].shape[0])
            n_surv = int(recs[j, 14])
            p.update(segment=s, n_surv=n_surv, n_pairs=int(n_pairs), agreement=np.float64(n_surv) / np.float64(int(n_pairs)),
                     class_name=name, category=c)
            cands.append(p)
    res = pool_segment_candidates(cands, names, cfgs, select, score, nms_thresh, dev)
    res.update(segments=segments, candidates=cands, refused=refused, skipped=skipped)
    return res


def pool_segment_candidates(cands, names, cfgs=None, select="best", score="agreement", nms_thresh=0.3, device=None):
    """segment_detections' last step on its own, host arithmetic plus the NMS: the candidates (each gets score = its `agreement` or its
    `peak`) -> select_per_segment -> detections -> one pooled NMS pass (select="best") or pool_detections' pass per category
    (select="all").  The same candidates may be pooled again under another rule without running a network."""
    if select not in ("best", "all"):
        raise ValueError(f"select must be 'best' or 'all', got {select!r}")
    if score not in ("agreement", "peak"):
        raise ValueError(f"score must be 'agreement' or 'peak', got {score!r}")
    for p in cands:
        p["score"] = float(p[score])
    index = {id(p): k for k, p in enumerate(cands)}
    dets = [dict(class_name=p["class_name"], category=p["category"], score=p["score"], pose=p, proposal=index[id(p)], segment=p["segment"],
                 **_box(p)) for p in select_per_segment(cands, select) if _finite(p) and np.isfinite(p["score"])]
    return _suppress(dets, list(names), cfgs, nms_thresh, False, device, per_category=select == "all")


__all__ = ["pool_detections", "frame_detections", "segment_detections", "select_per_segment", "pool_segment_candidates"]
