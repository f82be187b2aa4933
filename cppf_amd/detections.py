"""Mask-free frame detections: one depth frame in, ONE list of detections of all categories out.

cppf_amd.scene_poses returns, per category network, every proposal of a scene; each network also votes on every other category's
points, and nothing filters what it proposes.  This module pools the categories' proposals and runs the
reference's scene-level post-processing on them -- the greedy 3D non-maximum suppression of sunrgbd/eval.py:13-35,116-145 per class,
on the device (evaluation.nms_3d -> cppf_box_nms_batch, all categories in one call):

  frame_detections   depth frame -> scene_frame per category (the dense cloud and its normals computed once per distinct
                     (res, knn)) -> pool_detections
  pool_detections    scene_poses / scene_frame dicts, one per category -> detections, per-category NMS, optionally a second,
                     cross-category pass over the survivors
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
    n = len(dets)
    cat = np.array([d["category"] for d in dets], np.int64).reshape(n)
    scores = np.array([d["score"] for d in dets], np.float64).reshape(n)
    RTs = np.stack([d["RT"] for d in dets]) if n else np.zeros((0, 4, 4))
    extents = np.stack([d.pop("extents") for d in dets]) if n else np.zeros((0, 3))
    keep = np.arange(n)
    if nms_thresh is not None and n:
        keep = np.concatenate(E.nms_3d(RTs, extents, scores, nms_thresh, groups=cat, device=device) + [np.zeros(0, np.int64)])
        if cross_category and len(keep):
            keep = np.sort(keep)
            (again,) = E.nms_3d(RTs[keep], extents[keep], scores[keep], nms_thresh, device=device)
            keep = keep[again]
    keep = np.sort(keep.astype(np.int64))
    keep = keep[np.argsort(scores[keep], kind="stable")[::-1]]
    kept = [dets[i] for i in keep]
    per_cat = lambda idx: OrderedDict((nm, int((cat[idx] == c).sum())) for c, nm in enumerate(names))
    total, left = per_cat(np.arange(n)), per_cat(keep)
    suppressed = OrderedDict((nm, total[nm] - left[nm]) for nm in names)
    extra = {}
    if verified:
        extra["filtered"] = OrderedDict(zip(names, dropped))
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


__all__ = ["pool_detections", "frame_detections"]
