#!/usr/bin/env python3
"""End-to-end accuracy on occluded input with a known answer: frames of several posed meshes (cppf_amd.mesh_frames.MeshFrameSampler:
one cppf_raster_instances render per frame, instance labels, ground truth) -> FrameRunner -> 3D-IoU AP and degree / cm AP by the
device evaluation path (evaluation.compute_degree_cm_mAP(device=...)).  Prints the two tables and the milliseconds per frame and
writes the record to profiles/mesh_frames_eval.json (--out).  No accuracy threshold is applied anywhere: the figure is reported.

Meshes: --meshes CATEGORY=DIR|NAMES (repeatable; what scripts/train_meshes.py takes), or --procedural for the procedural
bottles / cans / cameras built from tests/mesh_ref.py.  Networks: --weights CATEGORY=FILE (training.save_weights's format), or
--train-steps N to train each category on its meshes first (training.train_on_meshes).

    python scripts/eval_mesh_frames.py --procedural --train-steps 3000 --train-pairs 200000 --frames 60 --objects 4
    python scripts/eval_mesh_frames.py --meshes bottle=ShapeNetCore.v2/02876657 --weights bottle=bottle.npz --frames 200

--mask-free (opt-in; the default run above is unchanged): no instance masks.  Per frame and per category, scene_poses.scene_frame runs
that category's networks on the WHOLE depth image and every proposal becomes a prediction with the category's class id, scored by its
smoothed peak's height above its box edges.  The APs go to profiles/scene_poses_eval.json (--out) as a first figure, with no
threshold attached.

    python scripts/eval_mesh_frames.py --procedural --train-steps 3000 --train-pairs 200000 --frames 20 --objects 4 --mask-free

--mask-free --nms T [--cross-category]: the frames go through cppf_amd.detections.frame_detections instead -- the same proposals, then
the reference's scene-level post-processing (sunrgbd/eval.py: greedy 3D box NMS per class at IoU threshold T, on the device), and with
--cross-category a second pass over the survivors of all categories.  The cut to the 20 best-scored predictions happens after the
suppression.  The record (profiles/scene_detections_eval.json) holds the APs without NMS, with it per category and cross-category from
the same frames and seeds, and the proposals kept / suppressed per category.  Again a first figure, no threshold.

    python scripts/eval_mesh_frames.py --procedural --train-steps 3000 --train-pairs 200000 --frames 20 --objects 4 --mask-free --nms 0.3 --cross-category

--mask-free --score agreement [--min-agreement A] [--min-fill F] [--tune-frames N] [--cross-category]: proposal verification (DESIGN.md
3.7g).  The frames go through scene_frame(verify=True) once; the same proposals are then pooled three ways (NMS per category at --nms,
default 0.3): ranked by `diff` (today's baseline), ranked by `agreement`, and ranked by `agreement` behind the min_agreement / min_fill
filters.  Without --min-agreement the bound is CHOSEN on --tune-frames frames of a separate sampler (seed + 1000, pair seeds apart
from the reported frames'): the candidate with the best mean IoU25 AP there.  The record (profiles/scene_verify_eval.json) also holds,
for the un-suppressed proposals of the reported frames, how each of agreement / leak / fill / purity / diff correlates with the proposal
being a true positive (IoU >= 0.25 with a ground truth of its class).  Figures, no threshold.

    python scripts/eval_mesh_frames.py --procedural --train-steps 3000 --train-pairs 200000 --frames 20 --objects 4 --mask-free --score agreement --tune-frames 20

--mask-free --refine: every proposal once more as an instance (scene_frame(refine=BatchPoseRunner): the proposal's point mask gathers
its dense points on the device, scene_poses.refine_poses).  The same frames and the same networks in ONE run give two AP tables, the
first pass's poses and the refined ones (a proposal without a refined pose keeps its first-pass pose; the scores are the first
pass's in both), written to profiles/refine_eval.json (--out) under `mesh_frames`.  Figures, no threshold.

    python scripts/eval_mesh_frames.py --procedural --train-steps 3000 --train-pairs 200000 --frames 20 --objects 4 --mask-free --refine

--mask-free --segments [--seg-planes N] [--seg-min-pixels M] [--seg-tol-mm T] [--seg-slope S] [--intra-frac F]: depth segments (DESIGN.md
3.7j).  Every frame is segmented on the device first (cppf_amd.segments.frame_segments; --seg-planes 0, the default, suits rendered
frames, which have no background) and each category's pairs are drawn inside the segments (scene_frame(segments=...)); the time per
frame includes the segmentation.  Works with the plain --mask-free run and with --nms; the record gains `segments`, the options and
the mean number of segments per frame, and goes to profiles/segments_eval.json unless --out says otherwise.  Figures, no threshold.

    python scripts/eval_mesh_frames.py --procedural --weights bottle=... --weights can=... --weights camera=... --frames 20 --objects 4 --mask-free --segments

--tabletop [--min-gap G] (any mode but --score agreement): the frames come from mesh_frames.TabletopFrameSampler -- the objects stand
upright on one support plane and may touch (G = 0) -- instead of floating in empty space; the record gains `tabletop`.  Next to
--segments: --planes N (= --seg-planes) removes up to N RANSAC planes first, --concave cuts the frame at its concave creases
(segments.frame_segments(concave={})); both may be given.

    python scripts/eval_mesh_frames.py --procedural --weights ... --frames 20 --objects 4 --tabletop --mask-free --segments --planes 1 --concave

--segment-instances [--planes N] [--concave] [--select best|all] [--score agreement|peak] [--max-extent-ratio R] (a mode of its own, with or
without --tabletop): the frame's depth segments are taken as the instance masks -- detections.segment_detections: every
segment through the instance path of every category, the best candidate per segment by a score that means the same for every network.
The timed run uses --select / --score; the same candidates are then pooled under the other three combinations on the host, and the
record (profiles/segment_instances_eval.json) holds the four AP tables, the candidates and refusals per frame and how often the best
candidate of an object's own segment has the object's category.  Figures, no threshold.

    python scripts/eval_mesh_frames.py --procedural --weights ... --frames 20 --objects 4 --tabletop --segment-instances --planes 1
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf_amd import evaluation as E                   # noqa: E402
from cppf_amd import mesh_frames as MF                 # noqa: E402
from cppf_amd import meshes as M                       # noqa: E402
from cppf_amd import training                          # noqa: E402
from cppf_amd.config import CATEGORIES                 # noqa: E402
from cppf_amd.frames import FrameRunner                # noqa: E402


def _procedural(tmp):
    """OBJ files of procedural stand-ins, scaled to a unit bounding-box diagonal like ShapeNet's model_normalized.obj"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_ref as R
    shapes = {"bottle": [R.necked_cylinder(0.15, 0.40 + 0.03 * k, neck=0.35 + 0.05 * k, n_lon=48) for k in range(4)],
              "can": [R.necked_cylinder(0.2, 0.28 + 0.03 * k, neck=0.95, n_lon=48) for k in range(4)],
              "camera": [R.box(0.30 + 0.02 * k, 0.2, 0.12 + 0.02 * k)[:2] for k in range(4)]}
    out = {}
    for cat, ms in shapes.items():
        out[cat] = []
        for k, (v, f) in enumerate(ms):
            p = os.path.join(tmp, f"{cat}{k}.obj")
            open(p, "w").write(R.to_obj(v / np.linalg.norm(v.max(0) - v.min(0)), f))
            out[cat].append(p)
    return out


def _pairs(items, what):
    out = {}
    for it in items or []:
        if "=" not in it:
            sys.exit(f"--{what} takes CATEGORY=PATH, got {it!r}")
        cat, path = it.split("=", 1)
        out[cat] = path
    return out


def _tables(iou_aps, pose_aps, names, cats, deg, sh, rec):
    """print the two AP tables (per category and the mean over the categories that were drawn) and put them into `rec`"""
    ids = [names.index(c) for c in cats]
    rows = cats + ["mean"]
    print(f"{'3D IoU AP':12s}" + "".join(f"{'IoU' + str(t):>9s}" for t in (25, 50, 75)))
    for c in rows:
        r = iou_aps[names.index(c)] if c != "mean" else iou_aps[ids].mean(0)
        rec["iou_ap"][c] = {f"iou{t}": float(r[t]) for t in (25, 50, 75)}
        print(f"{c:12s}" + "".join(f"{100 * r[t]:9.1f}" for t in (25, 50, 75)))
    combos = [(0, 0), (1, 0), (1, 1), (2, 2)]
    print(f"{'pose AP':12s}" + "".join(f"{str(deg[d]) + 'deg' + str(sh[s]) + 'cm':>11s}" for d, s in combos))
    for c in rows:
        r = pose_aps[names.index(c)] if c != "mean" else pose_aps[ids].mean(0)
        rec["pose_ap"][c] = {f"{deg[d]}deg_{sh[s]}cm": float(r[d, s]) for d, s in combos}
        print(f"{c:12s}" + "".join(f"{100 * r[d, s]:11.1f}" for d, s in combos))


def _mask_free_record(fr, preds):
    """MeshFrame.record's dict with the proposals as predictions.  preds: [(class id, pose dict, score)]"""
    K, n = len(fr.categories), len(preds)
    RTs = np.tile(np.eye(4), (n, 1, 1))
    scales = np.ones((n, 3))
    for i, (_, p, _) in enumerate(preds):
        RTs[i, :3, :3] = np.asarray(p["R"], np.float64) * float(p["scale_norm"])
        RTs[i, :3, 3] = np.asarray(p["T"], np.float64)
        scales[i] = np.asarray(p["scale"], np.float64) / float(p["scale_norm"])
    rec = fr.record([None] * len(fr.visible(1)), min_pixels=1)             # the ground-truth half, no predictions
    rec.update(pred_class_ids=np.array([c for c, _, _ in preds], np.int32).reshape(n), pred_RTs=RTs, pred_scales=scales,
               pred_scores=np.array([s for _, _, s in preds], np.float64).reshape(n))
    assert rec["gt_class_ids"].shape[0] == K
    return rec


def _segments(args, fr, log):
    """--segments: scene_frame's keywords for one frame -- frame_segments with the flags' options -- or {} without the flag; log: the
    segment counts so far"""
    if not args.segments:
        return {}
    from cppf_amd.segments import frame_segments
    seg = frame_segments(fr.depth_mm, fr.intrinsics, n_planes=args.seg_planes, min_pixels=args.seg_min_pixels, tol_mm=args.seg_tol_mm,
                         slope_permille=args.seg_slope, concave={} if args.concave else None)
    log.append(seg["n_segments"])
    return dict(segments=seg, intra_frac=args.intra_frac)


def _segments_record(args, log):
    if not args.segments:
        return None
    rec = dict(n_planes=args.seg_planes, min_pixels=args.seg_min_pixels, tol_mm=args.seg_tol_mm, slope_permille=args.seg_slope,
               intra_frac=args.intra_frac, segments_per_frame_mean=float(np.mean(log)) if log else 0.0)
    if args.concave:                                                          # (without the flag: the record it always was)
        from cppf_amd.segments import concave_options
        rec["concave"] = concave_options()
    return rec


def _mask_free(args, sampler, encs, pencs, dev):
    """the frames through scene_frame per category -> (result records, ms per frame, proposals, ground truths); with --refine also the
    records with the refined poses in place of the first pass's and how many proposals have one (else None, 0)"""
    from cppf_amd.scene_poses import scene_frame
    names = sampler.synset_names
    ok = lambda p: all(np.all(np.isfinite(p[k])) for k in ("T", "R", "scale")) and p["scale_norm"] > 0
    runner = None
    if args.refine:
        from cppf_amd.batch import BatchPoseRunner
        runner = BatchPoseRunner(encs, dev, point_encoders=pencs)
    results, refined, ms, n_prop, n_gt, n_ref = [], [], [], 0, 0, 0
    for i in range(args.frames):
        fr = sampler.sample()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preds = []
        seg_kw = _segments(args, fr, args.seg_log)
        for c in sampler.categories:
            out = scene_frame(fr.depth_mm, fr.intrinsics, encs[c], pencs[c], CATEGORIES[c], n_pairs=args.scene_pairs, seed=i,
                              thresh=args.thresh, max_proposals=args.max_proposals, **({} if runner is None else dict(refine=runner)), **seg_kw)
            for p in out["poses"]:
                if ok(p):
                    preds.append((names.index(c), p, p["diff"]))
        ms.append((time.perf_counter() - t0) * 1e3)
        preds = sorted(preds, key=lambda t: -t[2])[:20]                  # (the evaluation's match tables hold 20 predictions per image)
        results.append(_mask_free_record(fr, preds))
        if runner is not None:
            use = lambda p: p["refined"] if p.get("refined") is not None and ok(p["refined"]) else p
            refined.append(_mask_free_record(fr, [(c, use(p), s_) for c, p, s_ in preds]))
            n_ref += sum(use(p) is not p for _, p, _ in preds)
        n_prop += len(preds)
        n_gt += len(fr.categories)
    return results, ms, n_prop, n_gt, (refined if runner is not None else None), n_ref


def _detections(args, sampler, encs, pencs, dev):
    """--mask-free with --nms / --cross-category: every frame once through detections.frame_detections (no suppression: the
    categories' proposals), then pooled three ways from those same proposals -- unfiltered (the run without --nms), NMS per category,
    and, with --cross-category, the second pass over the survivors.  The cut to the 20 best-scored predictions of a frame (the
    evaluation's match tables hold 20) happens after the suppression.  -> ({variant: records}, ms per frame (the proposals and the
    per-category NMS), {variant: {category: [kept, suppressed]}}, proposals, ground truths)"""
    from collections import OrderedDict
    from cppf_amd.detections import frame_detections, pool_detections
    names = sampler.synset_names
    cats = list(sampler.categories)
    variants = ["no_nms", "nms_per_category"] + (["nms_cross_category"] if args.cross_category else [])
    results = {v: [] for v in variants}
    counts = {v: {c: [0, 0] for c in cats} for v in variants}
    ms, n_prop, n_gt = [], 0, 0
    for i in range(args.frames):
        fr = sampler.sample()
        nets = OrderedDict((c, (pencs[c], encs[c], CATEGORIES[c])) for c in cats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = frame_detections(fr.depth_mm, fr.intrinsics, nets, n_pairs=args.scene_pairs, seed=i, nms_thresh=args.nms,
                               thresh=args.thresh, max_proposals=args.max_proposals, **_segments(args, fr, args.seg_log))
        ms.append((time.perf_counter() - t0) * 1e3)
        pooled = dict(no_nms=pool_detections(res["outs"], cats, None, nms_thresh=None), nms_per_category=res)
        if args.cross_category:
            pooled["nms_cross_category"] = pool_detections(res["outs"], cats, None, nms_thresh=args.nms, cross_category=True, device=dev)
        for v in variants:
            dets = pooled[v]["detections"][:20]
            results[v].append(_mask_free_record(fr, [(names.index(d["class_name"]), d["pose"], d["score"]) for d in dets]))
            for c in cats:
                counts[v][c][0] += pooled[v]["kept_per_category"][c]
                counts[v][c][1] += pooled[v]["suppressed"][c]
        n_prop += len(pooled["no_nms"]["detections"])
        n_gt += len(fr.categories)
    return results, ms, counts, n_prop, n_gt


SEGMENT_VARIANTS = [("best", "agreement"), ("all", "agreement"), ("best", "peak"), ("all", "peak")]


def _segment_instances(args, sampler, encs, pencs, dev):
    """--segment-instances: every frame through detections.segment_detections (timed: the segmentation, the labelled cloud, the gather,
    every category's batch, the selection and the NMS under --select / --score); the frame's candidates are then pooled again, untimed
    and on the host, under the other three of SEGMENT_VARIANTS.  Per ground-truth object with a segment of its own (the segment that
    holds most of its pixels, at least half of them) it is counted whether select_per_segment's best candidate of that segment, under
    each score, has the object's category.  -> ({variant: records}, ms per frame, counters)"""
    from collections import OrderedDict
    from cppf_amd.batch import BatchPoseRunner
    from cppf_amd.detections import pool_segment_candidates, segment_detections, select_per_segment
    names, cats = sampler.synset_names, list(sampler.categories)
    nets = OrderedDict((c, (pencs[c], encs[c], CATEGORIES[c])) for c in cats)
    runner = BatchPoseRunner(encs, dev, point_encoders=pencs)
    primary = (args.select, "peak" if args.score == "peak" else "agreement")
    results = {f"{s}/{k}": [] for s, k in SEGMENT_VARIANTS}
    ms, count = [], dict(ground_truths=0, segments=0, candidates=0, refused=0, skipped_min_points=0, skipped_extent=0, detections=0,
                         objects_with_a_segment=0, best_true_category={"agreement": 0, "peak": 0})
    for i in range(args.frames):
        fr = sampler.sample()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = segment_detections(fr.depth_mm, fr.intrinsics, nets, runner, n_pairs=args.n_pairs, seed=i, select=primary[0], score=primary[1],
                                 nms_thresh=args.nms if args.nms is not None else 0.3, max_extent_ratio=args.max_extent_ratio,
                                 segment_kw=dict(n_planes=args.seg_planes, min_pixels=args.seg_min_pixels, tol_mm=args.seg_tol_mm,
                                                 slope_permille=args.seg_slope, concave={} if args.concave else None))
        ms.append((time.perf_counter() - t0) * 1e3)
        cands, seg = res["candidates"], res["segments"]
        args.seg_log.append(seg["n_segments"])
        for s, k in SEGMENT_VARIANTS:
            pooled = res if (s, k) == primary else pool_segment_candidates(cands, cats, None, s, k, args.nms if args.nms is not None else 0.3, dev)
            dets = pooled["detections"][:20]                                 # (the evaluation's match tables hold 20 predictions per image)
            results[f"{s}/{k}"].append(_mask_free_record(fr, [(names.index(d["class_name"]), d["pose"], d["score"]) for d in dets]))
        count["ground_truths"] += len(fr.categories)
        count["segments"] += seg["n_segments"]
        count["candidates"] += len(cands)
        count["refused"] += len(res["refused"])
        count["skipped_min_points"] += len(res["skipped"]["min_points"])
        count["skipped_extent"] += len(res["skipped"]["extent"])
        count["detections"] += len(res["detections"])
        # the true category of a segment: the object that owns it
        seg_lab, gt_lab = seg["labels"].cpu().numpy(), fr.labels.cpu().numpy()
        owners = {}
        for k_obj, cat in enumerate(fr.categories):
            m = gt_lab == k_obj
            inside = seg_lab[m]
            inside = inside[inside >= 0]
            if inside.size and np.bincount(inside).max() * 2 >= m.sum():
                owners[int(np.bincount(inside).argmax())] = cat
        count["objects_with_a_segment"] += len(owners)
        for k in ("agreement", "peak"):
            for p in cands:
                p["score"] = float(p[k])
            count["best_true_category"][k] += sum(owners.get(p["segment"]) == p["class_name"] for p in select_per_segment(cands, "best"))
    return results, ms, count


def _verified_frames(args, sampler, encs, pencs, n_frames, seed0):
    """n_frames frames of `sampler` through scene_frame(verify=True) per category (pair seed seed0 + i) -> ([(frame, [dict(poses)])],
    ms per frame).  Only the pose lists are kept: pool_detections reads nothing else."""
    from cppf_amd.scene_poses import frame_cloud, scene_frame
    frames, ms = [], []
    for i in range(n_frames):
        fr = sampler.sample()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs, clouds = [], {}
        for c in sampler.categories:
            cfg = CATEGORIES[c]
            key = (float(cfg.res), int(cfg.knn))
            if key not in clouds:
                clouds[key] = frame_cloud(fr.depth_mm, fr.intrinsics, cfg)
            out = scene_frame(fr.depth_mm, fr.intrinsics, encs[c], pencs[c], cfg, n_pairs=args.scene_pairs, seed=seed0 + i, cloud=clouds[key],
                              thresh=args.thresh, max_proposals=args.max_proposals, verify=True)
            outs.append(dict(poses=out["poses"]))
        ms.append((time.perf_counter() - t0) * 1e3)
        frames.append((fr, outs))
    return frames, ms


def _pooled_ap(frames, sampler, cats, dev, **pool_kw):
    """the frames' proposals pooled with pool_kw -> (iou_aps, pose_aps, detections evaluated, kept per category, filtered per category)"""
    from cppf_amd.detections import pool_detections
    names = sampler.synset_names
    recs, n_det = [], 0
    kept, filtered = {c: 0 for c in cats}, {c: 0 for c in cats}
    for fr, outs in frames:
        res = pool_detections(outs, cats, None, device=dev, **pool_kw)
        dets = res["detections"][:20]                                   # (the evaluation's match tables hold 20 predictions per image)
        recs.append(_mask_free_record(fr, [(names.index(d["class_name"]), d["pose"], d["score"]) for d in dets]))
        n_det += len(dets)
        for c in cats:
            kept[c] += res["kept_per_category"][c]
            filtered[c] += res.get("filtered", {}).get(c, 0)
    deg, sh = [5, 10, 15], [5, 10, 15]
    iou = [float(t) for t in np.round(np.linspace(0, 1, 101), 2)]
    iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP(recs, names, None, deg, sh, iou, 0.1, True, device=dev)
    return iou_aps, pose_aps, n_det, kept, filtered


def _true_positive_table(frames, sampler, cats):
    """every finite proposal of the frames (no NMS, no filter) with its verify ratios, its diff and whether it is a true positive: IoU
    >= 0.25 (compute_3d_iou, the up-symmetry sweep included) with a ground truth of its class.  -> dict(n, true_positives, per
    quantity: Pearson r with the true-positive flag, mean over the true and over the false positives)"""
    from cppf_amd.detections import pool_detections
    names = sampler.synset_names
    rows = []
    for fr, outs in frames:
        gt = fr.record([None] * len(fr.visible(1)), min_pixels=1)
        for d in pool_detections(outs, cats, None, nms_thresh=None)["detections"]:
            cid = names.index(d["class_name"])
            best = 0.0
            for j in np.nonzero(gt["gt_class_ids"] == cid)[0]:
                best = max(best, E.compute_3d_iou(d["RT"], gt["gt_RTs"][j], d["scales"], gt["gt_scales"][j], bool(gt["gt_up_syms"][j]),
                                                  d["class_name"], d["class_name"]))
            v = d["pose"]["verify"]
            rows.append([float(best >= 0.25), v["agreement"], v["leak"], v["fill"], v["purity"], float(d["pose"]["diff"])])
    t = np.array(rows, np.float64).reshape(-1, 6)
    out = dict(n=int(t.shape[0]), true_positives=int(t[:, 0].sum()) if t.size else 0, quantities={})
    for k, q in enumerate(("agreement", "leak", "fill", "purity", "diff"), 1):
        tp, fp = t[t[:, 0] == 1, k], t[t[:, 0] == 0, k]
        r = float(np.corrcoef(t[:, 0], t[:, k])[0, 1]) if tp.size and fp.size and t[:, k].std() > 0 else None
        out["quantities"][q] = dict(pearson_r_with_true_positive=r, mean_true_positive=float(tp.mean()) if tp.size else None,
                                    mean_false_positive=float(fp.mean()) if fp.size else None)
    return out


def _verify_eval(args, cat_paths, sampler, encs, pencs, trained, weights, dev):
    """--mask-free --score agreement / --min-agreement / --min-fill: see the module docstring"""
    cats = list(sampler.categories)
    names = sampler.synset_names
    deg, sh = [5, 10, 15], [5, 10, 15]
    mean25 = lambda iou_aps: float(iou_aps[[names.index(c) for c in cats]].mean(0)[25])
    tuning = None
    min_agreement = args.min_agreement
    if min_agreement is None and args.tune_frames > 0:
        tune_sampler = MF.MeshFrameSampler(cat_paths, args.objects, device=dev, seed=args.seed + 1000)
        tune, _ = _verified_frames(args, tune_sampler, encs, pencs, args.tune_frames, seed0=1_000_000)
        table = []
        for a in [round(0.05 * k, 2) for k in range(0, 20)]:
            iou_aps, _, n_det, _, _ = _pooled_ap(tune, tune_sampler, cats, dev, nms_thresh=args.nms, score="agreement", min_agreement=a,
                                                 min_fill=args.min_fill)
            table.append(dict(min_agreement=a, mean_iou25_ap=mean25(iou_aps), detections=n_det))
        best = max(table, key=lambda r: (r["mean_iou25_ap"], -r["min_agreement"]))
        min_agreement = best["min_agreement"]
        tuning = dict(frames=args.tune_frames, sampler_seed=args.seed + 1000, pair_seeds="1000000 + frame", candidates=table, chosen=min_agreement,
                      rule="the candidate with the best mean IoU25 AP on the tuning frames, the lowest bound on a tie")
        print(f"min_agreement chosen on {args.tune_frames} separate frames: {min_agreement}")
    frames, ms = _verified_frames(args, sampler, encs, pencs, args.frames, seed0=0)
    n_gt = sum(len(fr.categories) for fr, _ in frames)
    variants = [("score_diff", dict(score="diff")), ("score_agreement", dict(score="agreement")),
                ("score_agreement_filtered", dict(score="agreement", min_agreement=min_agreement, min_fill=args.min_fill))]
    variants = [(n, dict(kw, nms_thresh=args.nms)) for n, kw in variants]
    if args.cross_category:
        variants += [(n + "_cross_category", dict(kw, cross_category=True)) for n, kw in list(variants)]
    variants.insert(0, ("score_diff_no_nms", dict(score="diff", nms_thresh=None)))      # (profiles/scene_poses_eval.json's figure, re-run)
    rec = dict(device=torch.cuda.get_device_name(0), mode="mask-free: scene_frame(verify=True) per category on the whole depth image; the same "
               "proposals pooled by detections.pool_detections with NMS per category, ranked by diff, by agreement, and by agreement behind "
               "the filters", frames=args.frames, objects_per_frame=args.objects, scene_pairs=args.scene_pairs, thresh=args.thresh,
               max_proposals=args.max_proposals, nms_thresh=args.nms, seed=args.seed, categories={c: len(p) for c, p in cat_paths.items()},
               procedural=bool(args.procedural), trained=trained, weights=weights, ground_truths=n_gt,
               ms_per_frame_median_with_verify=float(np.median(ms[min(1, len(ms) - 1):])), min_agreement=min_agreement, min_fill=args.min_fill,
               tuning=tuning, variants={}, note="figures: no threshold is attached to these APs")
    for name, kw in variants:
        iou_aps, pose_aps, n_det, kept, filtered = _pooled_ap(frames, sampler, cats, dev, **kw)
        one = dict(pool=kw, evaluated_predictions=n_det, detections_kept=int(sum(kept.values())),
                   detections_kept_per_ground_truth=round(sum(kept.values()) / max(n_gt, 1), 3), kept_per_category=kept,
                   filtered_per_category=filtered, iou_ap={}, pose_ap={})
        print(f"--- {name}: kept {sum(kept.values())} for {n_gt} ground truths, filtered {sum(filtered.values())}")
        _tables(iou_aps, pose_aps, names, cats, deg, sh, one)
        rec["variants"][name] = one
    rec["true_positive_correlation"] = _true_positive_table(frames, sampler, cats)
    print("true positives among the un-suppressed proposals:", json.dumps(rec["true_positive_correlation"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", action="append", help="CATEGORY=directory of OBJ files or names file (repeatable)")
    ap.add_argument("--shapenet-root", default=None)
    ap.add_argument("--procedural", action="store_true", help="procedural bottle / can / camera meshes instead of --meshes")
    ap.add_argument("--weights", action="append", help="CATEGORY=weights file (repeatable)")
    ap.add_argument("--train-steps", type=int, default=0, help="train each category without --weights for N steps first")
    ap.add_argument("--train-pairs", type=int, default=60000, help="pairs per training step (train_on_meshes' n_pairs)")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--objects", type=int, default=4)
    ap.add_argument("--min-pixels", type=int, default=400, help="instances with fewer visible pixels get no mask (unmatched ground truth)")
    ap.add_argument("--n-pairs", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mask-free", action="store_true", help="no masks: scene_frame per category on the whole image (see above)")
    ap.add_argument("--scene-pairs", type=int, default=1_000_000, help="--mask-free: pairs drawn over the whole frame")
    ap.add_argument("--thresh", type=float, default=50.0, help="--mask-free: the proposal loop's threshold")
    ap.add_argument("--max-proposals", type=int, default=6, help="--mask-free: proposals per category and frame (the 20 best-scored "
                    "predictions of a frame are evaluated)")
    ap.add_argument("--refine", action="store_true", help="--mask-free: also refine every proposal as an instance (scene_poses.refine_poses) "
                    "and report the AP table with and without it from the same frames")
    ap.add_argument("--nms", type=float, default=None, metavar="T", help="--mask-free: the frames go through detections.frame_detections "
                    "with 3D box NMS per category at IoU threshold T (the reference's 0.3); AP with and without it from the same frames")
    ap.add_argument("--cross-category", action="store_true", help="--mask-free --nms: also a second NMS pass over the survivors of "
                    "all categories (scores of different networks are not calibrated against each other)")
    ap.add_argument("--score", choices=("diff", "agreement", "peak"), default="diff", help="--mask-free: 'agreement' evaluates proposal "
                    "verification (scene_frame(verify=True)): the same proposals ranked by diff, by agreement and by agreement behind the filters; "
                    "--segment-instances: 'agreement' (also what the default stands for there) or 'peak', segment_detections' scores")
    ap.add_argument("--segment-instances", action="store_true", help="the frame's depth segments taken as instance masks: "
                    "detections.segment_detections, no scene stage (DESIGN.md 3.7m); with --planes / --concave / --select / --score")
    ap.add_argument("--select", choices=("best", "all"), default="best", help="--segment-instances: the best candidate per segment, or all")
    ap.add_argument("--max-extent-ratio", type=float, default=None, help="--segment-instances: segment_detections' max_extent_ratio")
    ap.add_argument("--min-agreement", type=float, default=None, help="--mask-free --score agreement: the filter's bound (default: chosen "
                    "on --tune-frames separate frames)")
    ap.add_argument("--min-fill", type=float, default=None, help="--mask-free --score agreement: drop proposals whose mask fills less of "
                    "their box")
    ap.add_argument("--tune-frames", type=int, default=0, help="--score agreement without --min-agreement: frames of a separate sampler "
                    "(seed + 1000) on which the bound is chosen")
    ap.add_argument("--segments", action="store_true", help="--mask-free: segment every frame on the device first and draw the pairs inside "
                    "the segments (DESIGN.md 3.7j)")
    ap.add_argument("--seg-planes", "--planes", type=int, default=0, help="--segments: planes removed before the labelling (0 suits rendered "
                    "frames without a support)")
    ap.add_argument("--concave", action="store_true", help="--segments: cut the frame at its concave creases before the labelling "
                    "(segments.frame_segments(concave={}), DESIGN.md 3.7l)")
    ap.add_argument("--tabletop", action="store_true", help="frames of objects standing on a support plane (mesh_frames.TabletopFrameSampler) "
                    "instead of objects floating in empty space")
    ap.add_argument("--min-gap", type=float, default=0.0, help="--tabletop: the least distance between two footprints in metres (0: contact)")
    ap.add_argument("--seg-min-pixels", type=int, default=200, help="--segments: the smallest component kept")
    ap.add_argument("--seg-tol-mm", type=int, default=10, help="--segments: the link rule's constant term")
    ap.add_argument("--seg-slope", type=int, default=10, help="--segments: the link rule's slope, per mille of the nearer depth")
    ap.add_argument("--intra-frac", type=float, default=1.0, help="--segments: share of the pairs drawn inside one segment")
    ap.add_argument("--out", default=None, help="default profiles/mesh_frames_eval.json (profiles/scene_poses_eval.json with --mask-free, "
                    "profiles/scene_detections_eval.json with --nms, profiles/scene_verify_eval.json with --score agreement)")
    args = ap.parse_args()
    args.seg_log = []
    verify_mode = not args.segment_instances and (args.score == "agreement" or args.min_agreement is not None or args.min_fill is not None)
    if args.segment_instances and (args.mask_free or args.segments or args.refine or args.cross_category):
        sys.exit("--segment-instances is a mode of its own: it takes --planes, --concave, --select, --score, --nms, --n-pairs and --tabletop")
    if args.score == "peak" and not args.segment_instances:
        sys.exit("--score peak belongs to --segment-instances")
    if args.segment_instances and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "segment_instances_eval.json")
    if (args.cross_category or verify_mode) and args.nms is None:
        args.nms = 0.3
    if verify_mode and not args.mask_free:
        sys.exit("--score agreement / --min-agreement / --min-fill belong to --mask-free")
    if verify_mode and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "scene_verify_eval.json")
    if args.nms is not None and not (args.mask_free or args.segment_instances):
        sys.exit("--nms / --cross-category belong to --mask-free")
    if args.refine and (not args.mask_free or args.nms is not None or verify_mode):
        sys.exit("--refine belongs to the plain --mask-free run (no --nms, no --score agreement)")
    if args.segments and (not args.mask_free or verify_mode):
        sys.exit("--segments belongs to --mask-free (plain, --nms or --refine)")
    if args.concave and not (args.segments or args.segment_instances):
        sys.exit("--concave belongs to --segments or --segment-instances")
    if args.tabletop and verify_mode:
        sys.exit("--tabletop: the verification run tunes on a second sampler of floating objects; not wired up")
    if args.segments and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "segments_eval.json")
    if args.refine and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "refine_eval.json")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "scene_detections_eval.json" if args.nms is not None else
                                ("scene_poses_eval.json" if args.mask_free else "mesh_frames_eval.json"))
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    if args.procedural:
        cat_paths = _procedural(tmp.name)
    else:
        cat_paths = {c: M.mesh_paths(p, args.shapenet_root) for c, p in _pairs(args.meshes, "meshes").items()}
    if not cat_paths or not all(cat_paths.values()):
        sys.exit("no meshes: --meshes CATEGORY=DIR (repeatable) or --procedural")
    for c in cat_paths:
        if c not in CATEGORIES:
            sys.exit(f"category {c!r} has no built-in config")
    weights = _pairs(args.weights, "weights")
    encs, pencs, trained = {}, {}, {}
    for c, paths in cat_paths.items():
        if c in weights:
            pencs[c], encs[c] = training.load_weights(weights[c], CATEGORIES[c], dev)
        elif args.train_steps > 0:
            t0 = time.perf_counter()
            pencs[c], encs[c], losses = training.train_on_meshes(c, paths, dev, steps=args.train_steps, n_pairs=args.train_pairs,
                                                                     seed=args.seed)
            torch.cuda.synchronize()
            trained[c] = dict(steps=args.train_steps, pairs=args.train_pairs, seconds=time.perf_counter() - t0, final_loss=float(losses[-1]))
            print(f"{c}: trained {args.train_steps} steps on {len(paths)} meshes in {trained[c]['seconds']:.1f} s, loss {losses[-1]:.4f}")
        else:
            sys.exit(f"category {c}: --weights {c}=FILE or --train-steps N")
    if args.tabletop:
        sampler = MF.TabletopFrameSampler(cat_paths, args.objects, device=dev, seed=args.seed, min_gap=args.min_gap)
    else:
        sampler = MF.MeshFrameSampler(cat_paths, args.objects, device=dev, seed=args.seed)
    if verify_mode:
        _verify_eval(args, cat_paths, sampler, encs, pencs, trained, weights, dev)
        tmp.cleanup()
        return
    if args.segment_instances:
        results, ms, count = _segment_instances(args, sampler, encs, pencs, dev)
        deg, sh = [5, 10, 15], [5, 10, 15]
        iou = [float(t) for t in np.round(np.linspace(0, 1, 101), 2)]
        score = "peak" if args.score == "peak" else "agreement"
        n_fr = max(args.frames, 1)
        rec = dict(device=torch.cuda.get_device_name(0), mode="segment instances: detections.segment_detections -- the depth segments as "
                   "instance masks, every category's instance path on every segment, no scene stage; the same candidates pooled under "
                   "select best / all and score agreement / peak", frames=args.frames, objects_per_frame=args.objects, n_pairs=args.n_pairs,
                   nms_thresh=args.nms if args.nms is not None else 0.3, max_extent_ratio=args.max_extent_ratio, seed=args.seed,
                   timed_variant=f"{args.select}/{score}", categories={c: len(p) for c, p in cat_paths.items()},
                   procedural=bool(args.procedural), trained=trained, weights=weights, ground_truths=count["ground_truths"],
                   ms_per_frame_median=float(np.median(ms[min(3, len(ms) - 1):])), segments_per_frame=count["segments"] / n_fr,
                   candidates_per_frame=count["candidates"] / n_fr, refused_per_frame=count["refused"] / n_fr,
                   skipped_min_points_per_frame=count["skipped_min_points"] / n_fr, skipped_extent_per_frame=count["skipped_extent"] / n_fr,
                   detections_per_frame=count["detections"] / n_fr, objects_with_a_segment=count["objects_with_a_segment"],
                   best_picked_the_true_category=count["best_true_category"],
                   segments=dict(n_planes=args.seg_planes, min_pixels=args.seg_min_pixels, tol_mm=args.seg_tol_mm, slope_permille=args.seg_slope,
                                 concave=bool(args.concave)),
                   variants={}, note="figures: no threshold is attached to these APs")
        if args.tabletop:
            rec["tabletop"] = dict(min_gap=args.min_gap)
        print(f"{args.frames} frames, {count['ground_truths']} ground truths, {rec['segments_per_frame']:.1f} segments, "
              f"{rec['candidates_per_frame']:.1f} candidates and {rec['refused_per_frame']:.2f} refusals per frame; "
              f"{rec['ms_per_frame_median']:.1f} ms per frame (median after the first 3; {rec['timed_variant']}); best picked the true category of "
              f"{count['objects_with_a_segment']} objects with a segment: {count['best_true_category']}")
        for v, recs in results.items():
            iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP(recs, sampler.synset_names, None, deg, sh, iou, 0.1, True, device=dev)
            one = dict(evaluated_predictions=int(sum(len(r["pred_class_ids"]) for r in recs)), iou_ap={}, pose_ap={})
            print(f"--- select/score {v}: {one['evaluated_predictions']} predictions")
            _tables(iou_aps, pose_aps, sampler.synset_names, list(cat_paths), deg, sh, one)
            rec["variants"][v] = one
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
        tmp.cleanup()
        return
    if args.mask_free and args.nms is not None:
        results, ms, counts, n_prop, n_gt = _detections(args, sampler, encs, pencs, dev)
        deg, sh = [5, 10, 15], [5, 10, 15]
        iou = [float(t) for t in np.round(np.linspace(0, 1, 101), 2)]
        rec = dict(device=torch.cuda.get_device_name(0), mode="mask-free: detections.frame_detections on the whole depth image; the same "
                   "proposals pooled without NMS, with NMS per category" + (" and with the cross-category pass" if args.cross_category else ""),
                   frames=args.frames, objects_per_frame=args.objects, scene_pairs=args.scene_pairs, thresh=args.thresh,
                   max_proposals=args.max_proposals, nms_thresh=args.nms, seed=args.seed, categories={c: len(p) for c, p in cat_paths.items()},
                   procedural=bool(args.procedural), trained=trained, weights=weights, ground_truths=n_gt, proposals=n_prop,
                   ms_per_frame_median=float(np.median(ms[min(1, len(ms) - 1):])), variants={},
                   note="a first figure: no threshold is attached to these APs")
        if args.segments:
            rec["segments"] = _segments_record(args, args.seg_log)
        if args.tabletop:
            rec["tabletop"] = dict(min_gap=args.min_gap)
        print(f"{args.frames} frames, {n_gt} ground truths, {n_prop} proposals; {rec['ms_per_frame_median']:.1f} ms per frame (all categories, NMS included)")
        for v, recs in results.items():
            iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP(recs, sampler.synset_names, None, deg, sh, iou, 0.1, True, device=dev)
            one = dict(evaluated_predictions=int(sum(len(r["pred_class_ids"]) for r in recs)),
                       kept_suppressed_per_category={c: dict(kept=k, suppressed=s_) for c, (k, s_) in counts[v].items()}, iou_ap={}, pose_ap={})
            print(f"--- {v}: " + ", ".join(f"{c} kept {k} suppressed {s_}" for c, (k, s_) in counts[v].items()))
            _tables(iou_aps, pose_aps, sampler.synset_names, list(cat_paths), deg, sh, one)
            rec["variants"][v] = one
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
        tmp.cleanup()
        return
    if args.mask_free:
        results, ms, n_prop, n_gt, refined, n_ref = _mask_free(args, sampler, encs, pencs, dev)
        deg, sh = [5, 10, 15], [5, 10, 15]
        iou = [float(t) for t in np.round(np.linspace(0, 1, 101), 2)]
        iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP(results, sampler.synset_names, None, deg, sh, iou, 0.1, True, device=dev)
        if refined is not None:
            rec = dict(device=torch.cuda.get_device_name(0), mode="mask-free with refinement: scene_frame(refine=BatchPoseRunner) per category "
                       "on the whole depth image; the same proposals evaluated with the first pass's poses and with the refined ones",
                       frames=args.frames, objects_per_frame=args.objects, scene_pairs=args.scene_pairs, refine_pairs=100000, thresh=args.thresh,
                       max_proposals=args.max_proposals, seed=args.seed, categories={c: len(p) for c, p in cat_paths.items()},
                       procedural=bool(args.procedural), trained=trained, weights=weights, ground_truths=n_gt, proposals=n_prop,
                       proposals_with_a_refined_pose=n_ref, ms_per_frame_median_with_refine=float(np.median(ms[min(3, len(ms) - 1):])),
                       variants={}, note="figures: no threshold is attached to these APs")
            print(f"{args.frames} frames, {n_gt} ground truths, {n_prop} proposals, {n_ref} with a refined pose; "
                  f"{rec['ms_per_frame_median_with_refine']:.1f} ms per frame (all categories, refinement included)")
            r_iou, r_pose, _, _ = E.compute_degree_cm_mAP(refined, sampler.synset_names, None, deg, sh, iou, 0.1, True, device=dev)
            for v, (a, b) in (("first_pass", (iou_aps, pose_aps)), ("refined", (r_iou, r_pose))):
                print(f"--- {v}")
                one = dict(iou_ap={}, pose_ap={})
                _tables(a, b, sampler.synset_names, list(cat_paths), deg, sh, one)
                rec["variants"][v] = one
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            old = {}
            if os.path.exists(args.out):
                with open(args.out) as fh:
                    old = json.load(fh)
            old["mesh_frames"] = rec
            with open(args.out, "w") as fh:
                json.dump(old, fh, indent=1)
                fh.write("\n")
            tmp.cleanup()
            return
        rec = dict(device=torch.cuda.get_device_name(0), mode="mask-free: scene_frame per category on the whole depth image", frames=args.frames,
                   objects_per_frame=args.objects, scene_pairs=args.scene_pairs, thresh=args.thresh, max_proposals=args.max_proposals, seed=args.seed,
                   categories={c: len(p) for c, p in cat_paths.items()}, procedural=bool(args.procedural), trained=trained, weights=weights,
                   ground_truths=n_gt, proposals=n_prop, ms_per_frame_median=float(np.median(ms[min(1, len(ms) - 1):])), iou_ap={}, pose_ap={},
                   note="a first figure: no threshold is attached to these APs")
        if args.segments:
            rec["segments"] = _segments_record(args, args.seg_log)
        if args.tabletop:
            rec["tabletop"] = dict(min_gap=args.min_gap)
        print(f"{args.frames} frames, {n_gt} ground truths, {n_prop} proposals; {rec['ms_per_frame_median']:.1f} ms per frame (all categories)")
        _tables(iou_aps, pose_aps, sampler.synset_names, list(cat_paths), deg, sh, rec)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
        tmp.cleanup()
        return
    runner = FrameRunner(encs, pencs, dev, intrinsics=MF.frame_intrinsics(), n_pairs=args.n_pairs)
    results, ms, n_inst, n_gt, n_none = [], [], 0, 0, 0
    for i in range(args.frames):
        fr = sampler.sample()
        inst = fr.instances(args.min_pixels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses = runner.run(fr.depth_mm, inst, seed=i) if inst else []        # (ends in the frame's read-back)
        ms.append((time.perf_counter() - t0) * 1e3)
        ok = lambda p: all(np.all(np.isfinite(p[k])) for k in ("T", "R", "scale")) and p["scale_norm"] > 0
        poses = [p if p is not None and ok(p) else None for p in poses]       # (a pose that is no pose makes no prediction)
        results.append(fr.record(poses, min_pixels=args.min_pixels))
        n_inst += len(inst)
        n_gt += len(fr.categories)
        n_none += sum(p is None for p in poses)
    deg, sh = [5, 10, 15], [5, 10, 15]
    iou = [float(t) for t in np.round(np.linspace(0, 1, 101), 2)]
    names = sampler.synset_names
    t0 = time.perf_counter()
    iou_aps, pose_aps, _, _ = E.compute_degree_cm_mAP(results, names, None, deg, sh, iou, 0.1, True, device=dev)
    eval_s = time.perf_counter() - t0
    steady = ms[min(3, len(ms) - 1):]                                         # the first frames capture their chains
    rec = dict(device=torch.cuda.get_device_name(0), frames=args.frames, objects_per_frame=args.objects, min_pixels=args.min_pixels,
               n_pairs=args.n_pairs, seed=args.seed, categories={c: len(p) for c, p in cat_paths.items()},
               procedural=bool(args.procedural), trained=trained, weights=weights, ground_truths=n_gt, instances_run=n_inst,
               instances_skipped_by_the_frame_path=n_none, ms_per_frame_median=float(np.median(steady)),
               ms_per_frame_mean=float(np.mean(steady)), evaluation_seconds=eval_s, iou_ap={}, pose_ap={})
    if args.tabletop:
        rec["tabletop"] = dict(min_gap=args.min_gap)
    print(f"{args.frames} frames, {n_gt} ground truths, {n_inst} instances with >= {args.min_pixels} pixels, {n_none} skipped by the frame "
          f"path; {rec['ms_per_frame_median']:.2f} ms per frame (median after the first 3), evaluation {eval_s:.2f} s")
    _tables(iou_aps, pose_aps, names, list(cat_paths), deg, sh, rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    tmp.cleanup()


if __name__ == "__main__":
    main()
