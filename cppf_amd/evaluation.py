"""NOCS evaluation of pose predictions: 3D-IoU AP and degree / centimetre AP over the
result dictionaries `nocs/inference.py:338-345` pickles (see cppf_amd.inference.nocs_result for this package's side).

Two paths with the same entry points, arguments, return values and matching rules as the reference (`utils/util.py:181-255,
342-527,709-1008`, driven by `nocs/eval.py:16-49`):

* the host path (device=None) is numpy, like the reference's, and is the checker of the other one;
* the device path (device=a HIP device) flattens the whole result list once into (image, class) groups and work pairs, uploads
  it once, runs the box IoUs with their 20-rotation symmetry sweep, the degree / centimetre errors and both greedy matchings
  in three launches (csrc/pose_eval.hip, include/cppf.h "Pose evaluation") and reads the match tables back once; the AP sums
  stay on the host.  At a pose every 0.2 ms the host metric (about 1.3 ms per box pair with the sweep) is the slow end of a
  REAL275-sized run; pose_metrics_device gives a training loop the per-pair figures without leaving the device.

The implementation is this repository's own:

* the intersection volume of two oriented boxes is computed with the divergence theorem over the clipped faces of
  both boxes (each face of one box clipped by the six half-spaces of the other), not by collecting intersection points
  and taking their convex hull (`utils/iou.py`); the two agree to rounding (tests/golden/eval_map.npz: <= 1e-6);
* no plots are drawn (the reference's figures are a side effect; the AP tables it pickles next to them are written when
  `log_dir` is given).

nms_3d / nms_results are the scene-level post-processing of `sunrgbd/eval.py:13-35,110-145`: greedy 3D non-maximum suppression per
(image, class) over the same oriented-box IoU, on the host (the checker) or on the device (csrc/box_nms.hip, include/cppf.h
"Box NMS"; pinned on the reference's own pick lists, tests/golden/make_golden_nms.py -> nms_cases.npz).

Parity is pinned on outputs of the reference's own functions for seeded synthetic results (tests/golden/
make_golden_eval.py -> eval_map.npz; tests/test_evaluation.py)."""
import math
import os
import pickle

import numpy as np

SYNSET_NAMES = ["BG", "bottle", "bowl", "camera", "can", "laptop", "mug"]      # nocs/inference.py:19-27
_UP_SYMMETRIC = ("bowl", "bottle", "can")                                       # nocs/eval.py:32

# ------------------------------------------------------------------------------------------------ oriented boxes
_SIGNS = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
_EPS = 1e-9


def _frame(RT, scales):
    """(centre, unit axes as columns, half extents) of the box `Box.from_transformation(R / cbrt(det R), t, scales)`
    (utils/util.py:188-191); a residual scale in a column of R goes into that axis' extent."""
    R = np.asarray(RT, dtype=np.float64)[:3, :3]
    R = R / np.cbrt(np.linalg.det(R))
    norms = np.linalg.norm(R, axis=0)
    return np.asarray(RT, dtype=np.float64)[:3, 3].copy(), R / norms, 0.5 * np.asarray(scales, dtype=np.float64) * norms


def _faces(c, U, h):
    """the six faces of a box: (outward unit normal, plane offset n.x = d, 4 corners in cyclic order)"""
    out = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        for s in (1.0, -1.0):
            ctr = c + s * h[k] * U[:, k]
            ea, eb = h[a] * U[:, a], h[b] * U[:, b]
            quad = np.array([ctr - ea - eb, ctr + ea - eb, ctr + ea + eb, ctr - ea + eb])
            n = s * U[:, k]
            out.append((n, float(n @ ctr), quad))
    return out


def _clip(poly, n, d, tol):
    """part of the convex polygon `poly` ([m,3]) inside the half-space n.x <= d; `tol` only decides on which side a
    vertex that lies on the plane (to rounding) falls -- crossings are computed on the plane itself"""
    if len(poly) == 0:
        return poly
    dist = poly @ n - d
    inside = dist <= tol
    if inside.all():
        return poly
    if not inside.any():
        return poly[:0]
    out = []
    m = len(poly)
    for i in range(m):
        j = (i + 1) % m
        if inside[i]:
            out.append(poly[i])
        if inside[i] != inside[j]:
            t = min(1.0, max(0.0, dist[i] / (dist[i] - dist[j])))
            out.append(poly[i] + t * (poly[j] - poly[i]))
    return np.array(out)


def _flux(poly, n, d):
    """(n . x) * area of a planar convex polygon lying in the plane n.x = d"""
    if len(poly) < 3:
        return 0.0
    v = poly[1:] - poly[0]
    area = 0.5 * np.linalg.norm(np.cross(v[:-1], v[1:]).sum(0))
    return d * area


def box_intersection_volume(c1, U1, h1, c2, U2, h2):
    """volume of the intersection of two oriented boxes: V = 1/3 * sum over the faces of the intersection polytope of
    (n . x) * area.  Those faces are the faces of box 1 clipped by box 2 and vice versa; a face the two boxes share
    (coincident planes) is counted once: box 1's faces are clipped by closed half-spaces, box 2's by open ones.  A half-space
    whose normal points against the face's own normal is open for both boxes: two boxes that touch from opposite sides of a
    plane share no volume, and the face they share is a face of neither's intersection (counted once it would add d * area)."""
    f1, f2 = _faces(c1, U1, h1), _faces(c2, U2, h2)
    scale = float(max(h1.max(), h2.max()))
    tol = 1e-9 * scale
    total = 0.0
    for mine, other, t in ((f1, f2, tol), (f2, f1, -tol)):
        for n, d, quad in mine:
            poly = quad
            for n2, d2, _ in other:
                against = (n[0] * n2[0] + n[1] * n2[1]) + n[2] * n2[2] < 0.0
                poly = _clip(poly, n2, d2, -tol if against else t)
                if len(poly) < 3:
                    break
            total += _flux(poly, n, d)
    return max(total / 3.0, 0.0)


def _iou_frames(a, b):
    v = box_intersection_volume(*a, *b)
    va, vb = 8.0 * np.prod(a[2]), 8.0 * np.prod(b[2])
    if v <= _EPS * min(va, vb):
        return 0.0
    return float(v / (va + vb - v))


def _rot_y(theta):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, 0.0, s, 0.0], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, 0.0], [0.0, 0.0, 0.0, 1.0]])


def compute_3d_iou(RT_1, RT_2, scales_1, scales_2, up_sym, class_name_1, class_name_2):
    """utils/util.py:181-216: IoU of the boxes (RT_k normalised to a rotation, extents scales_k); for an up-symmetric
    ground truth of the same class the best of 20 rotations of box 1 about its own y axis.  -1 when a pose is missing."""
    if RT_1 is None or RT_2 is None:
        return -1
    try:
        fb = _frame(RT_2, scales_2)
        if class_name_1 == class_name_2 and up_sym:
            return max(_iou_frames(_frame(np.asarray(RT_1, dtype=np.float64) @ _rot_y(2.0 * math.pi * i / 20.0), scales_1), fb)
                       for i in range(20))
        return _iou_frames(_frame(RT_1, scales_1), fb)
    except (np.linalg.LinAlgError, FloatingPointError, ValueError):
        return 0


def compute_RT_degree_cm_symmetry(RT_1, RT_2, up_sym):
    """utils/util.py:219-255: [rotation error in degrees, translation error in centimetres]; with `up_sym` only the
    angle between the two y axes counts."""
    if RT_1 is None or RT_2 is None:
        return -1
    RT_1, RT_2 = np.asarray(RT_1, dtype=np.float64), np.asarray(RT_2, dtype=np.float64)
    if not (np.array_equal(RT_1[3], RT_2[3]) and np.array_equal(RT_1[3], [0, 0, 0, 1])):
        raise ValueError(f"homogeneous rows differ from [0 0 0 1]: {RT_1[3]} {RT_2[3]}")
    R1 = RT_1[:3, :3] / np.cbrt(np.linalg.det(RT_1[:3, :3]))
    R2 = RT_2[:3, :3] / np.cbrt(np.linalg.det(RT_2[:3, :3]))
    if up_sym:
        y1, y2 = R1[:, 1], R2[:, 1]
        cosv = y1.dot(y2) / (np.linalg.norm(y1) * np.linalg.norm(y2))
    else:
        cosv = (np.trace(R1 @ R2.T) - 1.0) / 2.0
    theta = math.degrees(math.acos(min(1.0, max(-1.0, float(cosv)))))     # (the reference lets rounding above 1 become NaN)
    return np.array([theta, np.linalg.norm(RT_1[:3, 3] - RT_2[:3, 3]) * 100.0])


# ------------------------------------------------------------------------------------------------ matching
def compute_3d_matches(gt_class_ids, gt_RTs, gt_scales, gt_up_syms, synset_names, pred_boxes, pred_class_ids, pred_scores,
                       pred_RTs, pred_scales, iou_3d_thresholds, score_threshold=0):
    """utils/util.py:342-416.  Predictions in descending score order claim, per IoU threshold, the unclaimed ground truth
    of their class with the highest IoU above the threshold (a candidate below it ends the search).  Returns
    (gt_matches [T, n_gt], pred_matches [T, n_pred] in sorted order, overlaps [n_pred, n_gt] float32, the sort order)."""
    n_pred, n_gt = len(pred_class_ids), len(gt_class_ids)
    order = np.zeros(0)
    if n_pred:
        order = np.argsort(pred_scores)[::-1]
        pred_class_ids, pred_scales, pred_RTs = pred_class_ids[order], pred_scales[order], pred_RTs[order]
    overlaps = np.zeros((n_pred, n_gt), dtype=np.float32)
    for i in range(n_pred):
        for j in range(n_gt):
            overlaps[i, j] = compute_3d_iou(pred_RTs[i], gt_RTs[j], pred_scales[i], gt_scales[j], gt_up_syms[j],
                                            synset_names[pred_class_ids[i]], synset_names[gt_class_ids[j]])
    n_thr = len(iou_3d_thresholds)
    pred_matches = -np.ones((n_thr, n_pred))
    gt_matches = -np.ones((n_thr, n_gt))
    ranked = [np.argsort(overlaps[i])[::-1] for i in range(n_pred)]
    for i in range(n_pred):
        keep = overlaps[i, ranked[i]] >= score_threshold
        if not keep.all():
            ranked[i] = ranked[i][:int(np.argmin(keep))]
    for s, thr in enumerate(iou_3d_thresholds):
        for i in range(n_pred):
            for j in ranked[i]:
                if gt_matches[s, j] > -1:
                    continue
                iou = overlaps[i, j]
                if iou < thr:
                    break
                if pred_class_ids[i] != gt_class_ids[j]:
                    continue
                if iou > thr:
                    gt_matches[s, j] = i
                    pred_matches[s, i] = j
                    break
    return gt_matches, pred_matches, overlaps, order


def compute_RT_overlaps(gt_class_ids, gt_RTs, gt_up_syms, pred_class_ids, pred_RTs):
    """utils/util.py:447-467: [n_pred, n_gt, 2] (degrees, centimetres)"""
    out = np.zeros((len(pred_class_ids), len(gt_class_ids), 2))
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            out[i, j] = compute_RT_degree_cm_symmetry(pred_RTs[i], gt_RTs[j], gt_up_syms[j])
    return out


def compute_match_from_degree_cm(overlaps, pred_class_ids, gt_class_ids, degree_thres_list, shift_thres_list):
    """utils/util.py:470-517: per (degree, shift) threshold pair every prediction takes the unclaimed ground truth of
    its class with the smallest degree + centimetre sum that is inside both thresholds."""
    n_pred, n_gt = len(pred_class_ids), len(gt_class_ids)
    pred_matches = -np.ones((len(degree_thres_list), len(shift_thres_list), n_pred))
    gt_matches = -np.ones((len(degree_thres_list), len(shift_thres_list), n_gt))
    if n_pred == 0 or n_gt == 0:
        return gt_matches, pred_matches
    if overlaps.shape != (n_pred, n_gt, 2):
        raise ValueError(f"overlaps {overlaps.shape} for {n_pred} predictions and {n_gt} ground truths")
    ranked = [np.argsort(overlaps[i].sum(-1)) for i in range(n_pred)]
    same = np.asarray(pred_class_ids)[:, None] == np.asarray(gt_class_ids)[None, :]
    for d, deg in enumerate(degree_thres_list):
        for s, sh in enumerate(shift_thres_list):
            for i in range(n_pred):
                for j in ranked[i]:
                    if gt_matches[d, s, j] > -1 or not same[i, j]:
                        continue
                    if overlaps[i, j, 0] > deg or overlaps[i, j, 1] > sh:
                        continue
                    gt_matches[d, s, j] = i
                    pred_matches[d, s, i] = j
                    break
    return gt_matches, pred_matches


def compute_ap_from_matches_scores(pred_match, pred_scores, gt_match):
    """utils/util.py:419-444: VOC-style AP (precision made monotone from the right, summed over recall steps)"""
    if pred_match.shape[0] != pred_scores.shape[0]:
        raise ValueError("one score per prediction")
    hit = (pred_match[np.argsort(pred_scores)[::-1]] > -1)
    tp = np.cumsum(hit)
    precisions = np.concatenate([[0.0], tp / (np.arange(len(hit)) + 1), [0.0]])
    recalls = np.concatenate([[0.0], tp.astype(np.float32) / len(gt_match), [1.0]])
    precisions = np.maximum.accumulate(precisions[::-1])[::-1]
    steps = np.where(recalls[:-1] != recalls[1:])[0] + 1
    return np.sum((recalls[steps] - recalls[steps - 1]) * precisions[steps])


# ------------------------------------------------------------------------------------------------ the metric
def _unit_scale(RTs, scales, eps):
    """RTs with the scale taken out of the rotation block, and the extents multiplied by it (utils/util.py:754-768)"""
    RTs = np.array(RTs, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)
    if len(RTs) == 0:
        return RTs.reshape(0, 4, 4), scales.reshape(0, 3)
    s = np.cbrt(np.linalg.det(RTs[:, :3, :3]))
    RTs[:, :3, :3] = RTs[:, :3, :3] / (s[:, None, None] + eps)
    return RTs, scales * s[:, None]


def _write_tables(log_dir, iou_list, deg_list, sh_list, iou_3d_aps, pose_aps, use_matches_for_pose):
    """the two tables the reference pickles next to its figures"""
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "IoU_3D_AP_{}-{}.pkl".format(iou_list[0], iou_list[-1])), "wb") as f:
        pickle.dump({"thres_list": iou_list, "aps": iou_3d_aps}, f)
    prefix = "Pose_Only_" if use_matches_for_pose else "Pose_Detection_"
    name = prefix + "AP_{}-{}degree_{}-{}cm.pkl".format(deg_list[0], deg_list[-2], sh_list[0], sh_list[-2])
    with open(os.path.join(log_dir, name), "wb") as f:
        pickle.dump({"degree_thres": deg_list, "shift_thres_list": sh_list, "aps": pose_aps}, f)


def compute_degree_cm_mAP(final_results, synset_names, log_dir, degree_thresholds=[360], shift_thresholds=[100],
                          iou_3d_thresholds=[0.1], iou_pose_thres=0.1, use_matches_for_pose=False, device=None):
    """utils/util.py:709-1008 (called by nocs/eval.py:44-49).  final_results: one dict per image with gt_class_ids,
    gt_RTs, gt_scales, gt_up_syms, pred_class_ids, pred_RTs, pred_scales, pred_scores (pred_bboxes is ignored, as there).
    Returns (iou_3d_aps [C+1, T], pose_aps [C+1, D+1, S+1], pose_pred_matches, pose_gt_matches [D+1, S+1, images, 20]);
    row C of the AP tables is the mean over the classes, the extra threshold is 360 degrees / 100 cm.
    device: None = the host path; a HIP device = IoUs, errors and matchings on that device (same return values; see
    _map_on_device for what it checks first)."""
    if device is not None:
        return _map_on_device(final_results, synset_names, log_dir, degree_thresholds, shift_thresholds, iou_3d_thresholds,
                              iou_pose_thres, use_matches_for_pose, device)
    n_cls = len(synset_names)
    deg_list = list(degree_thresholds) + [360]
    sh_list = list(shift_thresholds) + [100]
    iou_list = list(iou_3d_thresholds)
    nD, nS, nT = len(deg_list), len(sh_list), len(iou_list)
    if use_matches_for_pose and iou_pose_thres not in iou_list:
        raise ValueError("iou_pose_thres must be one of iou_3d_thresholds")
    iou_pm = [np.zeros((nT, 0)) for _ in range(n_cls)]
    iou_ps = [np.zeros((nT, 0)) for _ in range(n_cls)]
    iou_gm = [np.zeros((nT, 0)) for _ in range(n_cls)]
    pose_pm = [np.zeros((nD, nS, 0)) for _ in range(n_cls)]
    pose_ps = [np.zeros((nD, nS, 0)) for _ in range(n_cls)]
    pose_gm = [np.zeros((nD, nS, 0)) for _ in range(n_cls)]
    pose_gt_matches = np.full((nD, nS, len(final_results), 20), -1, dtype=int)
    pose_pred_matches = np.full((nD, nS, len(final_results), 20), -1, dtype=int)

    for img, res in enumerate(final_results):
        gt_cls = np.asarray(res["gt_class_ids"]).astype(np.int32)
        gt_RTs, gt_scales = _unit_scale(res["gt_RTs"], res["gt_scales"], 0.0)
        gt_sym = np.asarray(res["gt_up_syms"])
        pr_cls = np.asarray(res["pred_class_ids"])
        pr_scores = np.asarray(res["pred_scores"])
        pr_RTs, pr_scales = _unit_scale(res["pred_RTs"], res["pred_scales"], 1e-9)
        if len(gt_cls) == 0 and len(pr_cls) == 0:
            continue
        for c in range(1, n_cls):
            g_sel = np.where(gt_cls == c)[0] if len(gt_cls) else np.zeros(0, dtype=int)
            p_sel = np.where(pr_cls == c)[0] if len(pr_cls) else np.zeros(0, dtype=int)
            c_gt_cls, c_gt_RTs, c_gt_scales, c_gt_sym = gt_cls[g_sel], gt_RTs[g_sel], gt_scales[g_sel], gt_sym[g_sel]
            c_pr_cls, c_pr_RTs, c_pr_scales, c_pr_scores = pr_cls[p_sel], pr_RTs[p_sel], pr_scales[p_sel], pr_scores[p_sel]
            gm, pm, _, order = compute_3d_matches(c_gt_cls, c_gt_RTs, c_gt_scales, c_gt_sym, synset_names, None, c_pr_cls,
                                                  c_pr_scores, c_pr_RTs, c_pr_scales, iou_list)
            if len(order):
                p_sel, c_pr_cls, c_pr_RTs, c_pr_scores = p_sel[order], c_pr_cls[order], c_pr_RTs[order], c_pr_scores[order]
            iou_pm[c] = np.concatenate((iou_pm[c], pm), -1)
            iou_ps[c] = np.concatenate((iou_ps[c], np.tile(c_pr_scores, (nT, 1))), -1)
            iou_gm[c] = np.concatenate((iou_gm[c], gm), -1)
            if use_matches_for_pose:                       # only the instances matched at iou_pose_thres are scored for pose
                k = iou_list.index(iou_pose_thres)
                keep_p, keep_g = pm[k] > -1, gm[k] > -1
                p_sel, c_pr_cls, c_pr_RTs, c_pr_scores = p_sel[keep_p], c_pr_cls[keep_p], c_pr_RTs[keep_p], c_pr_scores[keep_p]
                g_sel, c_gt_cls, c_gt_RTs, c_gt_sym = g_sel[keep_g], c_gt_cls[keep_g], c_gt_RTs[keep_g], c_gt_sym[keep_g]
            errs = compute_RT_overlaps(c_gt_cls, c_gt_RTs, c_gt_sym, c_pr_cls, c_pr_RTs)
            p_gm, p_pm = compute_match_from_degree_cm(errs, c_pr_cls, c_gt_cls, deg_list, sh_list)
            # per-image tables in the image's own instance numbering
            for i in range(p_pm.shape[2]):
                m = p_pm[:, :, i].astype(int)
                pose_pred_matches[:, :, img, p_sel[i]] = np.where(m >= 0, g_sel[np.maximum(m, 0)] if len(g_sel) else -1, -1)
            for i in range(p_gm.shape[2]):
                m = p_gm[:, :, i].astype(int)
                pose_gt_matches[:, :, img, g_sel[i]] = np.where(m >= 0, p_sel[np.maximum(m, 0)] if len(p_sel) else -1, -1)
            pose_pm[c] = np.concatenate((pose_pm[c], p_pm), -1)
            pose_ps[c] = np.concatenate((pose_ps[c], np.tile(c_pr_scores, (nD, nS, 1))), -1)
            pose_gm[c] = np.concatenate((pose_gm[c], p_gm), -1)

    iou_3d_aps = np.zeros((n_cls + 1, nT))
    pose_aps = np.zeros((n_cls + 1, nD, nS))
    for c in range(1, n_cls):
        for s in range(nT):
            iou_3d_aps[c, s] = compute_ap_from_matches_scores(iou_pm[c][s], iou_ps[c][s], iou_gm[c][s])
        for d in range(nD):
            for s in range(nS):
                pose_aps[c, d, s] = compute_ap_from_matches_scores(pose_pm[c][d, s], pose_ps[c][d, s], pose_gm[c][d, s])
    iou_3d_aps[-1] = iou_3d_aps[1:-1].mean(0)
    pose_aps[-1] = pose_aps[1:-1].mean(0)
    if log_dir:
        _write_tables(log_dir, iou_list, deg_list, sh_list, iou_3d_aps, pose_aps, use_matches_for_pose)
    return iou_3d_aps, pose_aps, pose_pred_matches, pose_gt_matches


# ------------------------------------------------------------------------------------------------ the device path
GROUP_CAP = 32      # predictions / ground truths of one (image, class) group: include/cppf.h CPPF_POSE_EVAL_GROUP_CAP


def _device_tensor(x, np_dtype, device, tail, name):
    """a numpy array or a tensor -> a contiguous tensor of that dtype on `device` with the trailing shape `tail`"""
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np_dtype))
    x = x.to(device=device, dtype=getattr(torch, np.dtype(np_dtype).name)).contiguous()
    if tuple(x.shape[1:]) != tuple(tail) or x.dim() != 1 + len(tail):
        raise ValueError(f"{name}: expected shape [n{''.join(', %d' % t for t in tail)}], got {tuple(x.shape)}")
    return x


def _pairs_on_device(dev, pred_RTs, pred_scales, gt_RTs, gt_scales, gt_up_syms, pairs, sweep):
    """cppf_pose_eval_pairs on device tensors: (iou f64[M], err f64[M,2])"""
    import torch
    from . import _lib
    from ._torch_util import call, scratch, workspace
    M = int(pairs.shape[0])
    iou = torch.empty(M, dtype=torch.float64, device=dev)
    err = torch.empty((M, 2), dtype=torch.float64, device=dev)
    if M:
        need = _lib.lib().cppf_pose_eval_pairs_workspace_bytes(M)
        if need == 0:
            raise ValueError(f"{M} work pairs: more than one call takes")
        ws = workspace(need, dev, "pose_eval")
        call("cppf_pose_eval_pairs", dev, pred_RTs, pred_scales, int(pred_RTs.shape[0]), gt_RTs, gt_scales, gt_up_syms,
             int(gt_RTs.shape[0]), pairs, sweep, M, iou, err, scratch(ws))
    return iou, err


def pose_metrics_device(pred_RTs, pred_scales, gt_RTs, gt_scales, gt_up_syms, pairs, sweep, device=None):
    """Box IoU, rotation error (degrees) and translation error (centimetres) of M (prediction, ground truth) pairs on the device,
    e.g. as a validation metric inside a training loop: no host synchronisation when the arguments are device tensors.

    pred_RTs [Np,4,4], pred_scales [Np,3], gt_RTs [Ng,4,4], gt_scales [Ng,3], gt_up_syms [Ng], pairs [M,2] = (prediction index,
    ground-truth index), sweep [M] (non-zero: this pair's IoU is the best of the 20 rotations of the prediction about its y axis,
    what compute_3d_iou does for an up-symmetric ground truth of the same class); numpy arrays or tensors.  The RTs are used as
    given (compute_3d_iou / compute_RT_degree_cm_symmetry of the same arguments; compute_degree_cm_mAP passes them through
    _unit_scale first).  Returns device tensors (iou f64[M], degrees f64[M], centimetres f64[M]).  A pair index outside the arrays
    raises ValueError when `pairs` is a host array and gives NaN in all three when it is a device tensor."""
    import torch
    from ._torch_util import require_cuda
    require_cuda()
    if device is None:
        on_dev = [x.device for x in (pred_RTs, pred_scales, gt_RTs, gt_scales, gt_up_syms, pairs, sweep)
                  if isinstance(x, torch.Tensor) and x.is_cuda]
        device = on_dev[0] if on_dev else torch.device("cuda", 0)
    dev = torch.device(device)
    if not isinstance(pairs, torch.Tensor):
        pr = np.asarray(pairs).reshape(-1, 2)
        n_p, n_g = len(pred_RTs), len(gt_RTs)
        if len(pr) and (pr.min() < 0 or pr[:, 0].max() >= n_p or pr[:, 1].max() >= n_g):
            raise ValueError(f"pairs: an index outside {n_p} predictions x {n_g} ground truths")
        pairs = pr
    a = _device_tensor(pred_RTs, np.float64, dev, (4, 4), "pred_RTs")
    b = _device_tensor(pred_scales, np.float64, dev, (3,), "pred_scales")
    c = _device_tensor(gt_RTs, np.float64, dev, (4, 4), "gt_RTs")
    d = _device_tensor(gt_scales, np.float64, dev, (3,), "gt_scales")
    e = _device_tensor(gt_up_syms, np.int32, dev, (), "gt_up_syms")
    f = _device_tensor(pairs, np.int32, dev, (2,), "pairs")
    g = _device_tensor(sweep, np.int32, dev, (), "sweep")
    if a.shape[0] != b.shape[0] or c.shape[0] != d.shape[0] or c.shape[0] != e.shape[0] or f.shape[0] != g.shape[0]:
        raise ValueError("pose_metrics_device: one scale row per RT, one symmetry flag per ground truth, one sweep flag per pair")
    iou, err = _pairs_on_device(dev, a, b, c, d, e, f, g)
    return iou, err[:, 0], err[:, 1]


def _check_poses(RTs, scales, img, what):
    """what the device path refuses before anything is uploaded: non-finite values, a singular rotation block, a last row other
    than [0 0 0 1] (the host path divides by the determinant and raises on the last row, pair by pair)"""
    RTs = np.asarray(RTs, dtype=np.float64).reshape(-1, 4, 4)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1, 3)
    if len(RTs) != len(scales):
        raise ValueError(f"image {img}: {len(RTs)} {what} poses and {len(scales)} scales")
    if len(RTs) == 0:
        return
    bad = ~(np.isfinite(RTs).all((1, 2)) & np.isfinite(scales).all(1))
    if bad.any():
        raise ValueError(f"image {img}, {what} instance {int(np.argmax(bad))}: non-finite pose or scale")
    bad = (RTs[:, 3] != np.array([0.0, 0.0, 0.0, 1.0])).any(1)
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError(f"image {img}, {what} instance {k}: homogeneous row {RTs[k, 3]} differs from [0 0 0 1]")
    det = np.linalg.det(RTs[:, :3, :3])
    # zero to rounding: |det| <= 1e-12 * the product of the column norms (a scaled rotation has the ratio 1)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        bad = ~(np.abs(det) > 1e-12 * np.linalg.norm(RTs[:, :3, :3], axis=1).prod(1)) | ~np.isfinite(1.0 / det)
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError(f"image {img}, {what} instance {k}: singular rotation block (determinant {det[k]})")


def _iou_threshold_as_compared(thr):
    """the value the host's `overlaps[i, j] < thr` compares a float32 IoU with: numpy's promotion of (float32 scalar, thr) decides
    whether thr is rounded to float32 first (a Python float under NEP 50) or the IoU is widened (a float64 scalar)"""
    return float(np.asarray(thr).astype(np.result_type(np.float32(0), thr)))


def _flatten_results(final_results, n_cls):
    """the result list as (image, class) groups: every array compute_degree_cm_mAP's loop would select, concatenated in group
    order, predictions in each group in the host's descending-score order.  Groups with neither predictions nor ground truths
    are left out (they add nothing to any table)."""
    acc = dict(pred_RT=[], pred_sc=[], pred_score=[], pred_img=[], pred_inst=[], pred_cls=[], pred_g0=[],
               gt_RT=[], gt_sc=[], gt_sym=[], gt_img=[], gt_inst=[], gt_cls=[], gt_p0=[], pairs=[], sweep=[])
    pred_off, gt_off, pair_off = [0], [0], []
    n_pairs = 0
    for img, res in enumerate(final_results):
        gt_cls = np.asarray(res["gt_class_ids"]).astype(np.int32)
        _check_poses(res["gt_RTs"], res["gt_scales"], img, "ground-truth")
        _check_poses(res["pred_RTs"], res["pred_scales"], img, "predicted")
        gt_RTs, gt_scales = _unit_scale(res["gt_RTs"], res["gt_scales"], 0.0)
        gt_sym = np.asarray(res["gt_up_syms"])
        pr_cls = np.asarray(res["pred_class_ids"])
        pr_scores = np.asarray(res["pred_scores"])
        pr_RTs, pr_scales = _unit_scale(res["pred_RTs"], res["pred_scales"], 1e-9)
        if len(gt_cls) == 0 and len(pr_cls) == 0:
            continue
        if len(gt_sym) != len(gt_cls) or len(gt_RTs) != len(gt_cls) or len(pr_RTs) != len(pr_cls) or len(pr_scores) != len(pr_cls):
            raise ValueError(f"image {img}: one class id, pose, scale (and score / symmetry flag) per instance")
        for c in range(1, n_cls):
            g_sel = np.where(gt_cls == c)[0] if len(gt_cls) else np.zeros(0, dtype=int)
            p_sel = np.where(pr_cls == c)[0] if len(pr_cls) else np.zeros(0, dtype=int)
            n_p, n_g = len(p_sel), len(g_sel)
            if n_p == 0 and n_g == 0:
                continue
            if n_p > GROUP_CAP or n_g > GROUP_CAP:
                raise ValueError(f"image {img}, class {c}: {n_p} predictions and {n_g} ground truths; the device path takes "
                                 f"at most {GROUP_CAP} of each per image and class (device=None has no cap)")
            if n_p:
                p_sel = p_sel[np.argsort(pr_scores[p_sel])[::-1]]         # compute_3d_matches' order, ties included
            p0, g0 = pred_off[-1], gt_off[-1]
            acc["pred_RT"].append(pr_RTs[p_sel]); acc["pred_sc"].append(pr_scales[p_sel]); acc["pred_score"].append(pr_scores[p_sel])
            acc["pred_img"].append(np.full(n_p, img)); acc["pred_inst"].append(p_sel); acc["pred_cls"].append(np.full(n_p, c))
            acc["pred_g0"].append(np.full(n_p, g0))
            acc["gt_RT"].append(gt_RTs[g_sel]); acc["gt_sc"].append(gt_scales[g_sel]); acc["gt_sym"].append(gt_sym[g_sel] != 0)
            acc["gt_img"].append(np.full(n_g, img)); acc["gt_inst"].append(g_sel); acc["gt_cls"].append(np.full(n_g, c))
            acc["gt_p0"].append(np.full(n_g, p0))
            if n_p and n_g:
                gi = np.tile(np.arange(n_g), n_p)
                acc["pairs"].append(np.stack([p0 + np.repeat(np.arange(n_p), n_g), g0 + gi], -1))
                acc["sweep"].append((gt_sym[g_sel] != 0)[gi])
            pair_off.append(n_pairs)
            n_pairs += n_p * n_g
            pred_off.append(p0 + n_p)
            gt_off.append(g0 + n_g)

    def cat(key, dtype, tail):
        parts = acc[key]
        return (np.concatenate(parts) if parts else np.zeros((0,) + tail)).astype(dtype).reshape((-1,) + tail)

    flat = dict(pred_RT=cat("pred_RT", np.float64, (4, 4)), pred_sc=cat("pred_sc", np.float64, (3,)),
                pred_score=cat("pred_score", np.float64, ()),
                gt_RT=cat("gt_RT", np.float64, (4, 4)), gt_sc=cat("gt_sc", np.float64, (3,)), gt_sym=cat("gt_sym", np.int32, ()),
                pairs=cat("pairs", np.int32, (2,)), sweep=cat("sweep", np.int32, ()),
                pred_off=np.asarray(pred_off, np.int32), gt_off=np.asarray(gt_off, np.int32), pair_off=np.asarray(pair_off, np.int64))
    for key in ("pred_img", "pred_inst", "pred_cls", "pred_g0", "gt_img", "gt_inst", "gt_cls", "gt_p0"):
        flat[key] = cat(key, np.int64, ())
    return flat


def _match_tables_on_device(flat, iou_cmp, deg_list, sh_list, keep_row, dev):
    """one upload, cppf_pose_eval_pairs / _match_iou / _match_pose, one read-back: (iou_pm [T,P], iou_gm [T,G], pose_pm [D,S,P],
    pose_gm [D,S,G]) int32 with group-local indices; keep_row: the IoU threshold row whose matches select the instances scored
    for pose (read by the third kernel where the second wrote it), or None"""
    import torch
    from ._torch_util import call, require_cuda
    require_cuda()
    P, G, M, n_groups = len(flat["pred_RT"]), len(flat["gt_RT"]), len(flat["pairs"]), len(flat["pair_off"])
    nT, nD, nS = len(iou_cmp), len(deg_list), len(sh_list)
    parts = [("pred_RT", flat["pred_RT"]), ("pred_sc", flat["pred_sc"]), ("gt_RT", flat["gt_RT"]), ("gt_sc", flat["gt_sc"]),
             ("iou_thr", np.asarray(iou_cmp, np.float64)), ("deg_thr", np.asarray(deg_list, np.float64)),
             ("sh_thr", np.asarray(sh_list, np.float64)), ("pair_off", flat["pair_off"]), ("gt_sym", flat["gt_sym"]),
             ("pairs", flat["pairs"]), ("sweep", flat["sweep"]), ("pred_off", flat["pred_off"]), ("gt_off", flat["gt_off"])]
    chunks, where, pos = [], {}, 0
    for name, arr in parts:                                  # one byte buffer, every section 8-byte aligned
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        pad = (-len(raw)) % 8
        where[name] = (pos, len(raw), arr.dtype, arr.shape)
        chunks += [raw, np.zeros(pad, np.uint8)]
        pos += len(raw) + pad
    buf = torch.from_numpy(np.concatenate(chunks)).to(dev)   # the one upload

    def sec(name):
        o, n, dt, shape = where[name]
        return buf[o:o + n].view(getattr(torch, np.dtype(dt).name)).reshape(shape)

    tables = torch.empty((nT + nD * nS) * (P + G), dtype=torch.int32, device=dev)
    iou_pm, iou_gm = tables[:nT * P].view(nT, P), tables[nT * P:nT * (P + G)].view(nT, G)
    rest = tables[nT * (P + G):]
    pose_pm, pose_gm = rest[:nD * nS * P].view(nD, nS, P), rest[nD * nS * P:].view(nD, nS, G)
    if n_groups:
        iou, err = _pairs_on_device(dev, sec("pred_RT"), sec("pred_sc"), sec("gt_RT"), sec("gt_sc"), sec("gt_sym"), sec("pairs"),
                                    sec("sweep"))
        nul = lambda t_: t_ if t_.numel() else None
        call("cppf_pose_eval_match_iou", dev, nul(iou), sec("pred_off"), sec("gt_off"), sec("pair_off"), n_groups, sec("iou_thr"), nT,
             P, G, M, nul(iou_pm), nul(iou_gm))
        keep_p = nul(iou_pm[keep_row]) if keep_row is not None else None
        keep_g = nul(iou_gm[keep_row]) if keep_row is not None else None
        call("cppf_pose_eval_match_pose", dev, nul(err), sec("pred_off"), sec("gt_off"), sec("pair_off"), n_groups, sec("deg_thr"), nD,
             sec("sh_thr"), nS, keep_p, keep_g, P, G, M, nul(pose_pm), nul(pose_gm))
    host = tables.cpu().numpy()                              # the one read-back
    a, b = nT * P, nT * (P + G)
    c = b + nD * nS * P
    return host[:a].reshape(nT, P), host[a:b].reshape(nT, G), host[b:c].reshape(nD, nS, P), host[c:].reshape(nD, nS, G)


def _map_on_device(final_results, synset_names, log_dir, degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres,
                   use_matches_for_pose, device):
    """compute_degree_cm_mAP with the per-pair work and the matchings on `device`.  Differences from the host path, all refusals:
    a pose or scale that is not finite, a singular rotation block or a last row other than [0 0 0 1] raises ValueError naming the
    image and the instance before anything is uploaded, and so does an (image, class) group of more than GROUP_CAP predictions or
    ground truths.  Among ground truths of EQUAL IoU (or equal degree + cm sum) the device takes the higher (lower) index
    (include/cppf.h); the host's choice there is np.argsort's."""
    import torch
    n_cls = len(synset_names)
    deg_list = list(degree_thresholds) + [360]
    sh_list = list(shift_thresholds) + [100]
    iou_list = list(iou_3d_thresholds)
    nD, nS, nT = len(deg_list), len(sh_list), len(iou_list)
    if use_matches_for_pose and iou_pose_thres not in iou_list:
        raise ValueError("iou_pose_thres must be one of iou_3d_thresholds")
    keep_row = iou_list.index(iou_pose_thres) if use_matches_for_pose else None
    flat = _flatten_results(final_results, n_cls)
    iou_pm, iou_gm, pose_pm, pose_gm = _match_tables_on_device(
        flat, [_iou_threshold_as_compared(t) for t in iou_list], [float(d) for d in deg_list], [float(s) for s in sh_list], keep_row,
        torch.device(device))

    P, G = len(flat["pred_RT"]), len(flat["gt_RT"])
    keep_p = iou_pm[keep_row] > -1 if use_matches_for_pose else np.ones(P, bool)
    keep_g = iou_gm[keep_row] > -1 if use_matches_for_pose else np.ones(G, bool)
    # per-image tables in the image's own instance numbering
    pose_gt_matches = np.full((nD, nS, len(final_results), 20), -1, dtype=int)
    pose_pred_matches = np.full((nD, nS, len(final_results), 20), -1, dtype=int)
    if P:
        m = pose_pm[:, :, keep_p].astype(np.int64)
        to = flat["gt_inst"][np.clip(flat["pred_g0"][keep_p][None, None] + np.maximum(m, 0), 0, max(G - 1, 0))] if G else m
        pose_pred_matches[:, :, flat["pred_img"][keep_p], flat["pred_inst"][keep_p]] = np.where(m >= 0, to, -1)
    if G:
        m = pose_gm[:, :, keep_g].astype(np.int64)
        to = flat["pred_inst"][np.clip(flat["gt_p0"][keep_g][None, None] + np.maximum(m, 0), 0, max(P - 1, 0))] if P else m
        pose_gt_matches[:, :, flat["gt_img"][keep_g], flat["gt_inst"][keep_g]] = np.where(m >= 0, to, -1)

    iou_3d_aps = np.zeros((n_cls + 1, nT))
    pose_aps = np.zeros((n_cls + 1, nD, nS))
    scores = flat["pred_score"]
    for c in range(1, n_cls):
        pc, gc = flat["pred_cls"] == c, flat["gt_cls"] == c
        for s in range(nT):
            iou_3d_aps[c, s] = compute_ap_from_matches_scores(iou_pm[s][pc], scores[pc], iou_gm[s][gc])
        pk, gk = pc & keep_p, gc & keep_g
        for d in range(nD):
            for s in range(nS):
                pose_aps[c, d, s] = compute_ap_from_matches_scores(pose_pm[d, s][pk], scores[pk], pose_gm[d, s][gk])
    iou_3d_aps[-1] = iou_3d_aps[1:-1].mean(0)
    pose_aps[-1] = pose_aps[1:-1].mean(0)
    if log_dir:
        _write_tables(log_dir, iou_list, deg_list, sh_list, iou_3d_aps, pose_aps, use_matches_for_pose)
    return iou_3d_aps, pose_aps, pose_pred_matches, pose_gt_matches


# ------------------------------------------------------------------------------------------------ sunrgbd/eval.py: 3D NMS
NMS_GROUP_CAP = 1024      # boxes of one group on the device: include/cppf.h CPPF_BOX_NMS_GROUP_CAP


def _nms_valid(RTs, scales, scores):
    """the boxes NMS takes: everything finite (sunrgbd/eval.py:121), the last row [0 0 0 1] and a regular rotation block
    (_check_poses' criteria), every extent positive"""
    n = len(RTs)
    if n == 0:
        return np.zeros(0, bool)
    ok = np.isfinite(RTs).all((1, 2)) & np.isfinite(scales).all(1) & np.isfinite(scores)
    ok &= (RTs[:, 3] == np.array([0.0, 0.0, 0.0, 1.0])).all(1)
    safe = np.where(ok[:, None, None], RTs, np.eye(4)[None])
    det = np.linalg.det(safe[:, :3, :3])
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        ok &= (np.abs(det) > 1e-12 * np.linalg.norm(safe[:, :3, :3], axis=1).prod(1)) & np.isfinite(1.0 / det)
        ok &= (scales > 0).all(1)
    return ok


def _nms_greedy_host(RTs, scales, scores, thresh):
    """sunrgbd/eval.py:21-35 on one group: indices in pick order.  Ties: the higher index first (a stable ascending argsort read
    from the end); an IoU that is NaN suppresses nothing."""
    order = np.argsort(scores, kind="stable")[::-1]
    alive = np.ones(len(order), bool)
    pick = []
    for a, i in enumerate(order):
        if not alive[a]:
            continue
        pick.append(int(i))
        for b in range(a + 1, len(order)):
            if alive[b]:
                j = order[b]
                lo, hi = (i, j) if i < j else (j, i)             # the pair as the device forms it: the lower index is box 1
                if compute_3d_iou(RTs[lo], RTs[hi], scales[lo], scales[hi], False, None, None) > thresh:
                    alive[b] = False
    return np.asarray(pick, dtype=np.int64)


def _nms_on_device(dev, RTs, scales, scores, group_off, thresh):
    """cppf_box_nms_batch on host arrays already in group order: one upload, one call, one read-back -> (pick i32[n], n_pick i32[G])"""
    import torch
    from . import _lib
    from ._torch_util import call, require_cuda, scratch, workspace
    require_cuda()
    dev = torch.device(dev)
    n, G = len(RTs), len(group_off) - 1
    if n == 0 or G == 0:
        return np.zeros(0, np.int32), np.zeros(G, np.int32)
    buf = torch.from_numpy(np.concatenate([RTs.reshape(-1), scales.reshape(-1), scores.reshape(-1)]).astype(np.float64)).to(dev)
    res = torch.empty(n + G, dtype=torch.int32, device=dev)
    ws = workspace(_lib.lib().cppf_box_nms_workspace_bytes(n, G), dev, "box_nms")
    call("cppf_box_nms_batch", dev, buf[:16 * n], buf[16 * n:19 * n], buf[19 * n:], n, np.ascontiguousarray(group_off, np.int32), G,
         float(thresh), res[:n], res[n:], None, scratch(ws))
    out = res.cpu().numpy()                                      # the one read-back
    return out[:n], out[n:]


def nms_3d(RTs, scales, scores, thresh=0.3, groups=None, device=None):
    """Greedy 3D non-maximum suppression over oriented boxes (sunrgbd/eval.py:13-35): within a group the boxes are visited by
    descending score, a box that is not suppressed is picked and suppresses every later box whose IoU with it is strictly greater
    than `thresh`.  The IoU is compute_3d_iou(RT_i, RT_j, scales_i, scales_j, up_sym=False, ...) with the lower index as box 1: the
    rotation block may carry an isotropic scale (normalised by cbrt(det)), `scales` are the extents along the normalised axes.

    RTs [n,4,4], scales [n,3], scores [n]; groups: None (one group) or int [n], the group of every box, 0 <= id (e.g. one id per
    (image, class)).  Returns a list of int64 index arrays in pick order, one per group (max id + 1 of them; [one] for None); the
    indices refer to the arguments as given.
    Dropped before anything else, and never picked: a box with a non-finite RT, scale or score (sunrgbd/eval.py:121), with a last
    row other than [0 0 0 1] or a singular rotation block (_check_poses), or with a non-positive extent.
    Equal scores: the higher index goes first (a stable ascending argsort read from the end; the reference's np.argsort leaves ties
    open).  A NaN IoU suppresses nothing.
    device=None: numpy, the checker.  A HIP device: one cppf_box_nms_batch call for all groups and one read-back (csrc/box_nms.hip;
    at most NMS_GROUP_CAP valid boxes per group there)."""
    RTs = np.asarray(RTs, dtype=np.float64).reshape(-1, 4, 4)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1, 3)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    n = len(RTs)
    if len(scales) != n or len(scores) != n:
        raise ValueError(f"nms_3d: {n} poses, {len(scales)} scales and {len(scores)} scores")
    if groups is None:
        gid, G = np.zeros(n, np.int64), 1
    else:
        gid = np.asarray(groups).astype(np.int64).reshape(-1)
        if len(gid) != n or (n and gid.min() < 0):
            raise ValueError("nms_3d: groups holds one non-negative id per box")
        G = int(gid.max()) + 1 if n else 0
    valid = np.where(_nms_valid(RTs, scales, scores))[0]
    sel = valid[np.argsort(gid[valid], kind="stable")]           # group order; a group's boxes stay in index order
    group_off = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(gid[sel], minlength=G), out=group_off[1:])
    if device is None:
        return [sel[a:b][_nms_greedy_host(RTs[sel[a:b]], scales[sel[a:b]], scores[sel[a:b]], thresh)] if b > a else np.zeros(0, np.int64)
                for a, b in zip(group_off[:-1], group_off[1:])]
    if G and np.diff(group_off).max() > NMS_GROUP_CAP:
        raise ValueError(f"nms_3d: a group of {int(np.diff(group_off).max())} boxes; the device path takes at most {NMS_GROUP_CAP} per "
                         "group (device=None has no cap)")
    pick, n_pick = _nms_on_device(device, RTs[sel], scales[sel], scores[sel], group_off, thresh)
    return [sel[a:b][pick[a:a + k]].astype(np.int64) for a, b, k in zip(group_off[:-1], group_off[1:], n_pick)]


_NMS_PRED_KEYS = ("pred_class_ids", "pred_RTs", "pred_scales", "pred_scores", "pred_bboxes")


def nms_results(final_results, thresh=0.3, device=None):
    """sunrgbd/eval.py:110-145 for a list of result dicts in compute_degree_cm_mAP's format: every image's predictions go through
    nms_3d class by class; the kept ones are written class by class (ascending id), each class in pick order, with pred_class_ids,
    pred_RTs, pred_scales, pred_scores and -- where present -- pred_bboxes kept in step.  The boxes are the ones the metric scores:
    extents pred_scales * cbrt(det pred_RTs[:3,:3]) (_unit_scale).  All (image, class) groups of the list are one nms_3d call (one
    device call when `device` is given).  Returns new dicts (the other keys shared); the input is not modified."""
    RTs, scales, scores, gid, where = [], [], [], [], []
    n_groups = 0
    for img, res in enumerate(final_results):
        cls = np.asarray(res["pred_class_ids"]).reshape(-1)
        k = len(cls)
        if k == 0:
            continue
        rt = np.asarray(res["pred_RTs"], dtype=np.float64).reshape(-1, 4, 4)
        sc = np.asarray(res["pred_scales"], dtype=np.float64).reshape(-1, 3)
        s = np.asarray(res["pred_scores"], dtype=np.float64).reshape(-1)
        if len(rt) != k or len(sc) != k or len(s) != k:
            raise ValueError(f"image {img}: one class id, pose, scale and score per prediction")
        with np.errstate(invalid="ignore"):
            sc = sc * np.cbrt(np.linalg.det(np.where(np.isfinite(rt), rt, 0.0)[:, :3, :3]))[:, None]
        classes, inv = np.unique(cls, return_inverse=True)
        RTs.append(rt); scales.append(sc); scores.append(s); gid.append(n_groups + inv.reshape(-1))
        where.append((img, len(classes)))
        n_groups += len(classes)
    picks = []
    if RTs:
        picks = nms_3d(np.concatenate(RTs), np.concatenate(scales), np.concatenate(scores), thresh, np.concatenate(gid), device)
    out = [dict(res) for res in final_results]
    g, first = 0, 0
    for img, n_cls in where:
        res = final_results[img]
        keep = np.concatenate([picks[g + c] for c in range(n_cls)]).astype(np.int64) - first
        for key in _NMS_PRED_KEYS:
            if key in res:
                out[img][key] = np.asarray(res[key])[keep]
        g += n_cls
        first += len(np.asarray(res["pred_class_ids"]).reshape(-1))
    return out


# ------------------------------------------------------------------------------------------------ nocs/eval.py
def mark_up_symmetry(result, synset_names=SYNSET_NAMES):
    """nocs/eval.py:25-33: gt_up_syms from the class and the handle visibility (a mug whose handle is hidden counts as
    symmetric about its up axis)"""
    vis, cls = np.asarray(result["gt_handle_visibility"]), np.asarray(result["gt_class_ids"])
    if len(vis) != len(cls):
        raise ValueError(f"{len(vis)} handle flags for {len(cls)} instances")
    sym = np.zeros(len(cls), dtype=bool)
    for i, (c, v) in enumerate(zip(cls, vis)):
        name = synset_names[c]
        if v == 0:
            if name != "mug":
                raise ValueError(f"hidden handle on a {name}")
            sym[i] = True
        elif name in _UP_SYMMETRIC:
            sym[i] = True
    result["gt_up_syms"] = sym
    return result


def evaluate_prediction_dir(pred_dir, stride=10, synset_names=SYNSET_NAMES, device=None):
    """nocs/eval.py:16-49: every `stride`-th results_*.pkl of a prediction directory -> the four arrays of
    compute_degree_cm_mAP with the thresholds the paper reports (5/10/15 degrees, 5/10/15 cm, IoU 0..1 in steps of 0.01);
    `device` as there."""
    import glob
    files = sorted(glob.glob(os.path.join(pred_dir, "results_*.pkl")))[::stride]
    if not files:
        raise FileNotFoundError(f"no results_*.pkl under {pred_dir}")
    results = []
    for path in files:
        with open(path, "rb") as f:
            r = pickle.load(f)
        for one in (r if isinstance(r, list) else [r]):
            results.append(mark_up_symmetry(one, synset_names))
    return compute_degree_cm_mAP(results, synset_names, pred_dir + "_map", degree_thresholds=[5, 10, 15],
                                 shift_thresholds=[5, 10, 15], iou_3d_thresholds=np.linspace(0, 1, 101), iou_pose_thres=0.1,
                                 use_matches_for_pose=True, device=device)
