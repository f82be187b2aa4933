#!/usr/bin/env python3
"""Time of the 3D box NMS (cppf_amd.evaluation.nms_3d / nms_results): the host path (numpy, the checker) against the device path
(csrc/box_nms.hip, one cppf_box_nms_batch call for all groups) at two shapes --

  results   a seeded synthetic result list of REAL275's size (cppf_amd.synthetic.make_eval_results, scripts/bench_eval.py's
            generator) through nms_results: every (image, class) group of the list in one call;
  frame     one pooled frame of 12 categories x 32 proposals through nms_3d: 12 groups of 32 boxes, centres in a 1.5 m cube,
            extents 0.1 .. 0.4 m.

Method: one process; the outputs of both paths are compared first (they must be equal); then the two paths alternate repetition by
repetition, each timed as the whole call (the device path with its upload, its read-back and a synchronisation); medians and
inter-quartile ranges.  Project rule: the device path counts as faster only where the host median exceeds its median by more than
the host's IQR -- otherwise the verdict is "not faster".  Writes profiles/box_nms.json.

    python scripts/bench_nms.py --reps 7
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf_amd import evaluation as E                     # noqa: E402
from cppf_amd.synthetic import make_eval_results, random_rotation         # noqa: E402


def _frame(rng, cats=12, per=32):
    n = cats * per
    RT = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        RT[k, :3, :3] = random_rotation(rng)
    RT[:, :3, 3] = rng.uniform(-0.75, 0.75, (n, 3)) + [0.0, 0.0, 1.5]
    return RT, rng.uniform(0.1, 0.4, (n, 3)), rng.uniform(0.0, 1.0, n), np.repeat(np.arange(cats), per)


def _stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return dict(median_ms=float(med), iqr_ms=float(q3 - q1), reps=len(ms))


def _alternate(host, device, reps):
    th, td = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); host(); th.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); device(); torch.cuda.synchronize(); td.append((time.perf_counter() - t0) * 1e3)
    h, d = _stats(th), _stats(td)
    faster = h["median_ms"] - d["median_ms"] > h["iqr_ms"]
    return dict(host=h, device=d, verdict="device faster" if faster else "not faster")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2750, help="REAL275's test split has 2 754 images")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_nms.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rec = dict(device=torch.cuda.get_device_name(0), thresh=0.3, method="one process, host and device alternating repetition by "
               "repetition, outputs compared first, whole calls timed; device faster only if host median - device median > host IQR")

    results = make_eval_results(args.images, args.seed)
    a, b = E.nms_results(results, 0.3), E.nms_results(results, 0.3, device=dev)        # (also the device path's warm-up)
    same = all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("pred_class_ids", "pred_RTs", "pred_scales", "pred_scores"))
    if not same:
        sys.exit("results: the host and the device path disagree")
    n_pred = sum(len(r["pred_class_ids"]) for r in results)
    groups = sum(len(np.unique(r["pred_class_ids"])) for r in results)
    rec["results"] = dict(images=len(results), predictions=n_pred, groups=groups, kept=sum(len(r["pred_class_ids"]) for r in a),
                          **_alternate(lambda: E.nms_results(results, 0.3), lambda: E.nms_results(results, 0.3, device=dev), args.reps))

    RT, scales, scores, gid = _frame(np.random.default_rng(args.seed))
    a, b = E.nms_3d(RT, scales, scores, 0.3, gid), E.nms_3d(RT, scales, scores, 0.3, gid, device=dev)
    if not all(np.array_equal(x, y) for x, y in zip(a, b)):
        sys.exit("frame: the host and the device path disagree")
    rec["frame"] = dict(categories=12, proposals_per_category=32, kept=int(sum(len(x) for x in a)),
                        **_alternate(lambda: E.nms_3d(RT, scales, scores, 0.3, gid), lambda: E.nms_3d(RT, scales, scores, 0.3, gid, device=dev),
                                     args.reps))
    for shape in ("results", "frame"):
        r = rec[shape]
        print(f"{shape:8s} host {r['host']['median_ms']:9.2f} ms (IQR {r['host']['iqr_ms']:.2f})   device {r['device']['median_ms']:8.2f} ms "
              f"(IQR {r['device']['iqr_ms']:.2f})   {r['verdict']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
