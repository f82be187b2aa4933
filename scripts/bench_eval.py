#!/usr/bin/env python3
"""Time of the NOCS metric (cppf_amd.evaluation.compute_degree_cm_mAP with nocs/eval.py's thresholds) on a seeded synthetic result
set of REAL275's size (cppf_amd.synthetic.make_eval_results): the device path (csrc/pose_eval.hip) on all of it -- the whole call,
and its device part alone -- and the host path on every tenth image.  Checks that both paths give the same tables on that subset
and prints one JSON line.

    python scripts/bench_eval.py --images 2750 --reps 3
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf_amd import evaluation as E                     # noqa: E402
from cppf_amd.synthetic import make_eval_results         # noqa: E402

KW = dict(degree_thresholds=[5, 10, 15], shift_thresholds=[5, 10, 15], iou_3d_thresholds=np.linspace(0, 1, 101), iou_pose_thres=0.1,
          use_matches_for_pose=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2750, help="REAL275's test split has 2 754 images")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host-stride", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = [E.mark_up_symmetry(r) for r in make_eval_results(args.images, args.seed)]
    subset = results[::args.host_stride]
    E.compute_degree_cm_mAP(copy.deepcopy(subset), E.SYNSET_NAMES, None, device=dev, **KW)      # warm-up: library load, allocations
    torch.cuda.synchronize()
    whole = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out_dev = E.compute_degree_cm_mAP(results, E.SYNSET_NAMES, None, device=dev, **KW)
        whole.append(time.perf_counter() - t0)
    # the device part alone: upload, three launches, read-back
    flat = E._flatten_results(results, len(E.SYNSET_NAMES))
    thr = [E._iou_threshold_as_compared(t) for t in KW["iou_3d_thresholds"]]
    part = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E._match_tables_on_device(flat, thr, [5.0, 10.0, 15.0, 360.0], [5.0, 10.0, 15.0, 100.0], 10, dev)
        part.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    host = E.compute_degree_cm_mAP(copy.deepcopy(subset), E.SYNSET_NAMES, None, **KW)
    host_s = time.perf_counter() - t0
    sub_dev = E.compute_degree_cm_mAP(copy.deepcopy(subset), E.SYNSET_NAMES, None, device=dev, **KW)
    equal = bool(np.allclose(sub_dev[0], host[0], atol=1e-12, rtol=0) and np.allclose(sub_dev[1], host[1], atol=1e-12, rtol=0)
                 and np.array_equal(sub_dev[2], host[2]) and np.array_equal(sub_dev[3], host[3]))
    n_pairs, n_items = len(flat["pairs"]), int((flat["sweep"] != 0).sum() * 19 + len(flat["pairs"]))
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), images=len(results), box_pairs=n_pairs, clip_problems=n_items,
                          device_ms_per_image=1e3 * min(whole) / len(results), device_part_ms_per_image=1e3 * min(part[1:]) / len(results),
                          device_total_s=min(whole), device_part_s=min(part[1:]), host_images=len(subset),
                          host_ms_per_image=1e3 * host_s / len(subset), host_total_s=host_s, tables_equal_on_subset=equal,
                          mean_iou_ap_25_50_75=[float(out_dev[0][-1, k]) for k in (25, 50, 75)])))
    if not equal:
        sys.exit("the device tables differ from the host's on the subset")


if __name__ == "__main__":
    main()
