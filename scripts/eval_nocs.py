#!/usr/bin/env python3
"""The role of the reference's nocs/eval.py: score a directory of results_*.pkl files (the layout nocs/inference.py:338-345 writes,
cppf_amd.inference.nocs_result on this side) and print the two mean rows -- 3D-IoU AP at 25 / 50 / 75 %, and the degree /
centimetre AP table.  With --device the box IoUs, the errors and the matchings run on that HIP device (csrc/pose_eval.hip);
without it the host path runs.  The tables are pickled into --log-dir (default: <pred-dir>_map), as the reference does.

    python scripts/eval_nocs.py --pred-dir out/real_test --stride 10 --device cuda:0
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf_amd import evaluation as E       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred-dir", required=True)
    ap.add_argument("--stride", type=int, default=10, help="every stride-th results file (nocs/eval.py:18 uses 10)")
    ap.add_argument("--device", default=None, help="a HIP device such as cuda:0; default: the host path")
    ap.add_argument("--log-dir", default=None, help="where the AP tables are pickled; default <pred-dir>_map")
    args = ap.parse_args()
    t0 = time.perf_counter()
    iou_aps, pose_aps, _, _ = E.evaluate_prediction_dir(args.pred_dir, stride=args.stride, device=args.device)
    if args.log_dir:                            # the same two pickles, where they were asked for
        E._write_tables(args.log_dir, list(np.linspace(0, 1, 101)), [5, 10, 15, 360], [5, 10, 15, 100], iou_aps, pose_aps, True)
    dt = time.perf_counter() - t0
    np.set_printoptions(precision=4, suppress=True)
    print("3D IoU AP at 25 / 50 / 75 % (mean over classes):", iou_aps[-1, [25, 50, 75]])
    print("pose AP, rows 5 / 10 / 15 / 360 degrees, columns 5 / 10 / 15 / 100 cm (mean over classes):")
    print(pose_aps[-1])
    print(f"{dt:.2f} s on {'the host' if args.device is None else args.device}")


if __name__ == "__main__":
    main()
