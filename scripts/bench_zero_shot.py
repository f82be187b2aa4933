#!/usr/bin/env python3
"""Per-stage device times of the zero-shot scene path (cppf_amd/zero_shot.py) on the demo frame (tests/golden/demo_0000_depth.png,
res 4e-3: a ~321 x 222 x 164 grid), against the host scipy / numpy the notebook runs for cells 9 and 11.

    python scripts/bench_zero_shot.py [--pairs 5000000] [--reps 10]

The regression head is a seeded network whose last layer answers nearly the same (mu, nu) for every pair (no trained weights
exist here): the votes pile up and the proposal loop has peaks to work on.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cppf_amd import zero_shot  # noqa: E402
from cppf_amd.config import CATEGORIES  # noqa: E402
from cppf_amd.frames import NOCS_INTRINSICS  # noqa: E402
from cppf_amd.models.model import PointEncoder, PPFEncoder  # noqa: E402
from cppf_amd.utils.util import read_depth_png  # noqa: E402


def dev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_ms(fn, reps):
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = CATEGORIES["bowl"]
    torch.manual_seed(0)
    enc = PPFEncoder([84, 32, 32, 16], 9)
    with torch.no_grad():
        enc.final.weight.mul_(1e-3)
        enc.final.bias.copy_(torch.tensor([0.0, 0.02, 1.0, 1.5, 0.5, 0.0, 0.0, 0.0, 0.0]))
    enc = enc.to(dev).eval()
    penc = PointEncoder(k=cfg.knn, spfcs=[32, 64, 32, 32], out_dim=32, num_layers=1).to(dev).eval()
    depth = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    t0 = time.perf_counter()
    out = zero_shot.zero_shot_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, n_pairs=args.pairs, seed=0)
    torch.cuda.synchronize()
    frame_ms = (time.perf_counter() - t0) * 1e3
    grid, dims = out["grid"], out["dims"]
    ws = zero_shot.proposals_workspace(dims, dev)
    r = {"dims": list(dims), "n_points_hi": int(out["hi_pc"].shape[0]), "n_points": int(out["pc"].shape[0]),
         "n_pairs": out["n_pairs"], "n_proposals": len(out["poses"]), "frame_wall_ms_first_call": frame_ms}
    r["smooth_device_ms"] = dev_ms(lambda: zero_shot.smooth_grid(grid), args.reps)
    r["proposals_device_ms"] = dev_ms(lambda: zero_shot.scene_proposals_device(grid, ws=ws), args.reps)
    r["scene_tail_wall_ms"] = host_ms(lambda: zero_shot.zero_shot_scene(None, out["pc"], out["normals"], None, out["idx"], cfg,
                                                                        preds=out["preds"]), 3)
    try:
        from scipy.ndimage import gaussian_filter
        g = grid.cpu().numpy()
        r["smooth_host_scipy_ms"] = host_ms(lambda: gaussian_filter(g, sigma=1), 3)
        r["grid_copy_to_host_ms"] = host_ms(lambda: grid.cpu(), 3)
    except ImportError:
        r["smooth_host_scipy_ms"] = "not measured (no scipy)"
    print(json.dumps(r))


if __name__ == "__main__":
    main()
