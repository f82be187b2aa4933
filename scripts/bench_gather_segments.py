#!/usr/bin/env python3
"""cppf_gather_segments measured on the demo frame's dense cloud (tests/golden/demo_0000_depth.png), for S = 4 / 32 / 256 / 1024
segments -- the points labelled by the cell of a gx x gy grid over the image plane that they project into, so that labels are as
coherent along the cloud's pixel order as real segments are:

  new              segments.segment_clouds_device: one call (four launches) for all S segments, bounds included, nothing read back
  one_hot_passes   ceil(S / 32) calls of cppf_gather_instances with owner = labels and 32 one-hot mask rows each (the masks prepared
                   beforehand: their S x S upload is NOT in the timed region)
  torch_loop       S times hi[labels == s] and hi_nrm[labels == s] in torch

All routes in one process, alternating repetition by repetition, HIP events around each, outputs compared first, medians of --reps
calls after a warm-up with the inter-quartile range.  The new route counts as faster only where the baseline's median exceeds its
median by more than the baseline's IQR (DESIGN.md 3.1a's rule).

    python scripts/bench_gather_segments.py [--reps 200] [--out profiles/gather_segments.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf_amd import scene_stage, segments                     # noqa: E402
from cppf_amd.config import CATEGORIES                         # noqa: E402
from cppf_amd.frames import NOCS_INTRINSICS                    # noqa: E402
from cppf_amd.utils.util import read_depth_png                 # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GRIDS = {4: (2, 2), 32: (8, 4), 256: (16, 16), 1024: (32, 32)}


def grid_labels(hi, gx, gy):
    """i32[M]: the cell of a gx x gy grid over the bounding rectangle of the points' projections (x / z, y / z)"""
    u, v = hi[:, 0] / hi[:, 2], hi[:, 1] / hi[:, 2]
    cell = lambda t, n: ((t - t.min()) / (t.max() - t.min()).clamp(min=1e-12) * n).floor().clamp(0, n - 1).long()
    return (cell(v, gy) * gx + cell(u, gx)).to(torch.int32).contiguous()


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms, np.float64), [25, 50, 75])
    return dict(median_us=float(med * 1e3), iqr_us=float((q3 - q1) * 1e3), q1_us=float(q1 * 1e3), q3_us=float(q3 * 1e3))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rows(cloud, reps, warmup):
    hi, hi_nrm = cloud.hi, cloud.hi_nrm
    M, dev = hi.shape[0], hi.device
    out = []
    for S, (gx, gy) in GRIDS.items():
        lab = grid_labels(hi, gx, gy)
        labelled = cloud._replace(hi_labels=lab)
        bufs = segments.segment_clouds_device(labelled, S)
        new = lambda: segments.segment_clouds_device(labelled, S, out=bufs)
        groups = [torch.zeros((min(32, S - g), S), dtype=torch.uint8, device=dev) for g in range(0, S, 32)]
        for j, m in enumerate(groups):
            m[torch.arange(m.shape[0]), 32 * j + torch.arange(m.shape[0])] = 1
        old_bufs = [scene_stage.gather_instances_device(hi, hi_nrm, lab, m) for m in groups]

        def one_hot():
            for m, b in zip(groups, old_bufs):
                scene_stage.gather_instances_device(hi, hi_nrm, lab, m, out=b)

        def torch_loop():
            return [(hi[lab == s], hi_nrm[lab == s]) for s in range(S)]
        # outputs first: the packed rows equal both baselines, bit for bit
        new(), one_hot()
        off = bufs["offsets"].cpu().numpy()
        assert int(off[S]) == M
        for s, (p, n) in enumerate(torch_loop()):
            assert torch.equal(bufs["pts"][off[s]:off[s + 1]], p) and torch.equal(bufs["nrm"][off[s]:off[s + 1]], n), s
        for j, b in enumerate(old_bufs):
            o = b["offsets"].cpu().numpy()
            a0 = int(off[32 * j])
            assert np.array_equal(o, off[32 * j:32 * j + len(o)] - a0) and torch.equal(b["pts"][:o[-1]], bufs["pts"][a0:a0 + o[-1]]), j
        for _ in range(warmup):
            new(), one_hot(), torch_loop()
        t = dict(new=[], one_hot_passes=[], torch_loop=[])
        for _ in range(reps):                                                 # alternating, repetition by repetition
            t["new"].append(timed(new))
            t["one_hot_passes"].append(timed(one_hot))
            t["torch_loop"].append(timed(torch_loop))
        row = dict(S=S, grid=[gx, gy], dense_points=int(M), segments_with_points=int((np.diff(off) > 0).sum()), passes=len(groups), reps=reps,
                   **{k: quartiles(v) for k, v in t.items()})
        for base in ("one_hot_passes", "torch_loop"):
            row["faster_than_" + base] = bool(row[base]["median_us"] - row["new"]["median_us"] > row[base]["iqr_us"])
        out.append(row)
        print(json.dumps(row))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_segments.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gather_segments.py measures on a HIP device: none found")
    depth = read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))
    cfg = CATEGORIES["bottle"]
    cloud = scene_stage.frame_cloud(depth, NOCS_INTRINSICS, cfg)
    rec = dict(device=torch.cuda.get_device_name(0), depth_image="tests/golden/demo_0000_depth.png", res=cfg.res,
               rule="new counts as faster where the baseline's median exceeds its median by more than the baseline's IQR",
               labels="the cell of a gx x gy grid over the image plane that a point projects into; every point has a label",
               note="one_hot_passes: the one-hot masks are prepared outside the timed region; new writes the bounds as well",
               gather=rows(cloud, args.reps, args.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
