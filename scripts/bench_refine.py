#!/usr/bin/env python3
"""The refinement stage of the mask-free path, measured on the demo frame's dense cloud (tests/golden/demo_0000_depth.png):

  gather     cppf_gather_instances (scene_stage.gather_instances_device: two launches for all K proposals, nothing read back)
             against K boolean-index gathers in torch, hi[m_k] and hi_nrm[m_k] -- once with the membership m_k = masks[k][owner]
             computed inside the timed region (what the kernel also does), once with m_k prepared beforehand (the gathers alone).
             K = 1 / 8 / 32 ball-shaped proposals over the sparse cloud.  Both routes in one process, alternating repetition by
             repetition, HIP events around each, outputs compared first, medians with the inter-quartile range.  The new route counts
             as faster only where the baseline's median exceeds its median by more than the baseline's IQR (DESIGN.md 3.7e's rule).
  frame      wall time (host clock around a device synchronise) of scene_frame and of refine_poses on its output, per frame.

    python scripts/bench_refine.py [--reps 200] [--out profiles/refine.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf_amd import scene_poses, scene_stage, training       # noqa: E402
from cppf_amd.batch import BatchPoseRunner                     # noqa: E402
from cppf_amd.config import CATEGORIES                         # noqa: E402
from cppf_amd.frames import NOCS_INTRINSICS                    # noqa: E402
from cppf_amd.utils.util import read_depth_png  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def ball_masks(pc, K, radius, seed):
    """u8[K,N]: proposal k owns the sparse points within `radius` of a sparse point drawn at random"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = pc[torch.randint(0, pc.shape[0], (K,), generator=g).to(pc.device)]
    return (torch.cdist(centres, pc) <= radius).to(torch.uint8).contiguous()


def torch_route(hi, hi_nrm, owner_l, has, masks, members=None):
    out = []
    for k in range(masks.shape[0]):
        m = (masks[k][owner_l] != 0) & has if members is None else members[k]
        out.append((hi[m], hi_nrm[m]))
    return out


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


def gather_rows(hi, hi_nrm, ind, owner, reps, radius):
    pc = hi[ind].contiguous()
    owner_l, has = owner.long().clamp(min=0), owner >= 0
    rows = []
    for K in (1, 8, 32):
        masks = ball_masks(pc, K, radius, seed=K)
        members = [(masks[k][owner_l] != 0) & has for k in range(K)]
        total = int(sum(int(m.sum()) for m in members))
        bufs = scene_stage.gather_instances_device(hi, hi_nrm, owner, masks, capacity=max(total, 1))
        new = lambda: scene_stage.gather_instances_device(hi, hi_nrm, owner, masks, capacity=max(total, 1), out=bufs)
        base_full = lambda: torch_route(hi, hi_nrm, owner_l, has, masks)
        base_gather = lambda: torch_route(hi, hi_nrm, owner_l, has, masks, members)
        # outputs first: the packed rows equal the K gathers, bit for bit
        new()
        off = bufs["offsets"].cpu().numpy()
        assert int(off[K]) == total
        for k, (p, n) in enumerate(base_full()):
            assert torch.equal(bufs["pts"][off[k]:off[k + 1]], p) and torch.equal(bufs["nrm"][off[k]:off[k + 1]], n), k
        for _ in range(10):                                                   # warm-up of every route
            new(), base_full(), base_gather()
        t = dict(new=[], torch_with_membership=[], torch_gathers_only=[])
        for _ in range(reps):                                                 # alternating, repetition by repetition
            t["new"].append(timed(new))
            t["torch_with_membership"].append(timed(base_full))
            t["torch_gathers_only"].append(timed(base_gather))
        row = dict(K=K, dense_points=int(hi.shape[0]), sparse_points=int(pc.shape[0]), gathered_rows=total, reps=reps,
                   **{k: quartiles(v) for k, v in t.items()})
        for base in ("torch_with_membership", "torch_gathers_only"):
            row["faster_than_" + base] = bool(row[base]["median_us"] - row["new"]["median_us"] > row[base]["iqr_us"])
        rows.append(row)
        print(json.dumps(row))
    return rows


def frame_rows(depth, dev, frames, n_pairs, min_contrib):
    rows = []
    for cat in ("bottle", "mug"):
        cfg = CATEGORIES[cat]
        penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
        runner = BatchPoseRunner({cat: enc}, dev, point_encoders={cat: penc})
        t_scene, t_refine, n_ref, n_pts = [], [], 0, 0
        for i in range(frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, n_pairs=n_pairs, seed=0, thresh=5.0, max_proposals=4,
                                          min_contrib=min_contrib, keep_masks=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            refined = scene_poses.refine_poses(out, runner, cfg, seed=0)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_scene.append((t1 - t0) * 1e3), t_refine.append((t2 - t1) * 1e3)
            n_ref = sum(r is not None for r in refined)
            n_pts = sum(r["n_points"] for r in refined if r is not None)
        steady = slice(min(3, frames - 1), None)                              # the first frames capture the runner's pipelines
        row = dict(category=cat, frames=frames, scene_pairs=n_pairs, min_contrib=min_contrib, proposals=len(out["poses"]), refined=n_ref,
                   refined_points=n_pts, scene_frame_ms_median=float(np.median(t_scene[steady])),
                   refine_poses_ms_median=float(np.median(t_refine[steady])), refine_poses_ms_first=float(t_refine[0]))
        rows.append(row)
        print(json.dumps(row))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--scene-pairs", type=int, default=1_000_000)
    ap.add_argument("--radius", type=float, default=0.08, help="radius of the ball-shaped proposals of the gather rows, metres")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_refine.py measures on a HIP device: none found")
    dev = torch.device("cuda", 0)
    depth = read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))
    cfg = CATEGORIES["bottle"]
    cloud = scene_stage.frame_cloud(depth, NOCS_INTRINSICS, cfg)
    hi, hi_nrm, ind = cloud.hi, cloud.hi_nrm, cloud.ind
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    owner = scene_stage.voxel_owner(hi, ind, 4 * cfg.res)
    torch.cuda.synchronize()
    owner_ms = (time.perf_counter() - t0) * 1e3
    rec = dict(device=torch.cuda.get_device_name(0), depth_image="tests/golden/demo_0000_depth.png", res=cfg.res, voxel_owner_ms_first_call=owner_ms,
               rule="new counts as faster where the baseline's median exceeds its median by more than the baseline's IQR",
               gather=gather_rows(hi, hi_nrm, ind, owner, args.reps, args.radius),
               frame=frame_rows(depth, dev, args.frames, args.scene_pairs, 12) + frame_rows(depth, dev, args.frames, args.scene_pairs, 2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
