"""Proposal verification (csrc/verify.hip: cppf_proposal_support + cppf_box_support) timed beside the stage whose
outputs it reads -- cppf_backvote_multi and cppf_segment_instances (csrc/scene_multi.hip) -- in ONE process with HIP events, on the
scene and the shapes of scripts/bench_scene_poses.py: eight bowls with perfect (mu, nu) inside the objects, 500 000 and 5 000 000
pairs, K in {1, 8, 32} proposals on the objects' centres (then moved by two cells per round).

Per row the four routes alternate repetition by repetition after a warm-up, each repetition between its own pair of events (host launch
path included): `backvote` (cppf_backvote_multi), `segment` (cppf_segment_instances), `verify` (both verification kernels, as
scene_stage.verify_proposals enqueues them, without its read-back) and `support` (cppf_proposal_support alone).  Median and
inter-quartile range of the per-repetition times.  Before a row is timed the verification counts are compared with tests/verify_ref.py
(at 500 000 pairs; at 5 000 000 with the pair counts of proposal 0): a row that differs ends the script.

The expectation on record (not a pass mark): the stage reads 12 bytes per pair plus two 4-byte gathers, so `verify` should cost no more
than `segment` at the same shape; `verify_over_segment` is that ratio, and `verify_within_segment` says whether verify's median is at
most segment's plus segment's inter-quartile range.  Also times scene_poses.scene_frame on tests/golden/demo_0000_depth.png with the
committed bottle network with and without verify=True, alternating (wall clock per call, read-backs included).  Writes
profiles/scene_verify.json.  Needs a HIP device; there is no fall-back.

    python scripts/bench_verify.py [--reps 40] [--frame-pairs 5000000] [--out profiles/scene_verify.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import verify_ref as V                                                   # noqa: E402
from bench_precision import stats                                        # noqa: E402
from bench_scene_poses import N_OBJ, N_POINTS, proposal_centers, scene, timed_alternating    # noqa: E402
from cppf_amd import scene_poses, scene_stage, training                   # noqa: E402
from cppf_amd.config import CATEGORIES                                   # noqa: E402
from cppf_amd.inference import grid_shape                                # noqa: E402


def stage_rows(dev, reps):
    rows = []
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for P in (500_000, 5_000_000):
        cfg, pc, idx, out, centers = scene(P)
        corners, dims = grid_shape(pc, cfg.res)
        pcd, idxd, outd, corner = d(pc), d(idx), d(out), d(corners[0])
        N = pc.shape[0]
        ext = pc[:N_POINTS].max(0) - pc[:N_POINTS].min(0)                 # every object is the same bowl up to its seed: one box size
        for K in (1, 8, 32):
            cs = proposal_centers(centers, K, cfg.res)
            csd = d(cs)
            bits = torch.empty(P, dtype=torch.int32, device=dev)
            scene_poses.backvote_multi(pcd, outd, idxd, corner, cfg.res, dims, csd, 72, out=bits)
            masks, _, _ = scene_poses.segment_instances(idxd, bits, N, K, 12)
            poses = [dict(T=c.astype(np.float64), R=np.eye(3), scale=ext.astype(np.float64)) for c in cs]
            boxes = d(scene_stage.verify_boxes(poses, cfg))
            cen, axes, half = boxes[:, 0:3].contiguous(), boxes[:, 3:12].contiguous(), boxes[:, 12:15].contiguous()
            sup = torch.empty((K, 4), dtype=torch.int32, device=dev)
            box = torch.empty((K, 3), dtype=torch.int32, device=dev)

            def backvote():
                scene_poses.backvote_multi(pcd, outd, idxd, corner, cfg.res, dims, csd, 72, out=bits)

            def segment():
                scene_poses.segment_instances(idxd, bits, N, K, 12)

            def support():
                scene_stage.proposal_support(idxd, bits, masks, out=sup)

            def verify():
                scene_stage.proposal_support(idxd, bits, masks, out=sup)
                scene_stage.box_support(pcd, masks, cen, axes, half, out=box)

            verify()
            sup_h, box_h, bits_h, masks_h = sup.cpu().numpy(), box.cpu().numpy(), bits.cpu().numpy().view(np.uint32), masks.cpu().numpy()
            k_ref = K if P <= 500_000 else 1
            want = V.proposal_support(idx, bits_h, masks_h[:k_ref])
            if not np.array_equal(sup_h[:k_ref], want) or not np.array_equal(box_h[:, 0], masks_h.astype(bool).sum(1)):
                raise SystemExit(f"P = {P}, K = {K}: the verification counts differ from tests/verify_ref.py")
            ts = timed_alternating(dict(backvote=backvote, segment=segment, verify=verify, support=support), reps)
            r = {n: stats(t) for n, t in ts.items()}
            row = dict(pairs=P, proposals=K, points=N, within=[int(v) for v in sup_h[:, 0]][:8], agree=[int(v) for v in sup_h[:, 1]][:8],
                       counts_checked=int(k_ref), **r, verify_over_segment=round(r["verify"]["median_us"] / r["segment"]["median_us"], 3),
                       verify_over_backvote_plus_segment=round(r["verify"]["median_us"] / (r["backvote"]["median_us"] + r["segment"]["median_us"]), 3),
                       verify_within_segment=bool(r["verify"]["median_us"] <= r["segment"]["median_us"] + r["segment"]["iqr_us"]))
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def frame_row(dev, n_pairs, reps):
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    cfg = CATEGORIES["bottle"]
    penc, enc = training.load_weights(os.path.join(ROOT, "tests", "golden", "trained_bottle.npz"), cfg, dev)
    ms, out = {False: [], True: []}, None
    for i in range(reps + 1):                                            # the two forms alternate call by call
        for verify in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, n_pairs=n_pairs, seed=0, thresh=5.0, verify=verify)
            ms[verify].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for verify, name in ((False, "plain"), (True, "verify")):
        q1, med, q3 = np.percentile(ms[verify][1:], [25, 50, 75])        # (the first call packs the weights and sizes the scratch)
        res[name] = dict(median_ms=round(float(med), 2), iqr_ms=round(float(q3 - q1), 2))
    return dict(what="scene_poses.scene_frame on tests/golden/demo_0000_depth.png, committed bottle network, thresh 5, without and with "
                     "verify=True, alternating call by call; wall clock per call, read-backs included",
                pairs_drawn=n_pairs, pairs_kept=out["n_pairs"], points=int(out["pc"].shape[0]), proposals=len(out["poses"]), calls=reps,
                **res, verify_minus_plain_ms=round(res["verify"]["median_ms"] - res["plain"]["median_ms"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions per route and row")
    ap.add_argument("--frame-pairs", type=int, default=5_000_000)
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_verify.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify.py needs a HIP device")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps_per_route=args.reps,
               method="one process; per row the routes alternate repetition by repetition, HIP events around each repetition (host launch "
                      "path included); the verification counts compared with tests/verify_ref.py before timing",
               expectation="verify (cppf_proposal_support + cppf_box_support) costs no more than segment (cppf_segment_instances) at the same "
                           "shape: checked against the measured segment time, not a pass mark",
               scene=f"{N_OBJ} bowls of {N_POINTS} points, closed-form (mu, nu) within objects, random elsewhere; proposals on the objects' "
                     "centres, then moved by two cells per round; every box the bowl's extents + res",
               stage=stage_rows(dev, args.reps), scene_frame=frame_row(dev, args.frame_pairs, args.frame_reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["scene_frame"]))


if __name__ == "__main__":
    main()
