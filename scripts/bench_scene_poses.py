"""The per-proposal stage of a scene, one pass for all proposals against one pass per proposal, timed in ONE process with HIP events
(the method of scripts/bench_precision.py):

  new       cppf_backvote_multi + cppf_segment_instances                      (csrc/scene_multi.hip)
  baseline  K x (cppf_backvote_ws + cppf_segment_instance)                    (`single` below: what zero_shot_scene looped over before it took the new route)

on a synthetic scene of eight bowls with perfect (mu, nu) for within-object pairs, K in {1, 4, 8, 32} proposals at 500 000 and
5 000 000 pairs.  The K centres are the objects' centres, then the same centres moved by two cells per round, so every proposal sits
on a vote peak and keeps pairs.  Per row the two routes alternate repetition by repetition after a warm-up, each repetition between its
own pair of events; median and inter-quartile range of the per-repetition times.  Before a row is timed both routes' outputs are
compared (point masks and kept lists of every proposal): a row that differs ends the script.

The new route counts as faster at a row only where the baseline median exceeds its median by more than the baseline's inter-quartile
range of that row.  Also times scene_poses.scene_frame on tests/golden/demo_0000_depth.png with the committed bottle network (wall
clock around each call, ending in its read-back).  Writes profiles/scene_poses.json.  Needs a HIP device; there is no fall-back.

    python scripts/bench_scene_poses.py [--reps 40] [--frame-pairs 5000000] [--out profiles/scene_poses.json]"""
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

import cppf_amd.synthetic as syn                                        # noqa: E402
from bench_precision import stats                                        # noqa: E402
from cppf_amd import _lib, scene_poses, training                          # noqa: E402
from cppf_amd._torch_util import call, scratch, workspace                # noqa: E402
from cppf_amd.config import CATEGORIES                                   # noqa: E402
from cppf_amd.inference import grid_shape                                # noqa: E402

RULE = ("the new route counts as faster only if the baseline median exceeds its median by more than the baseline's inter-quartile "
        "range of the same row")
N_OBJ, N_POINTS = 8, 1024


def scene(n_pairs, seed=0):
    cfg = CATEGORIES["bowl"]
    rng = np.random.default_rng(seed)
    pcs, centers = [], []
    for k in range(N_OBJ):
        ob = syn.make_posed_object("bowl", N_POINTS, 50 + k, rotate=False)
        c = np.array([0.3 * (k % 4) - 0.45, 0.05 * (k % 2), 0.8 + 0.3 * (k // 4)])
        pcs.append((ob["pc"] - ob["center"] + c).astype(np.float32))
        centers.append(c)
    pc = np.concatenate(pcs)
    owner = np.repeat(np.arange(N_OBJ), N_POINTS)
    idx = rng.integers(0, pc.shape[0], (n_pairs, 2)).astype(np.int32)
    out = np.empty((n_pairs, 2), np.float32)
    out[:, 0] = rng.uniform(-cfg.vote_range[0], cfg.vote_range[0], n_pairs)
    out[:, 1] = rng.uniform(0, cfg.vote_range[1], n_pairs)
    for k in range(N_OBJ):
        w = (owner[idx[:, 0]] == k) & (owner[idx[:, 1]] == k)
        out[w] = syn.closed_form_outputs(pc, centers[k], idx[w], cfg, quantise=False)
    return cfg, pc, idx, out, np.array(centers)


def proposal_centers(centers, K, res):
    return np.ascontiguousarray(np.array([centers[k % N_OBJ] + np.array([2 * res * (k // N_OBJ), 0, 0]) for k in range(K)], np.float32))


def timed_alternating(routes, reps, warmup=3):
    """{name: fn} -> {name: [ms]}: the routes alternate repetition by repetition, each repetition between its own events"""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    evs = {n: [] for n in routes}
    for _ in range(reps):
        for n, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[n].append((e0, e1))
    torch.cuda.synchronize()
    return {n: [a.elapsed_time(b) for a, b in v] for n, v in evs.items()}


def single(pc, outputs, idx32, T32, corner, res, dims, num_rots, tol, min_contrib):
    """the baseline: back-vote at T32 + segmentation of one proposal, all enqueued: (point_mask u8[N], positions i32[P], count i32[1])"""
    dev = pc.device
    N, P = pc.shape[0], idx32.shape[0]
    surv = torch.empty(P, dtype=torch.uint8, device=dev)
    point_mask = torch.empty(N, dtype=torch.uint8, device=dev)
    pairs = torch.empty(P, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    call("cppf_backvote_ws", dev, pc, outputs, None, idx32, corner, float(res), P, num_rots, *(int(d) for d in dims), None, T32, tol, surv, None)
    sws = workspace(_lib.lib().cppf_segment_instance_workspace_bytes(N, P), dev, "segment")
    call("cppf_segment_instance", dev, idx32, surv, P, N, min_contrib, point_mask, pairs, count, scratch(sws))
    return point_mask, pairs, count


def stage_rows(dev, reps):
    rows = []
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for P in (500_000, 5_000_000):
        cfg, pc, idx, out, centers = scene(P)
        corners, dims = grid_shape(pc, cfg.res)
        pcd, idxd, outd, corner = d(pc), d(idx), d(out), d(corners[0])
        N = pc.shape[0]
        tol = float(np.float32(3 * cfg.res))
        for K in (1, 4, 8, 32):
            cs = d(proposal_centers(centers, K, cfg.res))
            bits = torch.empty(P, dtype=torch.int32, device=dev)

            def new():
                scene_poses.backvote_multi(pcd, outd, idxd, corner, cfg.res, dims, cs, 72, out=bits)
                return scene_poses.segment_instances(idxd, bits, N, K, 12)

            def base():
                return [single(pcd, outd, idxd, cs[k], corner, cfg.res, dims, 72, tol, 12) for k in range(K)]

            masks, pairs, offsets = new()
            off = offsets.cpu().numpy().astype(np.int64)
            if off[K] > pairs.shape[0]:
                masks, pairs, offsets = scene_poses.segment_instances(idxd, bits, N, K, 12, capacity=int(off[K]))
            for k, (pm, lst, cnt) in enumerate(base()):
                n = int(cnt.item())
                if n != off[k + 1] - off[k] or not torch.equal(pm, masks[k]) or not torch.equal(lst[:n], pairs[off[k]:off[k + 1]]):
                    raise SystemExit(f"P = {P}, K = {K}: the two routes differ at proposal {k}")
            ts = timed_alternating(dict(baseline=base, new=new), reps)
            r = {n: stats(t) for n, t in ts.items()}
            gain = r["baseline"]["median_us"] - r["new"]["median_us"]
            row = dict(pairs=P, proposals=K, kept_items=int(off[K]), outputs_equal=True, baseline=r["baseline"], new=r["new"],
                       baseline_over_new=round(r["baseline"]["median_us"] / r["new"]["median_us"], 3),
                       new_faster=bool(gain > r["baseline"]["iqr_us"]))
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def frame_row(dev, n_pairs, reps):
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    cfg = CATEGORIES["bottle"]
    penc, enc = training.load_weights(os.path.join(ROOT, "tests", "golden", "trained_bottle.npz"), cfg, dev)
    ms, out = [], None
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, n_pairs=n_pairs, seed=0, thresh=5.0)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[1:]                                                          # (the first call packs the weights and sizes the scratch)
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return dict(what="scene_poses.scene_frame on tests/golden/demo_0000_depth.png, committed bottle network, thresh 5 (a network that never "
                     "saw such a scene: the time is the figure, not the poses); wall clock per call, read-backs included",
                pairs_drawn=n_pairs, pairs_kept=out["n_pairs"], points=int(out["pc"].shape[0]), proposals=len(out["poses"]), calls=reps,
                median_ms=round(float(med), 2), iqr_ms=round(float(q3 - q1), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions per route and row")
    ap.add_argument("--frame-pairs", type=int, default=5_000_000)
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_poses.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_poses.py needs a HIP device")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps_per_route=args.reps, rule=RULE,
               method="one process; per row the routes alternate repetition by repetition, HIP events around each repetition (host launch "
                      "path included); outputs of both routes compared before timing",
               scene=f"{N_OBJ} bowls of {N_POINTS} points, closed-form (mu, nu) within objects, random elsewhere; proposals on the objects' "
                     "centres, then moved by two cells per round",
               per_proposal_stage=stage_rows(dev, args.reps), scene_frame=frame_row(dev, args.frame_pairs, args.frame_reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["scene_frame"]))


if __name__ == "__main__":
    main()
