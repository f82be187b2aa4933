"""The training-side kernels of csrc/scene_train.hip -- cppf_sample_scene_pairs + cppf_scene_pair_targets -- timed
against the torch route to the same targets, in ONE process with HIP events.

The torch route is what the tree offered before: a uniform pair draw (torch.randint), then per instance a mask over the pairs whose two
points carry that instance's label, and one training.targets call on the masked pairs (dense soft targets, as training.loss_fn takes
them).  The new route is the stratified draw (half the pairs in the positive stratum) and ONE targets launch for all instances, in
the compact form scene_loss_fn takes.  The two routes do not produce the same pair lists -- that is the point of the stratified draw --
so the row also holds how many positive pairs each route ends up with.

Shapes: 200 000 and 1 000 000 pairs, K = 4 and 32 instances of 1 024 points each (synthetic posed bottles, all of the target
category).  Per row the routes alternate repetition by repetition after a warm-up, 40 repetitions each, each between its own pair of
events (host launch path included; the torch route's boolean masks synchronise with the host, which is part of what it costs).
Verdict (DESIGN.md 3.7e's rule): "faster" only where the torch route's median exceeds the new route's by more than the torch route's
inter-quartile range.  Writes profiles/scene_targets.json.  Needs a HIP device; there is no fall-back.

    python scripts/bench_scene_targets.py [--reps 40] [--out profiles/scene_targets.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_precision import stats                                        # noqa: E402
from bench_scene_poses import timed_alternating                          # noqa: E402
from cppf_amd import scene_training as ST                                # noqa: E402
from cppf_amd import synthetic as syn                                    # noqa: E402
from cppf_amd import training                                            # noqa: E402
from cppf_amd.config import CATEGORIES                                   # noqa: E402

N_POINTS = 1024


def scene(K, seed=0):
    """K posed bottles on a grid 0.3 m apart, about 1 m away: (pc, nrm f32[K N_POINTS,3], inst i32, objects)"""
    obs, pcs, nrms = [], [], []
    for k in range(K):
        ob = syn.make_posed_object("bottle", N_POINTS, seed * 100 + k)
        c = np.array([0.3 * (k % 8) - 1.0, 0.3 * (k // 8) - 0.5, 1.0 + 0.05 * (k % 3)])
        ob["pc"] = (ob["pc"].astype(np.float64) - ob["center"] + c).astype(np.float32)
        ob["center"] = c
        obs.append(ob), pcs.append(ob["pc"]), nrms.append(ob["normals"])
    return np.concatenate(pcs), np.concatenate(nrms), np.repeat(np.arange(K, dtype=np.int32), N_POINTS), obs


STREAMED_BYTES = 8 + 27                   # per pair: the index pair in, kind + pair_inst + low + w_low + aux out (the gathers hit a cloud that fits L2)


def back_to_back(pcd, nrmd, instd, idx, tabled, flagsd, K, cfg, t, n=50, rounds=5):
    """cppf_scene_pair_targets alone, n raw calls into the same buffers between ONE pair of events: microseconds per call (the median of
    `rounds`) -- the larger of the kernel's time and the host's ~ctypes call, where the wrapper's allocations no longer hide the kernel"""
    from cppf_amd._torch_util import call
    dev, us = pcd.device, []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call("cppf_scene_pair_targets", dev, pcd, nrmd, instd, pcd.shape[0], idx, idx.shape[0], tabled, flagsd, K, float(cfg.vote_range[0]),
                 float(cfg.vote_range[1]), cfg.tr_num_bins, cfg.rot_num_bins, t["kind"], t["pair_inst"], t["low"], t["w_low"], t["aux"])
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / n)
    return float(np.median(us[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_targets.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_targets.py needs a HIP device")
    dev = torch.device("cuda:0")
    cfg = CATEGORIES["bottle"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows = []
    for K in (4, 32):
        pc, nrm, inst, obs = scene(K)
        pcd, nrmd, instd = d(pc), d(nrm), d(inst)
        table, flags = ST.instance_table([o["center"] for o in obs], [o["R"] for o in obs], [o["half_extents"] for o in obs], [True] * K, cfg)
        tabled, flagsd = d(table), d(flags)
        members, seg_off = ST.target_members(instd, flags)
        N = pc.shape[0]
        for P in (200_000, 1_000_000):
            gen = torch.Generator(device=dev).manual_seed(0)
            kept = {}

            def new_route():
                idx = ST.sample_scene_pairs(members, seg_off, instd, P, P // 2, 1)
                kept["new"] = ST.scene_pair_targets(pcd, nrmd, instd, idx, tabled, flagsd, cfg)

            def new_targets_only(idx=ST.sample_scene_pairs(members, seg_off, instd, P, P // 2, 1)):
                kept["new_t"] = ST.scene_pair_targets(pcd, nrmd, instd, idx, tabled, flagsd, cfg)

            def torch_route():
                idx = torch.randint(0, N, (P, 2), device=dev, generator=gen)
                la, lb = instd[idx[:, 0]], instd[idx[:, 1]]
                out = []
                for k, ob in enumerate(obs):
                    ik = idx[(la == k) & (lb == k)]
                    out.append(training.targets(pcd, nrmd, ik, ob["center"], ob["R"], ob["half_extents"], cfg))
                kept["torch"] = out

            ts = timed_alternating(dict(new=new_route, torch=torch_route, new_targets_only=new_targets_only), args.reps)
            r = {n: stats(t) for n, t in ts.items()}
            b2b = back_to_back(pcd, nrmd, instd, ST.sample_scene_pairs(members, seg_off, instd, P, P // 2, 1), tabled, flagsd, K, cfg, kept["new"])
            faster = r["torch"]["median_us"] - r["new"]["median_us"] > r["torch"]["iqr_us"]
            row = dict(pairs=P, instances=K, points=N, **r, positives_new=int((kept["new"]["kind"] == 1).sum()),
                       positives_torch=int(sum(t[0].shape[0] for t in kept["torch"])),
                       torch_over_new=round(r["torch"]["median_us"] / r["new"]["median_us"], 2),
                       new_pairs_per_us=round(P / r["new"]["median_us"], 1), targets_back_to_back_us=round(b2b, 2),
                       targets_back_to_back_gb_per_s=round(P * STREAMED_BYTES / b2b / 1e3, 1),
                       verdict="faster" if faster else "not shown faster")
            print(json.dumps(row), flush=True)
            rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0), reps_per_route=args.reps,
               method="one process; per row the routes alternate repetition by repetition after 3 warm-up calls each, HIP events around each "
                      "repetition (host launch path and, for the torch route, its host synchronisations included)",
               routes=dict(new="cppf_sample_scene_pairs (half the pairs in the positive stratum) + cppf_scene_pair_targets: compact targets of "
                               "every pair, all instances in one launch",
                           new_targets_only="cppf_scene_pair_targets alone on a list drawn before",
                           targets_back_to_back="cppf_scene_pair_targets, 50 raw calls into the same buffers between one pair of events, per call "
                                                "(median of 5 rounds); GB/s counts the 35 streamed bytes per pair, not the cached gathers",
                           torch="torch.randint pairs, then per instance a boolean mask over the pairs and one training.targets call on the "
                                 "masked pairs (dense targets)"),
               rule="'faster' only where the torch route's median exceeds the new route's by more than the torch route's inter-quartile range",
               scene=f"K posed synthetic bottles of {N_POINTS} points each, all of the target category", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
