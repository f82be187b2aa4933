#!/usr/bin/env python3
"""Mesh frames on the MI355X: one cppf_raster_instances pass (meshes.render_instances) against the route without it -- K single
renders (meshes._render, without a host synchronisation) into K buffers and a torch composite (min and arg-min over the covered
pixels) -- on the same meshes and matrices: K in {1, 8, 32} instances of a UV sphere of 10^3 and of 10^5 triangles at 640 x 480.

Every shape is warmed up, the two routes alternate in one process, each repetition is timed with device events (the route's
host work between the events included: that is what a caller waits for), and the two routes' outputs are compared in the same
run.  Medians and inter-quartile ranges go to profiles/mesh_frames.json (--out); "faster" is written for a shape only where the
medians differ by more than the baseline's inter-quartile range, "not faster" otherwise.

    python scripts/bench_mesh_frames.py --reps 200
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_ref as R                        # noqa: E402
from cppf_amd import meshes as M            # noqa: E402

SIZES = {"1e3": (11, 50), "1e5": (126, 400)}                         # (n_lat, n_lon) of the UV sphere: n_lon (2 n_lat - 2) faces


def _matrices(rng, K):
    out = []
    for _ in range(K):
        Rm, _ = M.draw_pose(rng, True)
        t = np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.3, 0.3), -rng.uniform(0.9, 2.0)])
        out.append(M.model_matrix(Rm, t, rng.uniform(0.25, 0.45), np.full(3, -0.5), np.full(3, 0.5)))
    return np.asarray(out)


def _quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), reps=len(ms))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--instances", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--sizes", nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_frames.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, W = M.HEIGHT, M.WIDTH
    inf = torch.tensor(float("inf"), device=dev)
    out = dict(device=torch.cuda.get_device_name(0), width=W, height=H, reps=args.reps, warmup=args.warmup,
               baseline="K meshes._render(sync=False) calls into K buffers + torch.where / min(0) composite",
               rule="faster: baseline median - single-pass median > baseline inter-quartile range", shapes=[])
    for name in args.sizes:
        v, f = R.uv_sphere(0.5, *SIZES[name])
        mesh = M._Mesh(v, f, dev)
        mset = M.mesh_set([(v, f)], dev)
        for K in args.instances:
            mvs = _matrices(np.random.default_rng(1000 + K), K)
            inst = np.zeros(K, np.int32)
            stack = torch.empty((K, H, W), dtype=torch.float32, device=dev)
            both = (torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev))
            res = {}

            def single_pass():
                M.render_instances(mset, inst, mvs, device=dev, out=both)

            def baseline():
                for k in range(K):
                    M._render(mesh, mvs[k], stack[k], sync=False)
                s = torch.where(stack > 0, stack, inf)
                d, lab = s.min(0)
                covered = d < inf
                res["depth"], res["labels"] = torch.where(covered, d, 0.0), torch.where(covered, lab, -1)

            for k in range(K):                                        # (the bin lists grow to what these matrices need)
                M._render(mesh, mvs[k], stack[k], sync=True)
            for _ in range(max(1, args.warmup)):
                single_pass()
                baseline()
            torch.cuda.synchronize()
            # the outputs of the two routes, in this run: depth bit for bit; labels against the first arg-min (torch's min(0) may
            # return any of several equal minima, so the lowest index is taken explicitly here, outside the timed composite)
            s = torch.where(stack > 0, stack, inf)
            idx = torch.arange(K, device=dev, dtype=torch.int32)[:, None, None]
            first = torch.where(s == s.min(0).values, idx, K).amin(0)
            first = torch.where(s.min(0).values < inf, first, -1).to(torch.int32)
            equal = bool(torch.equal(both[0].view(torch.int32), res["depth"].view(torch.int32)) and torch.equal(both[1], first))
            t_new, t_old = [], []
            for _ in range(args.reps):
                t_new.append(_timed(single_pass))
                t_old.append(_timed(baseline))
            q_new, q_old = _quartiles(t_new), _quartiles(t_old)
            faster = q_old["median_ms"] - q_new["median_ms"] > q_old["iqr_ms"]
            shape = dict(triangles_per_mesh=int(f.shape[0]), instances=K, covered_pixels=int((both[1] >= 0).sum().item()),
                         single_pass=q_new, baseline=q_old, outputs_equal=equal, verdict="faster" if faster else "not faster",
                         speedup=q_old["median_ms"] / q_new["median_ms"])
            out["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if not all(s["outputs_equal"] for s in out["shapes"]):
        sys.exit("the two routes' outputs differ")


if __name__ == "__main__":
    main()
