#!/usr/bin/env python3
"""Training views from meshes on the MI355X: device time per render (csrc/raster.hip) and per complete sample
(MeshViewSampler.sample: render, compaction, object frame, jitter, voxel dedupe, normals, pairs, targets) on procedural spheres of
about 10^3, 10^5 and 2*10^6 triangles; training steps/s of training.train_on_meshes next to training.train(); and the numpy
restatement's render time on the CPU (tests/mesh_ref.py) as the baseline.  Prints one JSON line.

    python scripts/bench_mesh_views.py --renders 50 --samples 20 --train-steps 100
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_ref as R                        # noqa: E402
from cppf_amd import meshes as M            # noqa: E402
from cppf_amd import training               # noqa: E402

SIZES = {"1e3": (22, 24), "1e5": (224, 224), "2e6": (1000, 1000)}     # (n_lat, n_lon) of the UV sphere


def _sphere(n_lat, n_lon):
    v, f = R.uv_sphere(0.5, n_lat, n_lon)
    return v / np.linalg.norm(v.max(0) - v.min(0)), f                 # unit bbox diagonal, as ShapeNet's model_normalized


def _device_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(n):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--renders", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=100)
    ap.add_argument("--cpu-sizes", nargs="*", default=["1e3", "1e5"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    out = dict(device=torch.cuda.get_device_name(0), render_ms={}, sample_ms={}, triangles={}, cpu_render_ms={})
    depth = torch.empty((M.HEIGHT, M.WIDTH), dtype=torch.float32, device=dev)
    models = []
    for _ in range(max(args.renders, 1) + 1):
        Rm, t = M.draw_pose(rng, True)
        models.append(M.model_matrix(Rm, t, rng.uniform(0.23, 0.46), np.full(3, -0.29), np.full(3, 0.29)))
    for name, (la, lo) in SIZES.items():
        v, f = _sphere(la, lo)
        out["triangles"][name] = int(f.shape[0])
        mesh = M._Mesh(v, f, dev)
        out["render_ms"][name] = _device_ms(lambda k=0: M._render(mesh, models[k], depth, sync=False), args.renders)
        sampler = M.MeshViewSampler(None, "bottle", dev, seed=1, n_pairs=60000, meshes=[(v, f)])
        out["sample_ms"][name] = _device_ms(lambda k=0: sampler.sample(), args.samples)
        if name in args.cpu_sizes:
            t0 = time.perf_counter()
            R.raster_ref(v, f, models[0])
            out["cpu_render_ms"][name] = (time.perf_counter() - t0) * 1e3
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k in range(4):
            v, f = R.necked_cylinder(0.15, 0.40 + 0.02 * k, n_lon=48)
            p = os.path.join(d, f"b{k}.obj")
            open(p, "w").write(R.to_obj(v / np.linalg.norm(v.max(0) - v.min(0)), f))
            paths.append(p)
        n = args.train_steps
        training.train_on_meshes("bottle", paths, dev, steps=5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        training.train_on_meshes("bottle", paths, dev, steps=n)
        torch.cuda.synchronize()
        out["train_on_meshes_steps_per_s"] = n / (time.perf_counter() - t0)
        training.train("bottle", dev, steps=5, n_points=(768, 2048))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        training.train("bottle", dev, steps=n, n_points=(768, 2048))
        torch.cuda.synchronize()
        out["train_synthetic_steps_per_s"] = n / (time.perf_counter() - t0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
