#!/usr/bin/env python3
"""gen_stats.py on the MI355X (cppf_amd.mesh_stats, csrc/mesh_stats.hip): for one category, the time of OBJ parsing (Python, host),
of the upload, of the surface sampling and of the statistics (device events), at two sizes -- a few hundred procedural meshes of
about 10^4 triangles, and one mesh of about 2*10^6 triangles -- and the numpy restatement (tests/mesh_stats_ref.py) on the host for
the same inputs.  Prints one JSON line.

    python scripts/bench_gen_stats.py --meshes 300 --reps 5
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
import mesh_stats_ref as SR                 # noqa: E402
from cppf_amd import mesh_stats as MS       # noqa: E402
from cppf_amd.meshes import load_obj        # noqa: E402


def _category(n, rng):
    """n ellipsoids of about 10^4 triangles (UV spheres 50 x 100, axes scaled 0.5-1.5), unit bbox diagonal"""
    out = []
    for _ in range(n):
        v, f = R.uv_sphere(0.5, 50, 100)
        v = v * rng.uniform(0.5, 1.5, 3)
        out.append((v / np.linalg.norm(v.max(0) - v.min(0)), f))
    return out


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _measure(meshes, dev, reps, n_samples, n_pairs, tmp, cpu):
    paths = []
    for k, (v, f) in enumerate(meshes):
        paths.append(os.path.join(tmp, f"m{k}.obj"))
        with open(paths[-1], "w") as fh:
            fh.write(R.to_obj(v, f))
    t0 = time.perf_counter()
    loaded = [load_obj(p) for p in paths]
    parse_ms = (time.perf_counter() - t0) * 1e3
    up = MS.upload_meshes(loaded, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        up = MS.upload_meshes(loaded, dev)
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3 / reps
    sample = lambda: MS.sample_surface_packed(*up, n_samples, seed=0)
    sample_ms = _events(sample, reps)
    pts, _, status = sample()
    stats_ms = _events(lambda: MS.vote_stats_batch(pts, n_pairs, seed=0), reps)
    rows = MS.vote_stats_batch(pts, n_pairs, seed=0)[0].cpu().numpy()
    nv, nf = int(up[2][-1]), int(up[3][-1])
    r = dict(meshes=len(meshes), triangles=nf, vertex_bytes=24 * nv, face_bytes=12 * nf, point_bytes=24 * len(meshes) * n_samples,
             parse_ms=parse_ms, upload_ms=upload_ms, sample_ms=sample_ms, stats_ms=stats_ms)
    if cpu:
        p = pts.cpu().numpy()
        t0 = time.perf_counter()
        ref_pts = [SR.sample_surface(v, f, n_samples, 0, m)[0] for m, (v, f) in enumerate(loaded)]
        t1 = time.perf_counter()
        ref_rows = [SR.vote_stats(ref_pts[m], n_pairs, 0, m) for m in range(len(loaded))]
        t2 = time.perf_counter()
        r.update(cpu_sample_ms=(t1 - t0) * 1e3, cpu_stats_ms=(t2 - t1) * 1e3,
                 equal=bool(np.array_equal(np.stack(ref_pts), p) and np.array_equal(np.stack(ref_rows), rows)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-samples", type=int, default=2048)
    ap.add_argument("--n-pairs", type=int, default=100000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    out = dict(device=torch.cuda.get_device_name(0), n_samples=args.n_samples, n_pairs=args.n_pairs)
    with tempfile.TemporaryDirectory() as tmp:
        out["category_1e4"] = _measure(_category(args.meshes, rng), dev, args.reps, args.n_samples, args.n_pairs, tmp, not args.no_cpu)
    with tempfile.TemporaryDirectory() as tmp:
        out["mesh_2e6"] = _measure([R.uv_sphere(0.5, 1000, 1000)], dev, args.reps, args.n_samples, args.n_pairs, tmp, not args.no_cpu)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
