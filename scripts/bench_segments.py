"""The kernels of csrc/segments.hip timed against what the tree offered before, in ONE process with HIP events.

cppf_depth_segments (depth on the device in, labels on the device out) against
  host    the depth copied off the device, the link graph in numpy, scipy.sparse.csgraph.connected_components, re-rooting and ranking in
          numpy (tests/segments_ref.py's route), the labels copied back
  torch   a min-propagation loop on the device: every live pixel takes the smallest label among itself and its linked 4-neighbours
          until nothing changes (one host synchronisation per 8 sweeps), then sizes by bincount and ranks by a prefix sum
on the demo frame (tests/golden/demo_0000_depth.png, 480 x 640) and one rendered frame (mesh_frames.MeshFrameSampler, 4 objects).
cppf_plane_ransac against the same 256 hypotheses in torch (one [N,256] distance matrix) at N = 215 686, the demo frame's valid pixels.
The outputs are compared first (labels exactly; counts exactly on the kernel's planes).  Per row the routes alternate repetition by
repetition after a warm-up, 40 repetitions each.  Verdict (DESIGN.md 3.7e's rule): "faster" only where the baseline's median exceeds
the new route's by more than the baseline's inter-quartile range.  Also: the demo frame's component table at n_planes = 0, 1, 2 and
the wall time of frame_segments.  Writes profiles/segments.json.  Needs a HIP device; there is no fall-back.

    python scripts/bench_segments.py [--reps 40] [--out profiles/segments.json]"""
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

import segments_ref as R                                                 # noqa: E402
from bench_precision import stats                                        # noqa: E402
from bench_scene_poses import timed_alternating                          # noqa: E402
from cppf_amd import mesh_frames as MF                                   # noqa: E402
from cppf_amd import segments as SG                                      # noqa: E402
from cppf_amd.frames import NOCS_INTRINSICS                              # noqa: E402
from cppf_amd.utils.util import backproject, read_depth_png              # noqa: E402

KW = dict(tol_mm=10, slope_permille=10, min_pixels=200, max_pixels=0, capacity=256)


def torch_segments(d16, tol_mm, slope_permille, min_pixels, max_pixels, capacity):
    """labels i32[H,W] by min-propagation on the device (depth: the int16 bits)"""
    z = d16.int() & 0xFFFF
    H, W = z.shape
    live = z > 0
    big = H * W
    lab = torch.where(live, torch.arange(big, device=z.device, dtype=torch.int32).view(H, W), torch.full_like(z, big))

    def linked(a, b):
        return (a > 0) & (b > 0) & ((a - b).abs() <= tol_mm + (slope_permille * torch.minimum(a, b)) // 1000)

    lh, lv = linked(z[:, 1:], z[:, :-1]), linked(z[1:, :], z[:-1, :])
    while True:
        before = lab
        for _ in range(8):
            new = lab.clone()
            new[:, 1:] = torch.where(lh, torch.minimum(new[:, 1:], lab[:, :-1]), new[:, 1:])
            new[:, :-1] = torch.where(lh, torch.minimum(new[:, :-1], lab[:, 1:]), new[:, :-1])
            new[1:, :] = torch.where(lv, torch.minimum(new[1:, :], lab[:-1, :]), new[1:, :])
            new[:-1, :] = torch.where(lv, torch.minimum(new[:-1, :], lab[1:, :]), new[:-1, :])
            lab = new
        if torch.equal(lab, before):                                     # (the host synchronisation of the loop)
            break
    root = lab.reshape(-1).long()
    size = torch.bincount(root[live.reshape(-1)], minlength=big + 1)
    keep = (size >= min_pixels) & ((size <= max_pixels) if max_pixels else torch.ones_like(size, dtype=torch.bool))
    keep[big] = False
    rank = torch.cumsum(keep.int(), 0) - 1
    return torch.where(keep[root], rank[root], torch.full_like(root, -1)).int().view(H, W)


def host_segments(d16, **kw):
    depth = d16.cpu().numpy().view(np.uint16)
    return torch.from_numpy(R.segments_ref(depth, None, **kw)["labels"]).to(d16.device)


def torch_plane_counts(p, planes, thresh):
    """counts of the kernel's own planes in torch: one [N, n_hyp] matrix of distances"""
    s = ((p[:, 0:1] * planes[None, :, 0] + p[:, 1:2] * planes[None, :, 1]) + p[:, 2:3] * planes[None, :, 2]) + planes[None, :, 3]
    ok = (planes[:, :3] != 0).any(-1)
    return ((s.abs() <= thresh) & ok[None]).sum(0).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segments.py needs a HIP device")
    dev = torch.device("cuda:0")
    demo = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    from test_gpu_scene_training import _meshes
    fr = MF.MeshFrameSampler(_meshes(), 4, device=dev, seed=1, z_range=(0.6, 1.2)).sample()
    rows = []
    for name, depth in (("demo_frame", demo), ("rendered_frame", fr.depth_mm)):
        d16 = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(dev)
        kept = {}
        routes = dict(new=lambda: kept.__setitem__("new", SG.depth_segments_device(d16, None, **KW)["labels"]),
                      host=lambda: kept.__setitem__("host", host_segments(d16, **KW)),
                      torch=lambda: kept.__setitem__("torch", torch_segments(d16, **KW)))
        for f in routes.values():
            f()
        torch.cuda.synchronize()
        assert torch.equal(kept["new"], kept["host"]) and torch.equal(kept["new"], kept["torch"]), name
        ts = timed_alternating(routes, args.reps)
        r = {n: stats(t) for n, t in ts.items()}
        row = dict(what="cppf_depth_segments", frame=name, shape=list(depth.shape), live_pixels=int((depth > 0).sum()), **r)
        for base in ("host", "torch"):
            faster = r[base]["median_us"] - r["new"]["median_us"] > r[base]["iqr_us"]
            row[f"{base}_over_new"] = round(r[base]["median_us"] / r["new"]["median_us"], 2)
            row[f"verdict_against_{base}"] = "faster" if faster else "not shown faster"
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the plane fit at the demo frame's valid pixels
    pts, _ = backproject(demo, NOCS_INTRINSICS, np.ones(demo.shape, bool), return_device=True)
    p = (pts / 1000.0).float().contiguous()
    planes, counts, _ = SG.plane_ransac_device(p, 256, 0.01, 0)
    assert torch.equal(counts, torch_plane_counts(p, planes, 0.01))
    kept = {}
    routes = dict(new=lambda: kept.__setitem__("new", SG.plane_ransac_device(p, 256, 0.01, 0)),
                  torch=lambda: kept.__setitem__("torch", torch_plane_counts(p, planes, 0.01)))
    ts = timed_alternating(routes, args.reps)
    r = {n: stats(t) for n, t in ts.items()}
    row = dict(what="cppf_plane_ransac", points=int(p.shape[0]), n_hyp=256, **r, torch_over_new=round(r["torch"]["median_us"] / r["new"]["median_us"], 2),
               verdict_against_torch="faster" if r["torch"]["median_us"] - r["new"]["median_us"] > r["torch"]["iqr_us"] else "not shown faster",
               note="the torch route counts the kernel's own planes (it does not draw or build them)")
    print(json.dumps(row), flush=True)
    rows.append(row)
    # the demo frame's component table through the device path, and frame_segments' wall time
    table = []
    for n_planes in (0, 1, 2):
        SG.frame_segments(demo, NOCS_INTRINSICS, n_planes=n_planes)        # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            t0 = time.perf_counter()
            s = SG.frame_segments(demo, NOCS_INTRINSICS, n_planes=n_planes)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        full = SG.depth_segments(demo, s["valid"], min_pixels=1, capacity=1024) if s["n_components"] <= 1024 else s
        sizes = sorted(full["sizes"].cpu().numpy().tolist(), reverse=True)
        pl, inl = s["planes"], None
        if pl:
            rest = p[SG.off_planes(p, pl[:-1], 0.015)]
            inl = int(((rest @ torch.from_numpy(pl[-1][:3].copy()).to(dev) + float(pl[-1][3])).abs() <= 0.01).sum())
        one = dict(n_planes=n_planes, planes_found=len(pl), components=s["n_components"], segments_of_200_pixels=s["n_segments"],
                   inliers_of_the_plane_just_removed=inl, largest_component_sizes=sizes[:10], frame_segments_wall_ms_median=float(np.median(ms)))
        print(json.dumps(one), flush=True)
        table.append(one)
    out = dict(device=torch.cuda.get_device_name(0), reps_per_route=args.reps,
               method="one process; per row the routes alternate repetition by repetition after a warm-up, HIP events around each repetition "
                      "(host launch path, allocations of the outputs and, for the baselines, their host synchronisations and copies included); "
                      "outputs compared first",
               rule="'faster' only where the baseline's median exceeds the new route's by more than the baseline's inter-quartile range",
               options=KW, rows=rows, demo_frame_table=table)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
