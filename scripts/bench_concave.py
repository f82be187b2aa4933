"""cppf_concave_edges (csrc/concave.hip) timed against a torch route on the device, in ONE process per step with HIP
events, following scripts/bench_segments.py's protocol.

  new     segments.concave_edges_device: depth on the device in; edge, normal and counts on the device out (three launches)
  torch   the same definition in torch ops on the device: the (2r+1)^2 window by torch.nn.functional.unfold, the nine sums as one
          masked reduction each, the Cramer determinants in int64, the surface and the edge tests in fp64 tensor arithmetic in the
          definition's order, the neighbours at +-step by padded slices
on the demo frame (tests/golden/demo_0000_depth.png, 480 x 640) and one tabletop frame (mesh_frames.TabletopFrameSampler, 4 objects,
min_gap 0, 640 x 480).  The outputs are compared first: the edge masks pixel by pixel (the number that differ is recorded; more than
1 in 10 000 stops the run) and the normals to 1e-9 -- the torch route's divisions and square roots are torch's, not pinned, so a test
that falls within a rounding of its threshold may go the other way.  The routes alternate repetition by repetition after a warm-up, 40 repetitions
each.  Verdict (DESIGN.md 3.7e's rule): "faster" only where the baseline's median exceeds the new route's by more than the baseline's
inter-quartile range.  A third step times frame_segments on the demo frame with the cut against two planes, and lists the frame's
components with the cut alone, with one plane, and with both.

Every step that uses the device is a child process of its own under its own time limit (--step names the one to run; without it the
steps run one after the other and the first that fails, hangs or faults ends the run).  Writes profiles/concave.json.  Needs a HIP
device; there is no fall-back.

    python scripts/bench_concave.py [--reps 40] [--out profiles/concave.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = {"demo_frame": 240, "tabletop_frame": 240, "frame_segments": 300}      # seconds each may take


def _shift(a, dy, dx, fill=0):
    """out[y, x] = a[y + dy, x + dx] inside the frame, `fill` elsewhere (a: [H,W] or [H,W,C])"""
    H, W = a.shape[:2]
    out = torch.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def torch_concave(d16, K, radius, step, tol_mm, slope_permille, min_count, cos_max, span_max):
    """(edge u8[H,W], normal f64[H,W,3], counts i32[4]) of include/cppf.h "Concave edges" in torch ops on d16's device"""
    F = torch.nn.functional
    f64 = torch.float64
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    z = (d16.int() & 0xFFFF).to(f64)
    H, W = z.shape
    live = z > 0
    k = 2 * radius + 1
    zq = F.unfold(z[None, None], k, padding=radius)[0].view(k * k, H, W)      # 0 outside the frame: dead
    off = torch.arange(-radius, radius + 1, device=z.device, dtype=f64)
    dv, du = (t.reshape(-1, 1, 1) for t in torch.meshgrid(off, off, indexing="ij"))
    lim = tol_mm + torch.floor(slope_permille * z / 1000.0)
    dz = zq - z
    adm = ((zq > 0) & live & (dz.abs() <= lim * torch.maximum(torch.maximum(du.abs(), dv.abs()), torch.ones_like(du)))).to(f64)
    dz = dz * adm
    n, Su, Sv, Suu, Suv, Svv, Sz, Szu, Szv = (t.sum(0).long() for t in (adm, adm * du, adm * dv, adm * du * du, adm * du * dv, adm * dv * dv,
                                                                        dz, dz * du, dz * dv))
    C00, C01, C02 = Suu * Svv - Suv * Suv, Suv * Sv - Su * Svv, Su * Suv - Suu * Sv
    C11, C12, C22 = n * Svv - Sv * Sv, Su * Sv - n * Suv, n * Suu - Su * Su
    D = n * C00 + Su * C01 + Sv * C02
    has = live & (n >= min_count) & (D > 0)
    Dd = torch.where(has, D, torch.ones_like(D)).to(f64)
    zero = torch.zeros_like(z)
    c = torch.where(has, (z + (C00 * Sz + C01 * Szu + C02 * Szv).to(f64) / Dd) / 1000.0, zero)
    am = torch.where(has, ((C01 * Sz + C11 * Szu + C12 * Szv).to(f64) / Dd) / 1000.0, zero)
    bm = torch.where(has, ((C02 * Sz + C12 * Szu + C22 * Szv).to(f64) / Dd) / 1000.0, zero)
    v, u = torch.meshgrid(torch.arange(H, device=z.device, dtype=f64), torch.arange(W, device=z.device, dtype=f64), indexing="ij")
    xu, yv = u - cx, v - cy
    pux, puy, puz = c / fx + (xu * am) / fx, (yv * am) / fy, am
    pvx, pvy, pvz = (xu * bm) / fx, c / fy + (yv * bm) / fy, bm
    nx, ny, nz = puy * pvz - puz * pvy, puz * pvx - pux * pvz, pux * pvy - puy * pvx
    P = torch.stack([(xu * c) / fx, (yv * c) / fy, c], -1)
    flip = (nx * P[..., 0] + ny * P[..., 1]) + nz * P[..., 2] > 0
    N = torch.stack([nx, ny, nz], -1)
    N = torch.where(flip[..., None], -N, N)
    ln = torch.sqrt((N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2])
    fit = torch.isfinite(ln) & (ln > 0)
    N = torch.where(fit[..., None], N / torch.where(fit, ln, torch.ones_like(ln))[..., None], torch.zeros_like(N))
    edge = torch.zeros_like(live)
    for dy, dx in ((0, step), (step, 0)):
        Nm, Np, Pm, Pp = _shift(N, -dy, -dx), _shift(N, dy, dx), _shift(P, -dy, -dx), _shift(P, dy, dx)
        both = _shift(fit, -dy, -dx, False) & _shift(fit, dy, dx, False)
        d, g = Pp - Pm, Np - Nm
        span2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        cosn = (Nm[..., 0] * Np[..., 0] + Nm[..., 1] * Np[..., 1]) + Nm[..., 2] * Np[..., 2]
        conv = (d[..., 0] * g[..., 0] + d[..., 1] * g[..., 1]) + d[..., 2] * g[..., 2]
        edge |= live & both & (span2 <= span_max * span_max) & (cosn < cos_max) & (conv < 0)
    counts = torch.stack([edge.sum(), fit.sum(), live.sum(), torch.zeros((), dtype=torch.int64, device=z.device)]).int()
    return edge.to(torch.uint8), N, counts


def tabletop_frame(dev):
    from cppf_amd import mesh_frames as MF
    import tabletop_cases as TC
    return MF.TabletopFrameSampler(TC.meshes(), 4, device=dev, seed=1, z_range=(0.6, 1.6), min_gap=0.0).sample()


def step_routes(name, reps):
    """one frame: the outputs compared, then the two routes timed"""
    from bench_precision import stats
    from bench_scene_poses import timed_alternating
    from cppf_amd import segments as SG
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    dev = torch.device("cuda:0")
    if name == "demo_frame":
        depth, K = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png")), np.asarray(NOCS_INTRINSICS, np.float64)
    else:
        fr = tabletop_frame(dev)
        depth, K = fr.depth_mm, fr.intrinsics
    o = SG.concave_options()
    d16 = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(dev)
    out = SG.concave_edges_device(d16, K, None, **o)
    t_edge, t_normal, t_counts = torch_concave(d16, K, **o)
    torch.cuda.synchronize()
    differ = int((out["edge"] != t_edge).sum())
    err = float((out["normal"] - t_normal).abs().max())
    assert differ <= d16.numel() // 10000 and err <= 1e-9, (name, differ, err, out["counts"].tolist(), t_counts.tolist())
    kept = {}
    routes = dict(new=lambda: kept.__setitem__("new", SG.concave_edges_device(d16, K, None, **o)),
                  torch=lambda: kept.__setitem__("torch", torch_concave(d16, K, **o)))
    r = {n: stats(t) for n, t in timed_alternating(routes, reps).items()}
    n_edge, n_fit, n_live, _ = out["counts"].cpu().numpy().tolist()
    return dict(what="cppf_concave_edges", frame=name, shape=list(depth.shape), live_pixels=n_live, fits=n_fit, edge_pixels=n_edge,
                edge_pixels_that_differ_from_torch=differ, largest_normal_difference=err, **r,
                torch_over_new=round(r["torch"]["median_us"] / r["new"]["median_us"], 2),
                verdict_against_torch="faster" if r["torch"]["median_us"] - r["new"]["median_us"] > r["torch"]["iqr_us"] else "not shown faster")


def step_frame_segments():
    """the demo frame's components with the cut alone, with one plane, with both, with two planes and with neither, and
    frame_segments' wall time for each"""
    from cppf_amd import segments as SG
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    demo = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    table = []
    for n_planes, concave in ((0, None), (0, {}), (0, dict(radius=4, step=5)), (1, None), (1, {}), (2, None), (2, {})):
        SG.frame_segments(demo, NOCS_INTRINSICS, n_planes=n_planes, concave=concave)        # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            t0 = time.perf_counter()
            s = SG.frame_segments(demo, NOCS_INTRINSICS, n_planes=n_planes, concave=concave)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        full = SG.depth_segments(demo, s["valid"], min_pixels=1, capacity=1024) if s["n_components"] <= 1024 else None
        sizes = sorted((full or s)["sizes"].cpu().numpy().tolist(), reverse=True)
        table.append(dict(n_planes=n_planes, concave=s.get("concave"), planes_found=len(s["planes"]), components=s["n_components"],
                          segments_of_200_pixels=s["n_segments"], edge_pixels=int(s["edge"].sum()) if "edge" in s else None,
                          largest_component_sizes=sizes[:10], sizes_are_of=("all components" if full else "the kept segments"),
                          frame_segments_wall_ms_median=round(float(np.median(ms)), 3),
                          frame_segments_wall_ms_iqr=round(float(np.subtract(*np.percentile(ms, [75, 25]))), 3)))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concave.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="run this one step in this process and print its JSON (what the driver starts)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_concave.py needs a HIP device")
    if args.step:
        res = step_frame_segments() if args.step == "frame_segments" else step_routes(args.step, args.reps)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    device = torch.cuda.get_device_name(0)
    parts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS.items():
            piece = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--out", piece]
            rc = subprocess.run(cmd).returncode
            if rc != 0:                                                        # a failure, a time limit or a fault: nothing more is started
                raise SystemExit(f"step {step} ended with status {rc}; stopping")
            parts[step] = json.load(open(piece))
            print(json.dumps(parts[step]), flush=True)
    from cppf_amd import segments as SG
    out = dict(device=device, reps_per_route=args.reps,
               method="one process per step, each under its own time limit; the routes alternate repetition by repetition after a warm-up, HIP "
                      "events around each repetition (host launch path and the allocations of the outputs included); outputs compared first",
               rule="'faster' only where the baseline's median exceeds the new route's by more than the baseline's inter-quartile range",
               options=SG.concave_options(), rows=[parts["demo_frame"], parts["tabletop_frame"]], demo_frame_table=parts["frame_segments"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
