"""fp32 against bf16 point encoder (PointEncoder.set_precision), timed with HIP events, the method of scripts/bench_precision.py
(DESIGN.md 3.1a): per shape ONE process runs every precision setting, the settings alternating in blocks of 40 calls after a warm-up
so that drift of the shared machine hits all alike; 240 timed calls per setting; median and inter-quartile range of the per-call
times.

  a. point_encoder_forward_batch on the reference-default batch: 8 clouds of 700-2000 points, k = 60, the committed trained
     networks -- once with the neighbour search in the call (three launches) and once with the neighbour sets already there
     (convolution + GlobalInfoProp fill: the two launches the precision touches)
  b. one cloud of N = 4096, k = 60: convolution + fill
  (a and b also as captured graphs, replayed: at these sizes the host's launch path is as long as the kernels)
  c. the demo frame (tests/golden/demo_0000_depth.png, six instances) through FrameRunner.run, per frame, in three settings:
     both encoders fp32, the point encoder alone in bf16, both in bf16

The baseline is the fp32 path of the same process.  bf16 counts as faster at a shape only where the fp32 median exceeds the bf16
median by more than the fp32 inter-quartile range of that run.  Every shape runs in a child process of its own under a time limit;
after a child that failed or ran out of time nothing more is started.  Writes profiles/bf16_point_encoder.json.  Needs a HIP
device; there is no fall-back.

    python scripts/bench_point_precision.py [--launches 240] [--out profiles/bf16_point_encoder.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = {"a": 300, "b": 180, "c": 420}          # shape -> its time limit in seconds
SIZES = [717, 1203, 1890, 960, 1544, 1333, 1777, 2000]
RULE = "bf16 counts as faster only if the fp32 median exceeds the bf16 median by more than the fp32 inter-quartile range of this run"


def alternate(run, apply, settings, launches, block=40, warmup=20):
    """run() under every setting in alternating blocks of `block` calls (a warm-up after every switch) -> {setting: [ms]}"""
    import torch
    from bench_precision import timed
    ts = {s: [] for s in settings}
    while len(ts[settings[-1]]) < launches:
        for s in settings:
            apply(s)
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            ts[s] += timed(run, block)
    return ts


def replays(fn, apply, settings, launches):
    """the same comparison on captured graphs of fn() -- one per setting, replayed: the device time of the launches without the
    host's launch path (which at these sizes is as long as the kernels)"""
    import torch
    graphs = {}
    for s in settings:
        apply(s)
        fn()
        torch.cuda.synchronize()
        graphs[s] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[s]):
            fn()
    cur = [None]
    return alternate(lambda: cur[0].replay(), lambda s: cur.__setitem__(0, graphs[s]), settings, launches)


def verdicts(ts, baseline="fp32"):
    from bench_precision import stats
    r = {s: stats(t) for s, t in ts.items()}
    for s in ts:
        if s != baseline:
            r[s]["fp32_over_this"] = round(r[baseline]["median_us"] / r[s]["median_us"], 3)
            r[s]["faster_than_fp32"] = bool(r[baseline]["median_us"] - r[s]["median_us"] > r[baseline]["iqr_us"])
    r["rule"] = RULE
    return r


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    th, h = rng.uniform(0, 2 * np.pi, n), rng.uniform(-0.15, 0.15, n)
    pc = (np.stack([0.05 * np.cos(th), h, 0.05 * np.sin(th)], -1) + rng.normal(0, 1e-3, (n, 3))).astype(np.float32)
    nrm = np.stack([np.cos(th), np.zeros(n), np.sin(th)], -1) + rng.normal(0, 0.05, (n, 3))
    return pc, (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)


def trained(dev):
    import cppf_amd.synthetic as syn
    from cppf_amd import training
    return {c: training.load_weights(os.path.join(GOLDEN, f"trained_{c}.npz"), syn.CATEGORIES[c], dev) for c in ("bottle", "mug", "laptop")}


def shape_a(dev, launches):
    import torch
    from cppf_amd.models.model import point_encoder_forward_batch
    nets = trained(dev)
    pencs = [nets[("bottle", "mug", "laptop")[i % 3]][0] for i in range(len(SIZES))]
    members = []
    for i, n in enumerate(SIZES):
        pc, nrm = cloud(n, 900 + i)
        cap = 1024 if n <= 1024 else 2048
        pcd, nrmd = torch.zeros((cap, 3), device=dev), torch.zeros((cap, 3), device=dev)
        pcd[:n], nrmd[:n] = torch.from_numpy(pc).to(dev), torch.from_numpy(nrm).to(dev)
        members.append(dict(encoder=pencs[i], pc=pcd, nrm=nrmd, n_dev=torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev),
                            out=torch.zeros((cap, 40), device=dev), nbrs=torch.zeros((cap, 60), dtype=torch.int32, device=dev)))

    def apply(prec):
        for e in set(pencs):
            e.set_precision(prec)._packed_weights(dev)

    out = {}
    with torch.no_grad():
        point_encoder_forward_batch(members)                  # (leaves every member's neighbour sets in place)
        for key, ready in (("search_conv_fill", False), ("conv_fill", True)):
            ms = [dict(m, nbrs_ready=ready) for m in members]
            out[key] = verdicts(alternate(lambda: point_encoder_forward_batch(ms), apply, ("fp32", "bf16"), launches))
            out[key + "_graph"] = verdicts(replays(lambda: point_encoder_forward_batch(ms), apply, ("fp32", "bf16"), launches))
    out["what"] = (f"point_encoder_forward_batch, 8 clouds of {min(SIZES)}-{max(SIZES)} points in 1024 / 2048 buckets, k = 60, trained networks; "
                   "search_conv_fill: neighbour search + convolution + fill (3 launches), conv_fill: neighbour sets ready (2 launches); "
                   "HIP events around each call (host launch path included); *_graph: the same launches as a captured graph, replayed")
    return out


def shape_b(dev, launches):
    import torch
    penc = trained(dev)["bottle"][0]
    pc, nrm = cloud(4096, 5)
    pcd, nrmd = torch.from_numpy(pc).to(dev), torch.from_numpy(nrm).to(dev)
    with torch.no_grad():
        nbrs = penc.neighbours(pcd)
        apply = lambda p: penc.set_precision(p)._packed_weights(dev)
        out = dict(call=verdicts(alternate(lambda: penc._forward_device(pcd, nrmd, nbrs), apply, ("fp32", "bf16"), launches)),
                   graph=verdicts(replays(lambda: penc._forward_device(pcd, nrmd, nbrs), apply, ("fp32", "bf16"), launches)))
    out["what"] = "one cloud of N = 4096, k = 60, trained bottle network: convolution + fill (neighbour sets ready); call: HIP events around each call, graph: the same launches captured and replayed"
    return out


def shape_c(dev, launches):
    import cppf_amd.synthetic as syn
    from cppf_amd import training
    from cppf_amd.frames import FrameRunner
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))
    rects = [("mug", (262, 356), (124, 206), 90), ("bowl", (184, 246), (288, 366), 90), ("bowl", (194, 250), (370, 442), 90),
             ("mug", (186, 250), (436, 504), 90), ("can", (112, 184), (376, 408), 60), ("laptop", (118, 322), (92, 302), 260)]
    inst = []
    for cat, (r0, r1), (c0, c1), win in rects:
        msk = np.zeros(depth.shape, bool)
        patch = depth[r0:r1, c0:c1]
        msk[r0:r1, c0:c1] = np.abs(patch.astype(np.int64) - np.median(patch[patch > 0])) <= win
        inst.append((cat, msk))
    src = {"mug": "mug", "laptop": "laptop", "bowl": "bottle", "can": "bottle"}           # (bottle weights stand in for bowl / can)
    nets = {c: training.load_weights(os.path.join(GOLDEN, f"trained_{w}.npz"), syn.CATEGORIES[w], dev) for c, w in src.items()}
    encs, pencs = {c: v[1] for c, v in nets.items()}, {c: v[0] for c, v in nets.items()}
    runner = FrameRunner(encs, pencs, dev)
    settings = {"fp32": ("fp32", "fp32"), "point_bf16": ("bf16", "fp32"), "both_bf16": ("bf16", "bf16")}

    def apply(s):
        for c in encs:
            pencs[c].set_precision(settings[s][0])
            encs[c].set_precision(settings[s][1])
        for _ in range(4):                                     # (the precision is part of the graph key: captured again after a switch)
            runner.run(depth, inst)

    for s in settings:                                         # first sighting, capture of the chains, their slow first replays
        apply(s)
    out = verdicts(alternate(lambda: runner.run(depth, inst), apply, tuple(settings), launches, warmup=5))
    out["what"] = ("FrameRunner.run on the demo frame, six instances, 100 000 pairs each: upload, captured chains, one read-back; per "
                   "frame, HIP events around each call; point_bf16: point encoder bf16, pair encoder fp32")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=240, help="timed calls per precision setting")
    ap.add_argument("--shape", choices=sorted(SHAPES), help="run one shape in this process and print its JSON (what the parent starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_point_encoder.json"))
    args = ap.parse_args()
    if args.shape:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_point_precision.py needs a HIP device")
        r = {"a": shape_a, "b": shape_b, "c": shape_c}[args.shape](torch.device("cuda:0"), args.launches)
        r["device"] = torch.cuda.get_device_name(0)
        print("RESULT " + json.dumps(r))
        return
    out = dict(launches_per_setting=args.launches, method="one process per shape, HIP events around every call, settings alternating in "
               "blocks of 40 after a warm-up", rule=RULE)
    names = {"a": "reference_default_batch", "b": "one_cloud_4096", "c": "demo_frame"}
    for s, limit in SHAPES.items():      # (the parent never opens the device: one process with the GPU open at a time)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", s, "--launches", str(args.launches)], timeout=limit,
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise SystemExit(f"shape {s} ended with status {p.returncode}: nothing more is started")
        r = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
        out["device"] = r.pop("device")
        out[names[s]] = r
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
