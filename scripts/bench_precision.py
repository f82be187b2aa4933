"""fp32 against bf16 pair encoder (PPFEncoder.set_precision), timed in ONE process with HIP events.

1. The batched first-pass launch at the headline shape -- 4 pair lists of N = 4096 points, K = 128 pairs per point
   (models.model.forward_decode_batch: one point-projection launch + one pair-kernel launch) -- in both precisions, the two
   alternating in blocks so that drift of the shared machine hits both alike: warm-up, then >= 200 timed launches each; median and
   spread (inter-quartile range, min, max) of the per-launch times.
2. The trained-regime step (the centre chain of the committed bottle network on one held-out posed object, bench_util.make_trained_set:
   pair kernel + vote + arg-max as one captured graph), both ways, the same way.

bf16 counts as faster only where its median beats fp32's by more than the fp32 spread (IQR) measured in the same run.
Writes profiles/bf16_pair_encoder.json.  Needs a HIP device; there is no fall-back.

    python scripts/bench_precision.py [--launches 240] [--out profiles/bf16_pair_encoder.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cppf_amd.synthetic as syn                                       # noqa: E402
from bench_util import make_trained_set                                # noqa: E402
from cppf_amd.models.model import PPFEncoder, forward_decode_batch     # noqa: E402


def stats(ts):
    ts = np.sort(np.asarray(ts, np.float64))
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return dict(n=int(ts.size), median_us=round(float(med) * 1e3, 2), iqr_us=round(float(q3 - q1) * 1e3, 2),
                min_us=round(float(ts[0]) * 1e3, 2), max_us=round(float(ts[-1]) * 1e3, 2))


def timed(fn, n):
    """n calls of fn, each between its own pair of events on the current stream -> ms per call"""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def alternate(run, set_precision, launches, block=40, warmup=20):
    """run() under fp32 and bf16 in alternating blocks of `block` launches (a warm-up after every switch) -> {precision: [ms]}"""
    ts = {"fp32": [], "bf16": []}
    while len(ts["bf16"]) < launches:
        for prec in ("fp32", "bf16"):
            set_precision(prec)
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            ts[prec] += timed(run, block)
    return ts


def verdict(r):
    gain = r["fp32"]["median_us"] - r["bf16"]["median_us"]
    r["fp32_over_bf16"] = round(r["fp32"]["median_us"] / r["bf16"]["median_us"], 3)
    r["bf16_faster"] = bool(gain > r["fp32"]["iqr_us"])
    r["rule"] = "bf16 counts as faster only if the fp32 median exceeds the bf16 median by more than the fp32 inter-quartile range of this run"
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=240, help="timed launches per precision (at least 200)")
    ap.add_argument("--lists", type=int, default=4)
    ap.add_argument("--n-points", type=int, default=4096)
    ap.add_argument("--pairs-per-point", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_pair_encoder.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_precision.py needs a HIP device")
    launches = max(args.launches, 200)
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # ---- 1. the batched first-pass launch, headline shape
    torch.manual_seed(0)
    items, encs = [], []
    for i in range(args.lists):
        ob = syn.make_object("bottle", args.n_points, i)
        enc = PPFEncoder(ob["cfg"].ppffcs, ob["cfg"].out_dim).to(dev).eval()
        idx = syn.make_pairs(args.n_points, args.pairs_per_point, i)
        u_tr, _ = syn.make_uniforms(idx.shape[0], i)
        items.append(dict(encoder=enc, pc=d(ob["pc"]), pc_normal=d(ob["normals"]), feat=d(ob["feat"]), idxs=d(idx), u_tr=d(u_tr),
                          vote_range=ob["cfg"].vote_range))
        encs.append(enc)

    def set_all(prec):
        for e in encs:
            e.set_precision(prec)
            e._packed_weights(dev)

    with torch.no_grad():
        ts = alternate(lambda: forward_decode_batch(items), set_all, launches)
    pairs = args.lists * args.n_points * args.pairs_per_point
    first = verdict({p: stats(t) for p, t in ts.items()})
    first["what"] = (f"forward_decode_batch, centre heads: {args.lists} lists of N = {args.n_points}, K = {args.pairs_per_point} "
                     f"({pairs} pairs); point projection + pair kernel, HIP events around each call (host launch path included)")

    # ---- 2. the trained-regime step: the captured centre chain of the committed bottle network
    # (ONE held-out object: rotating over several would put their different vote costs into the spread)
    objs, _, enc_t = make_trained_set(dev, args.n_points, args.pairs_per_point, 1, 900100, rotate=False)
    pipe = objs[0]["pipe"]

    def step():
        pipe.run(check_weights=False)

    def set_trained(prec):
        enc_t.set_precision(prec)
        pipe.run()                             # (the precision is part of the graph key: captured again on the first run after a switch)

    ts = alternate(step, set_trained, launches)
    trained = verdict({p: stats(t) for p, t in ts.items()})
    trained["what"] = (f"CenterPipeline.run (captured graph: pair kernel + centre vote + arg-max), trained bottle network, one held-out posed "
                       f"object, N = {args.n_points}, K = {args.pairs_per_point}; one instance at a time")

    out = dict(device=torch.cuda.get_device_name(0), launches_per_precision=launches, first_pass_batch=first, trained_regime_step=trained)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
