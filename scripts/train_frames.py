#!/usr/bin/env python3
"""Train the two networks of one category on WHOLE frames (cppf_amd.scene_training.train_on_frames): every step renders
a frame of several posed meshes (mesh_frames.MeshFrameSampler), runs SPRIN on the frame's dense cloud, draws pairs over the frame's
sparse cloud -- a share of them inside single instances of the category -- and takes the loss of train.py:68-87 over those.  Writes
training.save_weights' file, which scripts/eval_mesh_frames.py --weights CATEGORY=FILE reads as it stands.

Meshes: --meshes CATEGORY=DIR|NAMES (repeatable; the frames mix all categories given, --category names the one whose networks are
trained), or --procedural for the procedural bottles / cans / cameras scripts/eval_mesh_frames.py evaluates on.

    python scripts/train_frames.py --category bottle --procedural --objects 4 --steps 3000 --out bottle_frames.npz
    python scripts/train_frames.py --category bottle --procedural --steps 3000 --neg-weight 0.25 --out bottle_frames_neg.npz

--sampler-seed (default 5000) seeds the frames; scripts/eval_mesh_frames.py draws its frames from --seed (default 0) and its tuning
frames from --seed + 1000, so the default trains on frames the evaluation never sees.  Both seeds go into the file's meta."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cppf_amd import mesh_frames as MF                 # noqa: E402
from cppf_amd import meshes as M                       # noqa: E402
from cppf_amd import scene_training, training          # noqa: E402
from cppf_amd.config import CATEGORIES                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--category", required=True, help="the category whose networks are trained")
    ap.add_argument("--meshes", action="append", help="CATEGORY=directory of OBJ files or names file (repeatable)")
    ap.add_argument("--shapenet-root", default=None)
    ap.add_argument("--procedural", action="store_true", help="procedural bottle / can / camera meshes instead of --meshes")
    ap.add_argument("--objects", type=int, default=4, help="objects per frame")
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--n-pairs", type=int, default=200000, help="pairs drawn per step")
    ap.add_argument("--pos-frac", type=float, default=0.5, help="share of the pairs drawn inside single instances of the category")
    ap.add_argument("--neg-weight", type=float, default=0.0, help="weight of the negatives' nu term (0: negatives are ignored)")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0, help="initialisation and pair draws")
    ap.add_argument("--sampler-seed", type=int, default=5000, help="the frames (the evaluation uses 0 and 1000)")
    ap.add_argument("--out", default=None, help="weights file (default: trained_<category>_frames.npz)")
    args = ap.parse_args()
    from eval_mesh_frames import _pairs, _procedural
    tmp = tempfile.TemporaryDirectory()
    if args.procedural:
        cat_paths = _procedural(tmp.name)
    else:
        cat_paths = {c: M.mesh_paths(p, args.shapenet_root) for c, p in _pairs(args.meshes, "meshes").items()}
    if not cat_paths or not all(cat_paths.values()):
        sys.exit("no meshes: --meshes CATEGORY=DIR (repeatable) or --procedural")
    if args.category not in cat_paths:
        sys.exit(f"--category {args.category}: no meshes of it among {sorted(cat_paths)}")
    for c in cat_paths:
        if c not in CATEGORIES:
            sys.exit(f"category {c!r} has no built-in config")
    dev = torch.device("cuda", 0)
    sampler = MF.MeshFrameSampler(cat_paths, args.objects, device=dev, seed=args.sampler_seed)
    t0 = time.perf_counter()
    penc, enc, losses, skipped = scene_training.train_on_frames(args.category, sampler, dev, steps=args.steps, n_pairs=args.n_pairs,
                                                                pos_frac=args.pos_frac, neg_weight=args.neg_weight, lr=args.lr,
                                                                seed=args.seed, log=print)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = args.out or f"trained_{args.category}_frames.npz"
    training.save_weights(out, penc, enc, meta=dict(steps=args.steps, n_pairs=args.n_pairs, lr=args.lr, objects=args.objects,
                                                    pos_frac=args.pos_frac, neg_weight=args.neg_weight, seed=args.seed,
                                                    sampler_seed=args.sampler_seed, skipped_frames=skipped,
                                                    final_loss=losses[-1] if losses else float("nan")))
    print(json.dumps(dict(category=args.category, steps=args.steps, trained_steps=len(losses), skipped_frames=skipped, seconds=dt,
                          weights=out, seed=args.seed, sampler_seed=args.sampler_seed,
                          loss_curve=[float(np.round(x, 5)) for x in losses[::20]])))
    tmp.cleanup()


if __name__ == "__main__":
    main()
