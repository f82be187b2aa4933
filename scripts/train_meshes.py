#!/usr/bin/env python3
"""Train the two networks of train.py:34-35 for one category on training views of OBJ meshes (cppf_amd.meshes.MeshViewSampler:
the sample of utils/dataset.py:103-250 rendered on the device), save the weights in training.save_weights's format and print the
loss curve.  --meshes is a directory (every *.obj under it: a ShapeNet synset directory gives its
<model>/models/model_normalized.obj files) or a names file in the format of data/shapenet_names/*.txt (`<synset>/<model>` per
line, resolved against --shapenet-root):

    python scripts/train_meshes.py --category bottle --meshes ShapeNetCore.v2/02876657 --steps 20000 --out bottle.npz
    python scripts/train_meshes.py --category bottle --meshes data/shapenet_names/bottle.txt --shapenet-root ShapeNetCore.v2

A category outside cppf_amd.config.CATEGORIES trains from a category file (the flat form of config/category/*.yaml, e.g. written
by scripts/gen_stats.py --write-config):

    python scripts/train_meshes.py --category mycat --config mycat.yaml --meshes my_meshes/ --steps 2000
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cppf_amd import config, meshes, training     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--category", required=True)
    ap.add_argument("--meshes", required=True, help="directory of OBJ files, or a names file (<synset>/<model> per line)")
    ap.add_argument("--shapenet-root", default=None, help="where the names of a names file live (default: the file's directory)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--n-pairs", type=int, default=60000)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="weights file (default: trained_<category>_meshes.npz)")
    ap.add_argument("--config", default=None, help="category file (flat YAML of config/category/*.yaml) in place of the built-in one")
    args = ap.parse_args()
    cfg = config.load_category_yaml(args.config) if args.config else None
    if cfg is not None and cfg.category != args.category:
        sys.exit(f"{args.config} is for category {cfg.category!r}, not {args.category!r}")
    if cfg is None and args.category not in config.CATEGORIES:
        sys.exit(f"category {args.category!r} has no built-in config: pass --config FILE.yaml (scripts/gen_stats.py --write-config)")
    paths = meshes.mesh_paths(args.meshes, args.shapenet_root)
    missing = [p for p in paths if not os.path.exists(p)]
    if not paths or missing:
        sys.exit(f"no meshes under {args.meshes}" if not paths else f"{len(missing)} listed meshes are missing, e.g. {missing[0]}")
    dev = torch.device("cuda", 0)
    print(f"{args.category}: {len(paths)} meshes")
    t0 = time.perf_counter()
    penc, enc, losses = training.train_on_meshes(args.category, paths, dev, steps=args.steps, n_pairs=args.n_pairs, lr=args.lr,
                                                 seed=args.seed, log=print, cfg=cfg)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = args.out or f"trained_{args.category}_meshes.npz"
    training.save_weights(out, penc, enc, meta=dict(steps=args.steps, n_pairs=args.n_pairs, lr=args.lr, n_meshes=len(paths),
                                                    final_loss=losses[-1]))
    print(json.dumps(dict(category=args.category, steps=args.steps, seconds=dt, weights=out,
                          loss_curve=[float(np.round(x, 5)) for x in losses])))


if __name__ == "__main__":
    main()
