#!/usr/bin/env python3
"""The reference's gen_stats.py on the device: voting statistics of a category from its meshes (cppf_amd.mesh_stats), printed in
gen_stats.py's three lines.  --meshes is a directory (every *.obj under it) or a names file of data/shapenet_names/*.txt's form
(resolved against --shapenet-root).  With --write-config the derived category file is written too (mesh_stats.derive_config:
vote_range and scale_mean scaled by --scale-range the way the training views scale the meshes), ready for
scripts/train_meshes.py --config:

    python scripts/gen_stats.py --meshes my_meshes/
    python scripts/gen_stats.py --meshes my_meshes/ --write-config mycat.yaml --category mycat --res 5e-3 --scale-range 0.2 0.4
    python scripts/train_meshes.py --category mycat --config mycat.yaml --meshes my_meshes/ --steps 2000
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cppf_amd import config, mesh_stats, meshes     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", required=True, help="directory of OBJ files, or a names file (<synset>/<model> per line)")
    ap.add_argument("--shapenet-root", default=None, help="where the names of a names file live (default: the file's directory)")
    ap.add_argument("--seed", type=int, default=0, help="Philox key of the surface samples and pairs")
    ap.add_argument("--n-samples", type=int, default=2048, help="points per mesh (gen_stats.py: 2048)")
    ap.add_argument("--n-pairs", type=int, default=100000, help="pairs per mesh (gen_stats.py: 100000)")
    ap.add_argument("--write-config", default=None, metavar="OUT.yaml", help="also write the derived category file")
    ap.add_argument("--category", default=None, help="the category's name (with --write-config)")
    ap.add_argument("--res", type=float, default=None, help="voxel size / vote grid cell (with --write-config)")
    ap.add_argument("--scale-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="object scale drawn per training view (with --write-config)")
    ap.add_argument("--up-sym", action="store_true", help="the objects look like a cylinder from up to bottom")
    ap.add_argument("--right-sym", action="store_true", help="the objects look like a cylinder from left to right")
    ap.add_argument("--z-right", action="store_true", help="the right axis is [0, 0, 1] (default [1, 0, 0])")
    ap.add_argument("--regress-right", action="store_true", help="predict the right axis too")
    args = ap.parse_args()
    if args.write_config and (args.category is None or args.res is None or args.scale_range is None):
        ap.error("--write-config needs --category, --res and --scale-range")
    paths = meshes.mesh_paths(args.meshes, args.shapenet_root)
    missing = [p for p in paths if not os.path.exists(p)]
    if not paths or missing:
        sys.exit(f"no meshes under {args.meshes}" if not paths else f"{len(missing)} listed meshes are missing, e.g. {missing[0]}")
    stats = mesh_stats.category_stats(paths, n_samples=args.n_samples, n_pairs=args.n_pairs, seed=args.seed,
                                      device=torch.device("cuda", 0))
    print(mesh_stats.format_stats(stats))
    if args.write_config:
        cfg = mesh_stats.derive_config(args.category, stats, args.res, args.scale_range, up_sym=args.up_sym, right_sym=args.right_sym,
                                       z_right=args.z_right, regress_right=args.regress_right)
        config.save_category_yaml(cfg, args.write_config)
        print(f"wrote {args.write_config}: vote_range {cfg.vote_range} scale_mean {cfg.scale_mean} scale_range {cfg.scale_range}",
              file=sys.stderr)


if __name__ == "__main__":
    main()
