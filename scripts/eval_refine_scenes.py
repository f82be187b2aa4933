#!/usr/bin/env python3
"""Per-object pose errors of the refinement stage on scenes with a known answer (the two-bottle scene and the bottle + mug scene of
tests/test_gpu_refine.py, committed trained networks): first pass | refined | the instance path on the TRUE instance cloud (the scene
builder's membership; the same networks, n_pairs and seed -- the yardstick, not the code under test).  Centre error in cells, up and
right error in degrees modulo sign, largest relative scale error.  Written to profiles/refine_eval.json (--out) under `objects`,
beside the AP tables scripts/eval_mesh_frames.py --mask-free --refine puts there.  Figures, no threshold.

    python scripts/eval_refine_scenes.py [--seed 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_eval.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_refine_scenes.py runs on a HIP device: none found")
    import test_gpu_refine as T
    rows = T.scene_error_rows(torch.device("cuda", 0), seed=args.seed)
    objects = [dict(scene=name, category=cat, object=oid, first_pass=first, refined=refined, true_cloud_instance_path=true)
               for name, cat, oid, first, refined, true in rows]
    for o in objects:
        print(json.dumps(o))
    rec = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            rec = json.load(fh)
    rec["objects"] = dict(device=torch.cuda.get_device_name(0), seed=args.seed, n_pairs=T.N_PAIRS, thresh=T.TS.TRAINED_THRESH,
                          columns="t_cells, up_deg_mod_sign, right_deg_mod_sign, scale_rel (training.pose_errors)", rows=objects)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
