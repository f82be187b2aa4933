#!/usr/bin/env python3
"""The accuracy table of DESIGN.md 3.7l: scripts/eval_mesh_frames.py --tabletop with 3.7i / 3.7j's settings (procedural bottle / can /
camera meshes, networks frame-trained by scripts/train_frames.py for 3 000 steps of 200 000 pairs with --neg-weight 0.25, --seed S
--sampler-seed 5000 + S; 20 frames of 4 objects, 1 000 000 scene pairs, 6 proposals per category), per training seed and per
--min-gap, in six rows:

  masked            the instance path on the ground-truth masks
  uniform           --mask-free
  segments          --mask-free --segments                       (0 planes)
  plane             --mask-free --segments --planes 1
  concave           --mask-free --segments --concave
  plane+concave     --mask-free --segments --planes 1 --concave

--segment-instances [--planes N] [--concave] [--select best|all] [--score agreement|peak] adds a seventh row,

  segment-instances scripts/eval_mesh_frames.py --segment-instances with those flags: the segments as instance masks, no scene stage

whose record holds the four select / score variants pooled from the same candidates; with the flag --rows defaults to masked, plane
and segment-instances and --out to profiles/segment_instances_eval.json.  Without the flag the script does what it always did.

Every training and every evaluation is a child process under its own time limit; the first that fails, hangs or faults ends the run.
The records of the runs go into --out (profiles/tabletop_eval.json) under "<seed>/<min_gap>/<row>"; an existing file is extended, so the
seeds may be run one call at a time.  Weights are kept in --work and reused when they are there.  Needs a HIP device.

    python scripts/eval_tabletop.py --seeds 0 1 --gaps 0 0.05 [--work tabletop_work] [--out profiles/tabletop_eval.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = ("bottle", "can", "camera")
ROWS = {"masked": [], "uniform": ["--mask-free"], "segments": ["--mask-free", "--segments"],
        "plane": ["--mask-free", "--segments", "--planes", "1"], "concave": ["--mask-free", "--segments", "--concave"],
        "plane+concave": ["--mask-free", "--segments", "--planes", "1", "--concave"]}
KEEP = ("frames", "objects_per_frame", "scene_pairs", "max_proposals", "ground_truths", "proposals", "instances_run", "ms_per_frame_median",
        "iou_ap", "pose_ap", "segments", "tabletop", "n_pairs", "timed_variant", "segments_per_frame", "candidates_per_frame", "refused_per_frame",
        "skipped_min_points_per_frame", "detections_per_frame", "objects_with_a_segment", "best_picked_the_true_category", "variants")


def run(cmd, limit):
    rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
    if rc != 0:
        raise SystemExit(f"{' '.join(cmd[1:4])} ... ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1], help="training seeds (the frames of training: sampler seed 5000 + seed)")
    ap.add_argument("--gaps", type=float, nargs="+", default=[0.0, 0.05], help="--min-gap values: 0 lets objects touch")
    ap.add_argument("--rows", nargs="+", default=None, choices=list(ROWS) + ["segment-instances"])
    ap.add_argument("--segment-instances", action="store_true", help="add the row of detections.segment_detections (DESIGN.md 3.7m)")
    ap.add_argument("--planes", type=int, default=1, help="--segment-instances: planes removed before the labelling")
    ap.add_argument("--concave", action="store_true", help="--segment-instances: cut at the concave creases as well")
    ap.add_argument("--select", choices=("best", "all"), default="best", help="--segment-instances: the timed run's selection")
    ap.add_argument("--score", choices=("agreement", "peak"), default="agreement", help="--segment-instances: the timed run's score")
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--work", default=os.path.join(ROOT, "tabletop_work"))
    ap.add_argument("--out", default=None, help="default profiles/tabletop_eval.json (profiles/segment_instances_eval.json with "
                    "--segment-instances)")
    args = ap.parse_args()
    rows = dict(ROWS)
    if args.segment_instances:
        rows["segment-instances"] = (["--segment-instances", "--planes", str(args.planes), "--select", args.select, "--score", args.score]
                                     + (["--concave"] if args.concave else []))
    if args.rows is None:
        args.rows = ["masked", "plane", "segment-instances"] if args.segment_instances else list(ROWS)
    if "segment-instances" in args.rows and not args.segment_instances:
        sys.exit("the row segment-instances needs --segment-instances")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "segment_instances_eval.json" if args.segment_instances else "tabletop_eval.json")
    os.makedirs(args.work, exist_ok=True)
    out = json.load(open(args.out)) if os.path.exists(args.out) else dict(
        settings="procedural bottle / can / camera; scripts/train_frames.py --steps 3000 --neg-weight 0.25 --seed S --sampler-seed 5000+S; "
                 "scripts/eval_mesh_frames.py --tabletop --frames 20 --objects 4 (evaluation seed 0), 1 000 000 scene pairs, 6 proposals",
        note="figures: no threshold is attached to these APs", runs={})
    for seed in args.seeds:
        weights = []
        for cat in CATS:
            w = os.path.join(args.work, f"{cat}_frames_neg_s{seed}.npz")
            if not os.path.exists(w):
                run([sys.executable, os.path.join(ROOT, "scripts", "train_frames.py"), "--category", cat, "--procedural", "--steps", str(args.steps),
                     "--neg-weight", "0.25", "--seed", str(seed), "--sampler-seed", str(5000 + seed), "--out", w], 420)
            weights += ["--weights", f"{cat}={w}"]
        for gap in args.gaps:
            for row in args.rows:
                piece = os.path.join(args.work, f"s{seed}_g{gap}_{row}.json")
                run([sys.executable, os.path.join(ROOT, "scripts", "eval_mesh_frames.py"), "--procedural", *weights, "--frames", str(args.frames),
                     "--objects", "4", "--tabletop", "--min-gap", str(gap), *rows[row], "--out", piece], 300)
                rec = json.load(open(piece))
                out["runs"][f"{seed}/{gap}/{row}"] = {k: rec[k] for k in KEEP if k in rec}
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:                                 # after every run: what was measured is kept
                    json.dump(out, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
