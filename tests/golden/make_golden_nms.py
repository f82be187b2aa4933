#!/usr/bin/env python3
"""Generate tests/golden/nms_cases.npz: what the reference's own 3D non-maximum suppression picks on seeded random oriented boxes
(build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nms.py /root/reference

`sunrgbd/eval.py` cannot be imported here (its other imports need SUN RGB-D's packages), so its two functions `iou_3d` and `nms`
(:13-35) are taken from it at generation time: the file is parsed, the two function definitions are compiled AS THEY ARE into a
namespace that holds what they use (numpy and the reference's own utils.iou.IoU, which does import).  Nothing of the reference is
written to the repository: the stored DATA are the synthetic inputs and the values those functions return, per case k --
  RT_k f64[M,4,4], scales_k f64[M,3], scores_k f64[M], thresh_k,
  pick_k   the list `nms(boxes, scores, thresh)` returns, boxes = Box.from_transformation(R, t, scales) as sunrgbd/eval.py:122,
  iou_k    `iou_3d(boxes[i], boxes[j])` for i < j, row by row.
Cases: M = 1, 2, 33, 64, 65, 130; random rotations, centres uniform in a cube of side 0.4 .. 3 (SIDES), extents uniform in
[0.5, 1.5]; scores a permutation plus a uniform draw in [0, 0.5) -- distinct; thresh 0.3.
Every stored case has distinct scores and no pair with |IoU - thresh| < 1e-6 (asserted; a case that misses is drawn again): with
that margin, far above the disagreement of any two implementations of the IoU, the pick list is a discrete function on which the
reference, the host path and the device must agree exactly.
"""
import ast
import contextlib
import io
import os
import sys

import numpy as np

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
out_dir = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, ref)

from utils.box import Box  # noqa: E402
from utils.iou import IoU  # noqa: E402

WANT = {"iou_3d", "nms"}
path = os.path.join(ref, "sunrgbd", "eval.py")
tree = ast.parse(open(path).read())
ns = {"np": np, "IoU": IoU}
mod = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT], type_ignores=[])
assert {n.name for n in mod.body} == WANT
exec(compile(mod, path, "exec"), ns)

SIZES = (1, 2, 33, 64, 65, 130)
SIDES = (0.4, 0.4, 1.2, 1.6, 1.6, 3.0)                          # the cube of the centres: crowded enough that boxes are suppressed
THRESH = 0.3
MARGIN = 1e-6


def rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def draw(rng, M, side):
    RT = np.tile(np.eye(4), (M, 1, 1))
    for k in range(M):
        RT[k, :3, :3] = rot(rng)
    RT[:, :3, 3] = rng.uniform(-0.5 * side, 0.5 * side, size=(M, 3))
    scales = rng.uniform(0.5, 1.5, size=(M, 3))
    scores = rng.permutation(M).astype(np.float64) + rng.uniform(0.0, 0.5, size=M)
    return RT, scales, scores


def run(RT, scales, scores):
    boxes = [Box.from_transformation(RT[k, :3, :3], RT[k, :3, 3], scales[k]) for k in range(len(RT))]
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):                       # (iou_3d prints what it catches)
        pick = ns["nms"](boxes, scores, THRESH)
        iou = np.array([ns["iou_3d"](boxes[i], boxes[j]) for i in range(len(boxes)) for j in range(i + 1, len(boxes))], np.float64)
    assert sink.getvalue() == "", "the reference's IoU raised on a case: " + sink.getvalue()[:200]
    return np.asarray(pick, np.int64), iou


rng = np.random.default_rng(20251019)
out = {"n_cases": np.int64(len(SIZES))}
for k, (M, side) in enumerate(zip(SIZES, SIDES)):
    while True:
        RT, scales, scores = draw(rng, M, side)
        pick, iou = run(RT, scales, scores)
        if len(np.unique(scores)) == M and (len(iou) == 0 or np.abs(iou - THRESH).min() >= MARGIN):
            break
    assert len(np.unique(scores)) == M and (len(iou) == 0 or np.abs(iou - THRESH).min() >= MARGIN)
    out.update({f"RT_{k}": RT, f"scales_{k}": scales, f"scores_{k}": scores, f"thresh_{k}": np.float64(THRESH), f"pick_{k}": pick,
                f"iou_{k}": iou})
    print(f"case {k}: M {M}, picked {len(pick)}, min |IoU - thresh| {np.abs(iou - THRESH).min() if len(iou) else float('nan'):.3g}, "
          f"pairs above thresh {int((iou > THRESH).sum())}")
dst = os.path.join(out_dir, "nms_cases.npz")
np.savez_compressed(dst, **out)
assert os.path.getsize(dst) < 300 * 1024
print(dst, os.path.getsize(dst), "bytes")
