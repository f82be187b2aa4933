#!/usr/bin/env python3
"""tests/golden/zero_shot.npz from the reference's own nocs/zero_shot.ipynb (run in the build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_zero_shot.py /root/reference

The proposal cell (cell 9: scipy.ndimage.gaussian_filter, then the peak loop) and the segmentation lines of cell 11 are read
from the notebook at generation time and exec'd with the real numpy / scipy; this script holds none of their text.  The loop
is capped (its `while True:` becomes a bounded `for`): with a peak on the last plane of an axis the notebook never ends.  Cases:
several blobs, a peak on a last plane, nothing above the threshold, thin axes (a size-1 axis makes the notebook raise) --
inputs, a hash of the smoothed grid and the proposals (with the notebook's repeats as they came) are recorded; then a few
random survivor lists through the segmentation.  Only data is written."""
import hashlib
import json
import os
import sys

import numpy as np
from scipy.ndimage import gaussian_filter

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
out_dir = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
cells = json.load(open(os.path.join(ref, "nocs", "zero_shot.ipynb")))["cells"]
src9 = "".join(cells[9]["source"])
assert src9.count("while True:") == 1
src9 = src9.replace("while True:", "for _capped in range(64):")
lines11 = "".join(cells[11]["source"]).split("\n")
first = next(i for i, l in enumerate(lines11) if l.strip().startswith("pc_idxs = "))
last = next(i for i, l in enumerate(lines11) if l.strip().startswith("mask[pc_idxs]"))
src_seg = "\n".join(l.strip() for l in lines11[first:last + 1])


def blobs(rng, shape, centres, amp=(1500.0, 4000.0), noise=3.0):
    g = (rng.random(shape) * noise).astype(np.float32)
    for c in centres:
        a = rng.uniform(*amp)
        for d in np.ndindex(2, 2, 2):
            p = tuple(min(max(int(c[k]) + d[k] - 1, 0), shape[k] - 1) for k in range(3))
            g[p] += np.float32(a / 8)
    return g


rng = np.random.default_rng(909)
cases = {
    "blobs": blobs(rng, (20, 16, 12), [(4, 4, 3), (14, 10, 8), (9, 13, 2)]),
    "last_plane": blobs(rng, (18, 14, 12), [(17, 6, 5), (5, 9, 4)]),
    "below": (rng.random((16, 12, 10)) * 20).astype(np.float32),
    "thin1": blobs(rng, (1, 12, 10), [(0, 5, 5)]),
    "thin2": blobs(rng, (14, 2, 10), [(6, 1, 4), (2, 0, 8)]),
    "many": blobs(rng, (24, 18, 14), [(3, 3, 3), (20, 4, 10), (12, 15, 6), (5, 14, 11), (18, 12, 1)], amp=(900.0, 5000.0)),
}
out = {}
corner = np.array([-0.31, 0.12, 0.55], np.float32)
res = 4e-3
for name, g in cases.items():
    ns = dict(np=np, gaussian_filter=gaussian_filter, grid_obj=g.copy(), corners=np.stack([corner, corner + 1]), res=res)
    out[f"{name}.grid"] = g
    out[f"{name}.smoothed_sha256"] = np.frombuffer(hashlib.sha256(gaussian_filter(g, sigma=1).tobytes()).digest(), np.uint8)
    try:
        exec(compile(src9, "zero_shot.ipynb:cell9", "exec"), ns)
    except TypeError:
        out[f"{name}.raises"] = np.array(1)
        continue
    out[f"{name}.raises"] = np.array(0)
    P = ns["proposals"]
    out[f"{name}.loc"] = np.array([p[0] for p in P], np.int64).reshape(-1, 3)
    out[f"{name}.value"] = np.array([p[1] for p in P], np.float32)
    out[f"{name}.diff"] = np.array([p[2] for p in P], np.float32)
    out[f"{name}.world"] = np.array([s[0] for s in ns["scene_locs"]], np.float64).reshape(-1, 3)
out["cases"] = np.array(list(cases))
out["corner"], out["res"] = corner, np.float64(res)

for s in range(4):
    r = np.random.default_rng(50 + s)
    N, P = 200, 3000
    idx = r.integers(0, N, (P, 2))
    surv = r.random(P) < (0.3 + 0.2 * s)
    idx[:40, 1] = idx[:40, 0]                                           # a few (i, i) pairs: both endpoints count
    ns = dict(np=np, point_idxs_masked=idx[surv], pc=np.zeros((N, 3), np.float32))
    exec(compile(src_seg, "zero_shot.ipynb:cell11", "exec"), ns)
    out[f"seg{s}.idx"], out[f"seg{s}.surv"] = idx.astype(np.int32), surv
    out[f"seg{s}.point_mask"], out[f"seg{s}.pairs"] = ns["mask"], ns["point_idxs_masked"].astype(np.int32)

np.savez_compressed(os.path.join(out_dir, "zero_shot.npz"), **out)
print({k: v.shape for k, v in out.items() if k.endswith(".loc") or k.endswith(".pairs")})
