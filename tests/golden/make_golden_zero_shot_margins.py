#!/usr/bin/env python3
"""tests/golden/zero_shot_margins.npz from the reference's own nocs/zero_shot.ipynb (run in the build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_zero_shot_margins.py /root/reference

The proposal cell (cell 9) is read from the notebook at generation time and exec'd with the real numpy / scipy, as
make_golden_zero_shot.py does, with its one `margin = 10` line set to the margins the device documents as its limits (64, 1) and
its `while True:` bounded; this script holds none of the cell's text.  The grids are those of tests/limits_cases.py (made from
seeds, not stored): the 140 x 137 x 131 grid with peaks in two corners, on a face and inside, and a thin 33 x 7 x 70 one.  Only the
proposals (with the notebook's repeats as they came) are written."""
import json
import os
import sys

import numpy as np
from scipy.ndimage import gaussian_filter

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(here)), os.path.dirname(here)]
sys.dont_write_bytecode = True
import limits_cases as LC  # noqa: E402

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
cells = json.load(open(os.path.join(ref, "nocs", "zero_shot.ipynb")))["cells"]
src9 = "".join(cells[9]["source"])
assert src9.count("while True:") == 1 and src9.count("margin = 10\n") == 1 and src9.count("thresh = 50\n") == 1
src9 = src9.replace("while True:", "for _capped in range(64):")

out = {}
for name, g, thresh in (("peaks", LC.margin_grid(), 50), ("thin", LC.smooth_grid_case((33, 7, 70)), 1)):
    for margin in (64, 1):
        src = src9.replace("margin = 10\n", f"margin = {margin}\n").replace("thresh = 50\n", f"thresh = {thresh}\n")
        ns = dict(np=np, gaussian_filter=gaussian_filter, grid_obj=g.copy(), corners=np.zeros((2, 3), np.float32), res=4e-3)
        exec(compile(src, "zero_shot.ipynb:cell9", "exec"), ns)
        P = ns["proposals"]
        out[f"{name}.m{margin}.loc"] = np.array([p[0] for p in P], np.int64).reshape(-1, 3)
        out[f"{name}.m{margin}.value"] = np.array([p[1] for p in P], np.float32)
        out[f"{name}.m{margin}.diff"] = np.array([p[2] for p in P], np.float32)
        out[f"{name}.m{margin}.thresh"] = np.float32(thresh)
np.savez_compressed(os.path.join(here, "zero_shot_margins.npz"), **out)
print({k: v.shape for k, v in out.items() if k.endswith(".loc")})
