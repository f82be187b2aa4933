#!/usr/bin/env python3
"""Regenerates tests/golden/ref_vote.npz: what the reference's OWN vote kernels compute -- the executed text of
models/voting.py (ppf_voting, backvote, rot_voting), built as host C++ by oracle/ref_build.py into oracle/_ref/ -- on a
prefix of every case of tests/ref_vote_cases.py, with the inputs.  It pins oracle/cppf_oracle.c / voting_variants.c in a
checkout that has no reference at all (tests/test_ref_vote_cpu.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vote.py /root/reference

Per case `<name>`: the kernels' inputs (points, outputs, idx, rot, corner, dims, gt and meta = res, tol, n_rots, adaptive),
`grid_cells` / `grid_vals` (flat indices and fp32 values of the non-zero cells of ppf_voting's serial fp32 grid), `offsets`
(backvote) and `up` (rot_voting, first FIXTURE_ROT_PAIRS pairs); the two `-tol-` cases are the first case with another tol and
hold `meta`, `offsets` and `probe` (the survivor tol was put next to) only.  The archive is written with fixed time stamps:
running the script again gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import oracle as O          # noqa: E402
from oracle import ref_build            # noqa: E402
import ref_vote_cases as RC             # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    if ref_build.build(ref) is None:
        sys.exit("reference not found")
    O.build()
    arrays = {}
    names = []
    for c in RC.all_cases(O):
        n = min(RC.FIXTURE_PAIRS, c["idx"].shape[0])
        p = RC.prefix(c, n)
        names.append(c["name"])
        k = c["name"] + "."
        arrays[k + "meta"] = np.asarray([p["res"], p["tol"], p["n_rots"], int(p["adaptive"])], np.float64)
        arrays[k + "offsets"] = RC.host_run(p, "backvote")
        if "-tol-" in c["name"]:        # the first case's inputs with another tol: only the back-vote differs
            assert c["probe"] < n
            arrays[k + "probe"] = np.asarray(c["probe"], np.int32)
            continue
        for f in ("points", "outputs", "idx", "rot", "corner", "dims", "gt"):
            arrays[k + f] = np.ascontiguousarray(p[f])
        g = RC.host_run(p, "ppf_voting").reshape(-1)
        nz = np.nonzero(g)[0]
        arrays[k + "grid_cells"], arrays[k + "grid_vals"] = nz.astype(np.int32), g[nz]
        arrays[k + "up"] = RC.host_run(RC.prefix(c, min(RC.FIXTURE_ROT_PAIRS, n)), "rot_voting")
    arrays["names"] = np.asarray(names)
    out = os.path.join(HERE, "ref_vote.npz")
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[key], allow_pickle=False)
            zi = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
