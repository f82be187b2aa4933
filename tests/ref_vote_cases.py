"""Inputs on which the reference's own vote-kernel text (oracle/_ref/, built by oracle/ref_build.py) is executed and compared
with the oracle (tests/test_ref_vote_cpu.py), stored as a fixture (tests/golden/make_golden_vote.py) and compared with the HIP
kernels on the device (tests/test_gpu_ref_vote.py).  Not a test module.

A case is a dict of the kernels' arguments: points f32[N',3], outputs f32[P,2], probs f32[N'], idx i32[P,2], corner f32[3],
dims i32[3], res, n_rots, adaptive, gt f32[3], tol, rot f32[P], plus name and mode.  N = 512 points and K = 16 pairs per point
(FS.CASES_SMALL-sized inputs), four extra points appended for the edge pairs, and P cut to a count that is no multiple of 32.
The edge pairs sit in the first slots so that a prefix of a case (the fixture: FIXTURE_PAIRS) holds all of them:

  slot 0, 1    a -> a + (0.05, 0, 0) and back: ab along +-x, the `co` fallback of voting.py:27 / :92 / :135
  slot 2       |a - b| = 6e-8 < 1e-7: the early return of :21 / :87 / :131
  slot 3       |a - b| ~ 2.4e-7, just alive
  slot 4..7    a == b
  slot 8..11   odist = 1e-5 -> 0 adaptive rotations;  slot 12..15  odist = res / 4 -> 1 adaptive rotation
  rot[0..5]    0, pi/2 - 1 ulp, -(pi/2 - 1 ulp), -0.7, float(pi/2) (tan < 0), -float(pi/2): the sign branch of :142
and, as in tests/test_oracle_variants.py, idx[::97] degenerate and outputs[::53, 1] = 1e-5 through the rest of the list.
"""
import ctypes as C
import os

import numpy as np

import fmad_sensitivity as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
F = np.float32
FIXTURE_PAIRS, FIXTURE_ROT_PAIRS = 104, 64

#        name              cat       seed mode      n_rots adaptive  P
SPECS = [("bottle-ka-72",  "bottle", 0, "ka",      72,  True,  4001),
         ("bottle-uni-120", "bottle", 0, "uniform", 120, False, 3003),
         ("camera-ka-1",   "camera", 1, "ka",      1,   True,  4001),
         ("mug-uni-72",    "mug",    3, "uniform", 72,  True,  2999)]


def make_case(O, name, cat, seed, mode, n_rots, adaptive, P):
    ob, idx, outputs, heads, ocfg = FS.make_case(cat, 512, 16, seed, mode)
    res = float(ocfg["res"])
    pc = ob["pc"].astype(F)
    j = int(np.argmin(np.abs(pc[:, 0])))              # the point whose x has the finest fp32 spacing
    extra = np.repeat(pc[j][None], 4, 0)
    extra[0, 0] += F(0.05)
    extra[1, 0] += F(6e-8)
    extra[2] += F(1.4e-7)
    extra[3, 0] -= F(0.05)
    assert 0 < float(extra[1, 0]) - float(pc[j, 0]) < 1e-7
    points = np.concatenate([pc, extra]).astype(F)
    N = pc.shape[0]
    idx = idx[:P].astype(np.int32).copy()
    outputs = outputs[:P].astype(F).copy()
    rot = heads[:P, 0].astype(F).copy()
    idx[::97, 1] = idx[::97, 0]
    outputs[::53, 1] = 1e-5
    idx[0], idx[1], idx[2], idx[3] = (j, N), (N + 3, j), (j, N + 1), (j, N + 2)
    idx[4:8, 1] = idx[4:8, 0]
    outputs[8:12, 1] = 1e-5
    outputs[12:16, 1] = F(res / 4)
    h = np.nextafter(F(np.pi / 2), F(0))
    rot[:6] = [0.0, h, -h, -0.7, F(np.pi / 2), -F(np.pi / 2)]
    probs = np.ones(points.shape[0], F)
    corner, dims = O.grid_setup(points, res)
    g64, _ = O.ppf_voting_f64(points, outputs, probs, idx, dims, corner, res, n_rots, adaptive)
    gt = O.center_from_argmax(int(np.argmax(g64)), dims, corner, res).astype(F)
    return dict(name=name, mode=mode, points=points, outputs=outputs, probs=probs, idx=idx, corner=corner.astype(F),
                dims=np.asarray(dims, np.int32), res=res, n_rots=n_rots, adaptive=adaptive, gt=gt, tol=float(F(3 * res)), rot=rot)


def _centres_one_rotation(c):
    """fp64 centre of every pair's first sample (angle 0), and the unit ab"""
    p = c["points"].astype(np.float64)
    a, b = p[c["idx"][:, 0]], p[c["idx"][:, 1]]
    ab = a - b
    ln = np.linalg.norm(ab, axis=-1, keepdims=True)
    ab = ab / (ln + 1e-7)
    co = np.stack([np.zeros(len(ab)), -ab[:, 2], ab[:, 1]], -1)
    x = co / (np.linalg.norm(co, axis=-1, keepdims=True) + 1e-7)
    return a, ab, x, ln[:, 0]


def shell_case(base, per_face=6):
    """Pairs with ONE adaptive rotation (odist = res / 4) whose centre lies 0.005 cells inside a low face of the grid or 0.005
    cells below a high face (coordinate dim - 1.005), per_face pairs on each of the six faces in the order x low, x high, y low,
    y high, z low, z high, the other two coordinates well inside: ppf_voting's [0.01, dim - 1.01) test rejects all of them on that
    one comparison, backvote's [0, dim - 1) accepts all of them (tol is 10: every distance passes).  Margins: 0.005 cells against
    an fp32 error of ~1e-5 cells."""
    c = dict(base)
    res, dims, corner = c["res"], c["dims"], c["corner"].astype(np.float64)
    a, ab, x, ln = _centres_one_rotation(c)
    od = float(F(res / 4))
    rows, mus = [], []
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        for face in (0, 1):
            t = corner[ax] + (0.005 if face == 0 else dims[ax] - 1.005) * res
            with np.errstate(divide="ignore", invalid="ignore"):
                mu = (a[:, ax] + x[:, ax] * od - t) / ab[:, ax]
                g = (a - ab * mu[:, None] + x * od - corner) / res
            ok = (ln > 1e-3) & (np.abs(ab[:, ax]) > 0.3) & np.isfinite(mu) & (np.abs(mu) < 1.0)
            ok &= (g[:, o1] > 1) & (g[:, o1] < dims[o1] - 2) & (g[:, o2] > 1) & (g[:, o2] < dims[o2] - 2)
            r = np.nonzero(ok)[0][:per_face]
            assert r.size == per_face, "not enough pairs reach the grid face"
            assert np.all(np.abs(g[r, ax] - (0.005 if face == 0 else dims[ax] - 1.005)) < 1e-6)
            rows.append(r)
            mus.append(mu[r])
    r, mu = np.concatenate(rows), np.concatenate(mus)
    c.update(name=base["name"] + "-shell", idx=c["idx"][r].copy(), rot=c["rot"][r].copy(), tol=10.0,
             outputs=np.stack([mu, np.full(mu.shape, od)], -1).astype(F), adaptive=True, n_rots=72)
    return c


def tol_cases(O, base):
    """backvote with tol 1e-4 below / above the distance of one survivor's accepted centre from gt: on the low side that
    sample is rejected (voting.py:102), on the high side it is the accepted one."""
    oo, m = O.backvote(base["points"], base["outputs"], base["idx"], base["corner"], base["res"], base["n_rots"], base["dims"],
                       base["gt"], F(base["tol"]))
    a, ab, _, _ = _centres_one_rotation(base)
    ctr = a - ab * base["outputs"][:, :1].astype(np.float64) - oo.astype(np.float64)
    d = np.linalg.norm(ctr - base["gt"].astype(np.float64), axis=-1)
    surv = np.nonzero(m & (d > 0.3 * base["tol"]))[0]
    surv = surv[surv < FIXTURE_PAIRS]                            # (inside the prefix the fixture keeps)
    assert surv.size, "no survivor to put tol next to"
    k = int(surv[0])
    out = []
    for tag, s in (("below", 1 - 1e-4), ("above", 1 + 1e-4)):
        c = dict(base)
        c.update(name=f"{base['name']}-tol-{tag}", tol=float(F(d[k] * s)), probe=k)
        out.append(c)
    return out


def all_cases(O):
    cases = [make_case(O, *s) for s in SPECS]
    return cases + [shell_case(cases[0])] + tol_cases(O, cases[0])


def prefix(c, n):
    """the first n pairs of a case (grid, corner and gt unchanged)"""
    d = dict(c)
    for k in ("idx", "outputs", "rot"):
        d[k] = c[k][:n].copy()
    return d


# ------------------------------------------------------------------ the host build of the reference's text
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        so = os.path.join(REF_DIR, "libref_vote_host.so")
        _HOST = C.CDLL(so) if os.path.isfile(so) else False
    return _HOST or None


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _head(c):
    return [np.ascontiguousarray(c[k], F) for k in ("points", "outputs", "probs")] + [np.ascontiguousarray(c["idx"], np.int32)]


def host_run(c, kernel):
    """the reference's kernel text, host build, on case c -> its (zero-initialised) output array"""
    L = host_lib()
    pts, out, probs, idx = _head(c)
    corner, gt, rot = (np.ascontiguousarray(c[k], F) for k in ("corner", "gt", "rot"))
    P, (gx, gy, gz) = idx.shape[0], (int(d) for d in c["dims"])
    tail = [C.c_float(c["res"]), C.c_int(P), C.c_int(c["n_rots"]), C.c_int(gx), C.c_int(gy), C.c_int(gz)]
    if kernel == "ppf_voting":
        r = np.empty((gx, gy, gz), F)
        L.ref_host_ppf_voting(_p(pts), _p(out), _p(probs), _p(idx), _p(r), _p(corner), *tail, C.c_int(int(c["adaptive"])))
    elif kernel == "backvote":
        r = np.empty((P, 3), F)
        L.ref_host_backvote(_p(pts), _p(out), _p(r), _p(idx), _p(corner), *tail, _p(gt), C.c_float(c["tol"]))
    else:
        r = np.empty((P, c["n_rots"], 3), F)
        L.ref_host_rot_voting(_p(pts), _p(rot), _p(r), _p(idx), _p(corner), *tail)
    return r


# ------------------------------------------------------------------ the device build, through oracle/_ref/ref_vote_runner
def write_job(c, path):
    """the runner's input file (layout: oracle/ref_runner.c)"""
    pts, out, probs, idx = _head(c)
    gx, gy, gz = (int(d) for d in c["dims"])
    with open(path, "wb") as f:
        np.asarray([pts.shape[0], idx.shape[0], c["n_rots"], gx, gy, gz, int(c["adaptive"]), 0], np.int32).tofile(f)
        np.asarray([c["res"], c["tol"]], F).tofile(f)
        for a in (pts, out, probs, idx, np.ascontiguousarray(c["corner"], F), np.ascontiguousarray(c["gt"], F),
                  np.ascontiguousarray(c["rot"], F)):
            a.tofile(f)


def out_shape(c, kernel):
    P = c["idx"].shape[0]
    return {"ppf_voting": tuple(int(d) for d in c["dims"]), "backvote": (P, 3), "rot_voting": (P, c["n_rots"], 3)}[kernel]
