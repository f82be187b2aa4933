"""Inputs and float64 restatements for the pose tail's reductions, its bin arg-max and the record assembled on the device
(tests/test_gpu_pose_tail_edges.py).  Not a test module.

The cloud has 512 points; the first N_EXACT have coordinates k / 8 with small integers k and axis normals, so that the three
comparisons with zero of nocs/inference.py:287-298 can be hit exactly:
  a == b              den = 1e-7, ab_normed = 0, d = 0: no flip
  n orthogonal to a-b d == 0 exactly: no flip
  n orthogonal to best_dir = (0, 1, 0)   proj == 0 exactly: target 0
The pair list is PAIRS long, drawn once; rows k = 0 mod 97 are those exact pairs in turn.  heads f32[PAIRS, 8] holds what the tail
reads: aux logits in columns 2, 3 (LOGITS in turn; column 3 one step ahead), integer scale logits in columns 4..6.
"""
import functools
import math

import numpy as np

F, D = np.float32, np.float64
N_POINTS, N_EXACT, PAIRS = 512, 16, 131_073
SIZES = (0, 1, 255, 256, 257, 65_535, 65_536, 65_537, 131_073)
LOGITS = (-1e4, 1e4, -88.0, 88.0, -30.0, 30.0, -1.0, 1.0, -1e-30, 1e-30, -0.0, 0.0)      # row 0: -1e4 / +1e4, exact terms
# (a, b) among the exact points, by what they hit
EXACT_PAIRS = ((0, 0), (3, 3), (0, 1), (1, 0), (2, 4), (5, 6), (6, 5), (7, 8), (9, 10))


@functools.lru_cache(maxsize=None)
def cloud():
    rng = np.random.default_rng(7)
    pc = rng.normal(0.0, 0.1, (N_POINTS, 3)).astype(F)
    nrm = rng.normal(size=(N_POINTS, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    k = np.array([(0, 0, 0), (2, 0, 0), (0, 3, 0), (1, 1, 1), (0, 3, 5), (-1, 2, 0), (-1, 2, 4), (4, -4, 1), (4, 2, 1), (0, 0, 7), (3, 0, 7),
                  (1, -2, 3), (5, 5, 5), (-3, 1, 2), (2, 2, -6), (7, 0, -1)], D) / 8
    n = np.array([(0, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 1, 0), (1, 0, 0), (0, 1, 0), (1, 0, 0), (0, 0, -1), (0, -1, 0), (0, 0, 1),
                  (1, 0, 0), (0, 0, 1), (-1, 0, 0), (0, 0, -1), (0, 1, 0)], D)
    pc[:N_EXACT], nrm[:N_EXACT] = k, n
    return pc, nrm


@functools.lru_cache(maxsize=None)
def pairs():
    """-> idx i32[PAIRS,2], heads f32[PAIRS,8]"""
    rng = np.random.default_rng(11)
    idx = rng.integers(0, N_POINTS, (PAIRS, 2)).astype(np.int32)
    rows = np.arange(0, PAIRS, 97)
    idx[rows] = np.asarray(EXACT_PAIRS, np.int32)[np.arange(rows.size) % len(EXACT_PAIRS)]
    heads = np.full((PAIRS, 8), 77.0, F)                                      # (columns the tail does not read: poison)
    heads[:, :2] = 0.0
    lg = np.asarray(LOGITS, F)
    heads[:, 2] = lg[np.arange(PAIRS) % len(LOGITS)]
    heads[:, 3] = lg[(np.arange(PAIRS) + 1) % len(LOGITS)]
    heads[:, 4:7] = rng.integers(-8, 9, (PAIRS, 3)).astype(F)
    return idx, heads


def flipped_normals(pc, nrm, idx):
    """nocs/inference.py:287-293 in the fp32 arithmetic numpy gives it: n of a, turned where n . ab_normed < 0"""
    ab = (pc[idx[:, 0]] - pc[idx[:, 1]]).astype(F)
    distsq = ((ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]).astype(F) + ab[:, 2] * ab[:, 2]).astype(F)
    den = (np.sqrt(distsq).astype(F) + F(1e-7)).astype(F)
    abn = (ab / den[:, None]).astype(F)
    n = nrm[idx[:, 0]].astype(F)
    d = ((n[:, 0] * abn[:, 0] + n[:, 1] * abn[:, 1]).astype(F) + n[:, 2] * abn[:, 2]).astype(F)
    return np.where((d < 0)[:, None], -n, n).astype(F), d


def bce_terms(pc, nrm, idx, aux, best_dir):
    """:294-301 per pair in float64 -> (up terms, down terms, target): BCE-with-logits of aux against the target n . best_dir > 0
    and against its complement, as max(x, 0) - x t + log1p(exp(-|x|))"""
    n, _ = flipped_normals(pc, nrm, idx)
    b = np.asarray(best_dir, D)
    proj = (n[:, 0].astype(D) * b[0] + n[:, 1].astype(D) * b[1]) + n[:, 2].astype(D) * b[2]
    t = (proj > 0).astype(D)
    x = aux.astype(D)
    sp = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    return sp - x * t, sp - x * (1.0 - t), t


def fsum_bound(terms):
    """(exact sum, the bound on what ANY summation order of these fp64 terms can be off by: n 2^-53 sum|term|)"""
    return math.fsum(terms), len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms))


# ------------------------------------------------------------------ the record (nocs/inference.py:299-339) in float64
FALLBACK_HEX = ("0x1.017ed89db8441p-3", "-0x1.0e8cfe9bd45ccp-3", "0x1.47e57a468b06dp-1")     # csrc/pose_tail.hip: assemble_record


def assemble(T, bdirs, sums, scale_sums, n_surv, n_dirs, regress_right, scale_mean, argmax, peak, object_id):
    """The 16-double record from the tail's sums: bdirs f64[2,3] the best bins, sums[j] = (up, down) loss sums of direction j,
    scale_sums the three sums of the scale logits.  -> (record, which branches ran)"""
    n = max(float(n_surv), 1.0)
    dirs, flips = np.zeros((2, 3)), []
    for j in range(n_dirs):
        flip = sums[j][1] / n < sums[j][0] / n
        flips.append(bool(flip))
        dirs[j] = -np.asarray(bdirs[j], D) if flip else np.asarray(bdirs[j], D)
    up = dirs[0]
    if regress_right and n_dirs > 1:
        r = dirs[1] - ((up[0] * dirs[1][0] + up[1] * dirs[1][1]) + up[2] * dirs[1][2]) * up
    else:
        r = np.array([0.0, -up[2], up[1]])
    r = r / (np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + 1e-9)
    fallback = bool(np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) < 1e-7)
    if fallback:
        r = np.random.default_rng(0).standard_normal(3)
        r = r - ((r[0] * up[0] + r[1] * up[1]) + r[2] * up[2]) * up
        r = r / np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    mean = (np.asarray(scale_sums, D) / n).astype(F)
    scale = np.exp(mean.astype(D)).astype(F).astype(D) * np.asarray(scale_mean, D) * 2.0
    rec = np.concatenate([np.asarray(T, D), up, r, scale, [float(argmax), float(peak), float(n_surv), float(object_id)]])
    if argmax < 0:
        rec[:12] = np.nan
    return rec, dict(flips=flips, fallback=fallback)
