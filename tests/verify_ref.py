"""What csrc/verify.hip and scene_stage.verify_proposals are held to: a plain numpy restatement of the two kernels and of the ratios
(the reference has no such stage, so the definitions are this project's and this file pins them).  Integer counts by
boolean algebra, the box test in float64."""
import numpy as np

COUNTS = ("within", "agree", "cross", "cross_agree", "mask_pts", "mask_in_box", "box_pts")


def proposal_support(idx, surv_bits, masks):
    """idx int[P,2], surv_bits u32[P], masks [K,N] (non-zero = member) -> i64[K,4] = within, agree, cross, cross_agree per proposal.
    An endpoint outside [0, N) is a non-member; a pair (i, i) is one pair; bits >= K are never looked at."""
    idx = np.asarray(idx, np.int64).reshape(-1, 2)
    bits = np.asarray(surv_bits).astype(np.int64).reshape(-1) & 0xffffffff
    masks = np.asarray(masks) != 0
    K, N = masks.shape
    out = np.zeros((K, 4), np.int64)
    ok = (idx >= 0) & (idx < N)
    safe = np.where(ok, idx, 0)
    for k in range(K):
        a = ok[:, 0] & masks[k][safe[:, 0]]
        b = ok[:, 1] & masks[k][safe[:, 1]]
        s = ((bits >> k) & 1).astype(bool)
        within, cross = a & b, a ^ b
        out[k] = within.sum(), (within & s).sum(), cross.sum(), (cross & s).sum()
    return out


def box_coords(points, center, axes):
    """float64 coordinates of the points along the box axes: (p - c) . A[:, a], A = axes as the row-major 3x3 (columns = axes)"""
    d = np.asarray(points, np.float64) - np.asarray(center, np.float64)
    return d @ np.asarray(axes, np.float64).reshape(3, 3)


def box_support(points, masks, centers, axes, half):
    """points [N,3], masks [K,N], centers [K,3], axes [K,9], half [K,3] -> i64[K,3] = mask_pts, mask_in_box, box_pts.  Inside:
    |coordinate a| <= half[a] for a = 0, 1, 2 in float64; a point with a non-finite coordinate is inside no box, and a comparison
    with a NaN is false."""
    points = np.asarray(points, np.float64)
    masks = np.asarray(masks) != 0
    K = masks.shape[0]
    finite = np.isfinite(points).all(axis=1)
    out = np.zeros((K, 3), np.int64)
    for k in range(K):
        with np.errstate(invalid="ignore"):
            t = box_coords(np.where(finite[:, None], points, 0.0), centers[k], axes[k])
            inside = finite & (np.abs(t) <= np.asarray(half[k], np.float64)).all(axis=1)
        out[k] = masks[k].sum(), (masks[k] & inside).sum(), inside.sum()
    return out


def face_margin(points, centers, axes, half):
    """the smallest distance of any finite point to any face of any box, relative to that half extent (float64):
    min | |t_a| - half_a | / half_a -- the band the exact-equality tests assert to be empty"""
    points = np.asarray(points, np.float64)
    points = points[np.isfinite(points).all(axis=1)]
    best = np.inf
    for c, A, h in zip(centers, axes, half):
        h = np.asarray(h, np.float64)
        if points.shape[0] and (h > 0).all():
            best = min(best, float((np.abs(np.abs(box_coords(points, c, A)) - h) / h).min()))
    return best


def ratios(counts):
    """seven counts in COUNTS' order -> the dict of verify_proposals: the counts as ints, agreement = agree / within, leak =
    cross_agree / cross, fill = mask_in_box / mask_pts, purity = mask_in_box / box_pts; 0.0 where the denominator is 0"""
    d = {k: int(v) for k, v in zip(COUNTS, counts)}
    div = lambda a, b: float(a) / float(b) if b else 0.0
    d["agreement"] = div(d["agree"], d["within"])
    d["leak"] = div(d["cross_agree"], d["cross"])
    d["fill"] = div(d["mask_in_box"], d["mask_pts"])
    d["purity"] = div(d["mask_in_box"], d["box_pts"])
    return d


def boxes_of(poses, res, pad=None):
    """f32[K,15] {T | R row-major | scale / 2 + pad} (scale_3d on the zero-shot path; pad = res by default), fp64 rounded once; a pose
    that is not finite gets half extents of -1 (no point inside)"""
    pad = float(res) if pad is None else float(pad)
    out = np.zeros((len(poses), 15), np.float32)
    for k, p in enumerate(poses):
        ext = np.asarray(p["scale_3d"] if "scale_3d" in p else p["scale"], np.float64).reshape(3)
        row = np.concatenate([np.asarray(p["T"], np.float64).reshape(3), np.asarray(p["R"], np.float64).reshape(9), ext / 2 + pad])
        if np.isfinite(row).all():
            out[k] = row
        else:
            out[k, 12:] = -1
    return out


def verify(pc, idx, bits_groups, masks, poses, res, pad=None, group=32):
    """verify_proposals restated: bits_groups = one u32[P] per group of `group` proposals"""
    masks = np.asarray(masks)
    K = len(poses)
    boxes = boxes_of(poses, res, pad)
    out = []
    for i, g in enumerate(range(0, K, group)):
        e = min(g + group, K)
        sup = proposal_support(idx, bits_groups[i], masks[g:e])
        box = box_support(pc, masks[g:e], boxes[g:e, 0:3], boxes[g:e, 3:12], boxes[g:e, 12:15])
        out += [ratios(np.concatenate([sup[j], box[j]])) for j in range(e - g)]
    return out
