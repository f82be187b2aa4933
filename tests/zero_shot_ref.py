"""numpy restatement of the zero-shot scene path of nocs/zero_shot.ipynb: the pair filter (cell 6), the proposals (cell 9, bit for
bit: scipy's separable Gaussian and numpy's float32 mean, in their own order) and the unsupervised instance segmentation of cell 11.
The pose of a proposal is composed in `pose_ref` from the oracle's rot_voting / sphere_count / axis_sign plus the mean of exp.
The defined behaviour where the notebook has none is that of include/cppf.h `cppf_scene_proposals`."""
import numpy as np

_f = np.float32


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius), radius = int(truncate * sigma + 0.5): fp64 [2r+1]"""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum()


def reflect_index(i, n):
    """scipy's mode='reflect' (= np.pad 'symmetric'): ... c b a | a b c | c b a ..."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def smooth(grid, sigma=1.0, truncate=4.0):
    """scipy.ndimage.gaussian_filter(grid, sigma, mode='reflect', truncate=truncate) for float32 grids, bit for bit: one pass
    per axis in order 0, 1, 2, each output in fp64 as w[r] x[c] + sum over d = r .. 1 of (x[c-d] + x[c+d]) w[r-d] (scipy's
    symmetric correlate1d), rounded to float32 after every pass"""
    w = gaussian_weights(sigma, truncate)
    r = (w.shape[0] - 1) // 2
    out = np.ascontiguousarray(grid, dtype=_f)
    for ax in range(out.ndim):
        n = out.shape[ax]
        x = out.astype(np.float64)
        c = np.arange(n)
        take = lambda k: np.take(x, reflect_index(c + k, n), axis=ax)
        acc = x * w[r]
        for d in range(r, 0, -1):
            acc = acc + (take(-d) + take(d)) * w[r - d]
        out = acc.astype(_f)
    return out


def np_mean_f32(v):
    """np.mean of a float32 vector of at most 128 elements, in numpy's order (pairwise_sum's base case), as a float32"""
    v = np.asarray(v, _f)
    n = v.shape[0]
    assert 0 < n <= 128
    if n < 8:
        s = _f(0)
        for a in v:
            s = _f(s + a)
    else:
        r = [v[j] for j in range(8)]
        for i in range(8, n - n % 8, 8):
            for j in range(8):
                r[j] = _f(r[j] + v[i + j])
        s = _f(_f(_f(r[0] + r[1]) + _f(r[2] + r[3])) + _f(_f(r[4] + r[5]) + _f(r[6] + r[7])))
        for i in range(n - n % 8, n):
            s = _f(s + v[i])
    return _f(s / _f(n))


def edge_mean(g, lll, rrr):
    """the mean of cell 9's twelve box-edge means (slices half-open lll:rrr), float32 sums left to right"""
    a0, a1, a2 = lll
    b0, b1, b2 = rrr
    parts = [g[a0:b0, a1, a2], g[a0:b0, a1, b2], g[a0:b0, b1, a2], g[a0:b0, b1, b2],
             g[a0, a1:b1, a2], g[a0, a1:b1, b2], g[b0, a1:b1, a2], g[b0, a1:b1, b2],
             g[a0, a1, a2:b2], g[a0, b1, a2:b2], g[b0, a1, a2:b2], g[b0, b1, a2:b2]]
    s = _f(0)
    for k, p in enumerate(parts):
        m = np_mean_f32(p)
        s = m if k == 0 else _f(s + m)
    return _f(s / _f(12))


def proposals(smoothed, thresh=50, margin=10, max_proposals=32, max_iters=None):
    """cell 9's loop on an already smoothed grid (not modified) -> (loc i32[K,3], value f32[K], diff f32[K], iterations).
    Defined where the notebook is not: an axis < 2 gives nothing; the 0.7 max_val clause is false while max_val is unset;
    an iteration that repeats the previous one's (loc, diff) ends the loop; at most max_proposals / max_iters."""
    g = np.array(smoothed, dtype=_f, copy=True)
    max_iters = 4 * max_proposals if max_iters is None else max_iters
    locs, vals, diffs = [], [], []
    if g.ndim != 3 or min(g.shape) < 2:
        return np.zeros((0, 3), np.int32), np.zeros(0, _f), np.zeros(0, _f), 0
    dims = np.array(g.shape)
    th, max_val, prev, it = _f(thresh), None, None, 0
    while it < max_iters and len(locs) < max_proposals:
        it += 1
        loc = np.array(np.unravel_index(int(np.argmax(g)), g.shape))
        lll = np.maximum(0, loc - margin)
        rrr = np.minimum(dims - 1, loc + margin)
        val = g[loc[0], loc[1], loc[2]]
        diff = _f(val - edge_mean(g, lll, rrr))
        key = (tuple(loc), diff.tobytes())
        if key == prev:
            break
        prev = key
        if diff > th:
            if max_val is None:
                max_val = diff
            locs.append(loc)
            vals.append(val)
            diffs.append(diff)
        if diff < th or (max_val is not None and diff < _f(max_val * _f(0.7))):
            break
        g[lll[0]:rrr[0], lll[1]:rrr[1], lll[2]:rrr[2]] = 0
    return (np.array(locs, np.int32).reshape(-1, 3), np.array(vals, _f), np.array(diffs, _f), it)


def world(loc, corner, res):
    """scene_locs' coordinates: corners[0] + loc * res in fp64 from the float32 corner"""
    return np.asarray(corner, _f).astype(np.float64) + np.asarray(loc, np.int64) * float(res)


def distinct_mask(pc, nrm, idx):
    """cell 6: True for the pairs kept (not 'indistinguishable'), float32 throughout.  Defined where the notebook is not
    (include/cppf.h cppf_pair_filter_distinct): a pair with an endpoint outside [0, n_points) is dropped."""
    pc, nrm = np.asarray(pc, _f), np.asarray(nrm, _f)
    idx = np.asarray(idx, np.int64)
    ok = ((idx >= 0) & (idx < pc.shape[0])).all(1)
    idx = np.where(ok[:, None], idx, 0)
    n1, n2 = nrm[idx[:, 0]], nrm[idx[:, 1]]
    ab = pc[idx[:, 0]] - pc[idx[:, 1]]
    ab /= (np.linalg.norm(ab, axis=-1, keepdims=True) + 1e-7)
    ppf = np.stack([np.sum(n1 * n2, -1), np.sum(ab * n1, -1), np.sum(ab * n2, -1)], -1)
    mask = (np.abs(ppf[:, 0]) > 0.9) & (np.abs(ppf[:, 1]) < 0.1) & (np.abs(ppf[:, 2]) < 0.1)
    return ~mask & ok


def segment(idx, surv_mask, n_points, min_contrib=12):
    """cell 11's unsupervised segmentation: (point mask bool[N], positions i64[M] of the kept pairs in the full list).  Defined
    where the notebook is not (include/cppf.h cppf_segment_instance): an endpoint outside [0, n_points) is not counted and is in
    no instance; the pair's other endpoint counts as usual."""
    idx = np.asarray(idx, np.int64)
    pos = np.nonzero(surv_mask)[0]
    ends = idx[pos]
    ok = (ends >= 0) & (ends < n_points)
    cnt = np.bincount(ends[ok], minlength=n_points)
    pm = cnt > min_contrib
    keep = (ok & pm[np.where(ok, ends, 0)]).any(1)
    return pm, pos[keep]


def pose_ref(O, pc, nrm, idx, preds, sel, T, sphere_pts, scale_mean, angle_tol=2.0, max_rot_pairs=10000, n_rots=72):
    """the rest of cell 11 for one proposal, composed from the oracle: rot_voting on column 2 of the first max_rot_pairs kept
    pairs, sphere count, arg-max, axis sign on column 4, right = (0, -up_z, up_y), scale_3d = mean(exp(cols 6..8)) scale_mean 2"""
    pi = np.asarray(idx, np.int32)[sel]
    pr = np.asarray(preds, _f)[sel]
    sub = slice(0, max_rot_pairs)
    cands = O.rot_voting(pc, np.ascontiguousarray(pr[sub, 2]), np.ascontiguousarray(pi[sub]), n_rots)
    counts = O.sphere_count(cands, sphere_pts, angle_tol)
    best = np.array(sphere_pts[int(np.argmax(counts))], np.float64)
    flip, _ = O.axis_sign(pc, nrm, pi, np.ascontiguousarray(pr[:, 4]), best)
    up = -best if flip else best
    right = np.array([0, -up[2], up[1]])
    right = right / np.linalg.norm(right)
    R = np.stack([right, up, np.cross(right, up)], -1)
    scale_3d = np.mean(np.exp(pr[:, 6:9]).astype(np.float64), 0) * np.asarray(scale_mean, np.float64) * 2
    return dict(up=up, R=R, scale_3d=scale_3d, scale=float(np.linalg.norm(scale_3d)), T=np.asarray(T, np.float64))
