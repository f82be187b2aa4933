"""Restatement of csrc/segments.hip (include/cppf.h "Depth segments") without a device, and the images its tests share.
- segments_ref: the link graph of a depth image in numpy, scipy.sparse.csgraph.connected_components for the components, then the
  definition's own words: the root is the smallest flat index, the kept components are ranked by root;
- flood_ref: the same components by a plain Python flood fill (what segments_ref itself is held to);
- planes_ref / counts_ref / best_ref: cppf_plane_ransac in numpy fp32 in the stated operation order (the Philox block is
  cppf_amd.synthetic's host Philox, as tests/scene_training_ref.py draws it, on stream 5);
- the patterns of the device tests (serpentine, comb, checkerboard, ...);
- perfect_segment_scene: tests/scene_poses_ref.py's perfect-head scene with every pair drawn inside one true object."""
import numpy as np

import scene_training_ref as ST_REF

PLANE_STREAM = 5
_s32 = np.uint64(32)


# ------------------------------------------------------------------------------------------------------------------- the segments
def live_ref(depth, valid=None):
    z = np.asarray(depth).astype(np.uint16).astype(np.int64)
    live = z > 0
    if valid is not None:
        live &= np.asarray(valid) != 0
    return z, live


def _linked(za, zb, la, lb, tol, slope):
    return la & lb & (np.abs(za - zb) <= tol + (slope * np.minimum(za, zb)) // 1000)


def links_ref(depth, valid, tol, slope):
    """(horizontal bool[H,W-1]: (y,x)~(y,x+1); vertical bool[H-1,W]: (y,x)~(y+1,x))"""
    z, live = live_ref(depth, valid)
    return (_linked(z[:, :-1], z[:, 1:], live[:, :-1], live[:, 1:], tol, slope),
            _linked(z[:-1, :], z[1:, :], live[:-1, :], live[1:, :], tol, slope))


def _finish(root, live, min_pixels, max_pixels, capacity):
    """root i64[H*W] (the component's smallest flat index, -1 dead) -> the outputs of cppf_depth_segments by its definition"""
    n = root.shape[0]
    size_at = np.bincount(root[live], minlength=n)
    comp_size = np.where(live, size_at[np.maximum(root, 0)], 0).astype(np.int32)
    roots = np.nonzero(size_at > 0)[0]                                        # ascending
    kept = roots[(size_at[roots] >= min_pixels) & ((max_pixels == 0) | (size_at[roots] <= max_pixels))]
    S = kept.shape[0]
    counts = np.array([S, roots.shape[0], int(live.sum()), 0], np.int32)
    overflow = S > capacity
    first, sizes = np.full(capacity, -1, np.int32), np.zeros(capacity, np.int32)
    labels = np.full(n, -1, np.int32)
    if not overflow:
        first[:S], sizes[:S] = kept, size_at[kept]
        rank = np.full(n, -1, np.int64)
        rank[kept] = np.arange(S)
        labels = np.where(live, rank[np.maximum(root, 0)], -1).astype(np.int32)
    return dict(comp_size=comp_size, counts=counts, overflow=overflow, first=first, sizes=sizes, labels=labels)


def segments_ref(depth, valid=None, tol_mm=10, slope_permille=10, min_pixels=200, max_pixels=0, capacity=256):
    """cppf_depth_segments: dict(labels i32[H,W], comp_size i32[H,W], first i32[capacity], sizes i32[capacity], counts i32[4],
    overflow).  On overflow labels / first / sizes are not part of the definition (they hold -1 / -1 / 0)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    depth = np.asarray(depth)
    H, W = depth.shape
    _, live = live_ref(depth, valid)
    hl, vl = links_ref(depth, valid, int(tol_mm), int(slope_permille))
    flat = np.arange(H * W).reshape(H, W)
    a = np.concatenate([flat[:, :-1][hl], flat[:-1, :][vl]])
    b = np.concatenate([flat[:, 1:][hl], flat[1:, :][vl]])
    g = coo_matrix((np.ones(a.shape[0], np.int8), (a, b)), shape=(H * W, H * W))
    _, comp = connected_components(g, directed=False)
    smallest = np.full(H * W, H * W, np.int64)
    np.minimum.at(smallest, comp, np.arange(H * W))
    root = np.where(live.reshape(-1), smallest[comp], -1)
    out = _finish(root, live.reshape(-1), int(min_pixels), int(max_pixels), int(capacity))
    out["labels"], out["comp_size"] = out["labels"].reshape(H, W), out["comp_size"].reshape(H, W)
    return out


def flood_ref(depth, valid=None, tol_mm=10, slope_permille=10, min_pixels=200, max_pixels=0, capacity=256):
    """segments_ref's dict by a plain Python flood fill over the pixels in ascending order: the pixel a fill starts at is its
    component's smallest index"""
    depth = np.asarray(depth)
    H, W = depth.shape
    z, live = live_ref(depth, valid)
    root = np.full((H, W), -1, np.int64)

    def linked(y0, x0, y1, x1):
        if not (live[y0, x0] and live[y1, x1]):
            return False
        za, zb = int(z[y0, x0]), int(z[y1, x1])
        return abs(za - zb) <= int(tol_mm) + (int(slope_permille) * min(za, zb)) // 1000

    for y in range(H):
        for x in range(W):
            if not live[y, x] or root[y, x] >= 0:
                continue
            r = y * W + x
            root[y, x] = r
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and root[ny, nx] < 0 and linked(cy, cx, ny, nx):
                        root[ny, nx] = r
                        stack.append((ny, nx))
    out = _finish(root.reshape(-1), live.reshape(-1), int(min_pixels), int(max_pixels), int(capacity))
    out["labels"], out["comp_size"] = out["labels"].reshape(H, W), out["comp_size"].reshape(H, W)
    return out


# ------------------------------------------------------------------------------------------------------------------- patterns
def serpentine(H, W, z=1000):
    """a one-pixel-wide path through the whole image: even rows 0, 2, 4, ... are live over their whole width, the odd rows between
    have one live pixel, alternately at the right and the left end.  Pixel 0 is one END of the path."""
    d = np.zeros((H, W), np.uint16)
    d[0::2, :] = z
    for k, y in enumerate(range(1, H, 2)):
        d[y, W - 1 if k % 2 == 0 else 0] = z
    return d


def comb(H, W, z=1000):
    """teeth in every second column that join only in the LAST row"""
    d = np.zeros((H, W), np.uint16)
    d[:, 0::2] = z
    d[H - 1, :] = z
    return d


def checkerboard(H, W, z=1000):
    d = np.zeros((H, W), np.uint16)
    yy, xx = np.mgrid[:H, :W]
    d[(yy + xx) % 2 == 0] = z
    return d


def levels_image(seed, H=67, W=131):
    """depths from 4 levels in blocks, plus noise of a few mm, 20 % dead"""
    rng = np.random.default_rng(seed)
    levels = np.array([600, 900, 1500, 2600])
    by, bx = rng.integers(3, 12), rng.integers(3, 12)
    blocks = rng.integers(0, 4, ((H + by - 1) // by, (W + bx - 1) // bx))
    base = np.kron(blocks, np.ones((by, bx), np.int64))[:H, :W]
    d = levels[base] + rng.integers(-6, 7, (H, W))
    d[rng.random((H, W)) < 0.2] = 0
    return d.astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------- the planes
def plane_indices_ref(n_points, n_hyp, seed):
    h = np.arange(int(n_hyp), dtype=np.uint64)
    w = ST_REF.syn.philox4x32_10([h, np.zeros_like(h), np.full_like(h, PLANE_STREAM), np.zeros_like(h)], seed)
    N = np.uint64(int(n_points))
    return [((w[k] * N) >> _s32).astype(np.int64) for k in range(3)]


def planes_ref(points, n_hyp, seed):
    """planes f32[n_hyp,4] in numpy fp32, every operation rounded once in the stated order"""
    f = np.float32
    pts = np.asarray(points, f)
    ia, ib, ic = plane_indices_ref(pts.shape[0], n_hyp, seed)
    a, b, c = pts[ia], pts[ib], pts[ic]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f)
        l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(f)
        ok = (l > f(1e-12)) & np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & np.isfinite(c).all(-1)
        n = (n / np.where(ok, l, f(1))[:, None]).astype(f)
        d = (-((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2])).astype(f)
        flip = d < 0
        n, d = np.where(flip[:, None], -n, n), np.where(flip, -d, d)
        pl = np.concatenate([n, d[:, None]], -1).astype(f)
        ok &= np.isfinite(pl).all(-1)
    pl[~ok] = 0
    return pl


def counts_ref(points, planes, thresh):
    """counts i32[n_hyp] of `planes` (the device's own, for an exact comparison) over the points, in fp32 in the stated order"""
    f = np.float32
    p, pl = np.asarray(points, f), np.asarray(planes, f)
    out = np.zeros(pl.shape[0], np.int32)
    with np.errstate(all="ignore"):
        for h in range(pl.shape[0]):
            if not pl[h, :3].any():
                continue
            s = ((pl[h, 0] * p[:, 0] + pl[h, 1] * p[:, 1]) + pl[h, 2] * p[:, 2]) + pl[h, 3]
            out[h] = int((np.abs(s) <= f(thresh)).sum())
    return out


def best_ref(planes, counts):
    """{the lowest h with the largest count among the non-degenerate hypotheses, that count}, or {-1, 0}"""
    ok = np.asarray(planes)[:, :3].any(-1)
    if not ok.any():
        return np.array([-1, 0], np.int32)
    c = np.where(ok, np.asarray(counts, np.int64), -1)
    h = int(np.argmax(c))                                                      # (the first of equal maxima)
    return np.array([h, c[h]], np.int32)


# ------------------------------------------------------------------------------------------------------------------- perfect heads
PERFECT = ("mug", 3, 2)                                                       # (category, objects, seed): one of scene_poses_ref.PERFECT_SCENES


def perfect_segment_scene(draw=None):
    """scene_poses_ref.perfect_scene's objects with the pairs drawn INSIDE the true objects (labels = the true object ids, every pair
    in the positive stratum): draw(members, seg_off, inst, n_points, n_pairs, seed) -> idx [P,2] (default: the restatement of the
    scene draw); every pair gets the closed-form outputs and heads of its object.  -> (scene dict, idx i64[P,2], outputs, heads)"""
    import scene_poses_ref as S
    syn = ST_REF.syn
    cat, n_obj, seed = PERFECT
    sc = S.perfect_scene(cat, n_obj, seed, pairs_per_object=64)               # (its own pair list is not used)
    cfg, pc, nrm, owner = sc["cfg"], sc["pc"], sc["nrm"], sc["owner"].astype(np.int32)
    members, seg_off = ST_REF.members_ref(owner, np.ones(n_obj, np.int32))
    n_pairs = 150000 * n_obj
    draw = draw or (lambda m, o, i, n, p, s: ST_REF.draw_ref(m, o, i, n, p, p, s))
    idx = np.asarray(draw(members, seg_off, owner, pc.shape[0], n_pairs, 11)).astype(np.int64)
    assert np.array_equal(owner[idx[:, 0]], owner[idx[:, 1]])
    outputs, heads = np.empty((n_pairs, 2), np.float32), np.zeros((n_pairs, 8), np.float32)
    for k, ob in enumerate(sc["obs"]):
        w = owner[idx[:, 0]] == k
        outputs[w] = syn.closed_form_outputs(pc, ob["center"], idx[w], cfg, quantise=False)
        heads[w] = syn.closed_form_heads(pc, nrm, idx[w], cfg, quantise=False, seed=k)
    return sc, idx, outputs, heads
