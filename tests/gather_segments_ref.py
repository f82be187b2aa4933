"""What cppf_gather_segments (csrc/instances.hip) and segments.segment_clouds are held to, in numpy, with a plain Python loop beside it
for the restatement itself (tests/test_gather_segments_cpu.py), and the clouds and label patterns of both test files.

  segment of a point   labels[i] when 0 <= labels[i] < S, else none (-1, S, INT32_MAX, INT32_MIN: skipped, never an error)
  offsets              exclusive prefix of the segments' point counts
  pts / nrm / src      a STABLE argsort of the points on their label: segment s's points in increasing dense index at rows
                       offsets[s]:offsets[s+1]; rows >= capacity dropped
  bounds[s]            {min x, y, z, max x, y, z} over the segment's points whose three coordinates are all finite, ordered by the
                       sign-magnitude integer key of the float (-0.0 below +0.0); {+inf x 3, -inf x 3} when there is no such point
  chunk_counts[c][s]   segment s's points in the chunks (of 1024 points) before chunk c -- what the call leaves in its intermediate"""
import numpy as np

F32 = np.float32
POISON_F, POISON_I = F32(-7.5), np.int32(-77)
CHUNK = 1024
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY_BOUNDS = np.array([np.inf] * 3 + [-np.inf] * 3, F32)


def key(x):
    """i64: the sign-magnitude integer key of float32 values -- monotone in the float order, and key(-0.0) = -1 < 0 = key(+0.0)"""
    b = np.ascontiguousarray(np.asarray(x, F32)).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, b ^ 0x7FFFFFFF)


def unkey(k):
    """the float32 values of keys (the map is its own inverse on the 32-bit patterns)"""
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k, k ^ 0x7FFFFFFF).astype(np.int32).view(F32)


def in_range(labels, S):
    labels = np.asarray(labels, np.int32).reshape(-1)
    return (labels >= 0) & (labels < int(S))


def gather_segments_ref(hi, nrm, labels, S, capacity=None):
    """-> dict(offsets i32[S+1], pts f32[cap,3], nrm f32[cap,3], src i32[cap], bounds f32[S,6], chunk_counts i32[n_chunks,S]).  Rows the
    call leaves alone hold POISON_F / POISON_I (what the device test fills its buffers with beforehand)."""
    hi, nrm = np.asarray(hi, F32).reshape(-1, 3), np.asarray(nrm, F32).reshape(-1, 3)
    labels = np.asarray(labels, np.int32).reshape(-1)
    M, S = hi.shape[0], int(S)
    cap = M if capacity is None else int(capacity)
    ok = in_range(labels, S)
    rows = np.nonzero(ok)[0]
    rows = rows[np.argsort(labels[rows], kind="stable")]                      # the stable partition
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels[ok], minlength=S)[:S])]).astype(np.int32)
    out = dict(pts=np.full((cap, 3), POISON_F, F32), nrm=np.full((cap, 3), POISON_F, F32), src=np.full(cap, POISON_I, np.int32))
    n = min(cap, rows.size)
    out["pts"][:n], out["nrm"][:n], out["src"][:n] = hi[rows[:n]], nrm[rows[:n]], rows[:n]
    finite = ok & np.isfinite(hi).all(1)
    kb = np.tile(key(EMPTY_BOUNDS), (S, 1))                                   # min / max of the keys, then the floats with those keys
    np.minimum.at(kb[:, :3], labels[finite], key(hi[finite]))
    np.maximum.at(kb[:, 3:], labels[finite], key(hi[finite]))
    bounds = unkey(kb)
    n_chunks = (M + CHUNK - 1) // CHUNK
    per = np.zeros((n_chunks, S), np.int64)
    np.add.at(per, (rows // CHUNK, labels[rows]), 1)
    before = np.cumsum(per, 0) - per
    return dict(out, offsets=offsets, bounds=bounds, chunk_counts=before.astype(np.int32))


def gather_segments_loop(hi, nrm, labels, S):
    """offsets, the packed rows and the bounds by plain loops (roomy capacity); the bounds compare (sign, magnitude) pairs taken from
    the floats' bit patterns, not the floats"""
    hi, nrm = np.asarray(hi, F32).reshape(-1, 3), np.asarray(nrm, F32).reshape(-1, 3)
    lists = [[] for _ in range(S)]
    for i, l in enumerate(labels):
        if 0 <= int(l) < S:
            lists[int(l)].append(i)
    offsets = [0]
    for s in range(S):
        offsets.append(offsets[-1] + len(lists[s]))
    flat = [i for l in lists for i in l]

    def order(v):                                                             # sign-magnitude: negatives by descending magnitude first
        b = int(np.array(v, F32).view(np.uint32))
        sign, mag = b >> 31, b & 0x7FFFFFFF
        return (0, -mag) if sign else (1, mag)
    bounds = []
    for s in range(S):
        lo, hi_ = [float("inf")] * 3, [float("-inf")] * 3
        lo, hi_ = [F32(v) for v in lo], [F32(v) for v in hi_]
        for i in lists[s]:
            p = hi[i]
            if not all(np.isfinite(c) for c in p):
                continue
            for e in range(3):
                if order(p[e]) < order(lo[e]):
                    lo[e] = p[e]
                if order(p[e]) > order(hi_[e]):
                    hi_[e] = p[e]
        bounds.append(lo + hi_)
    return (np.array(offsets, np.int32), hi[flat].reshape(-1, 3), nrm[flat].reshape(-1, 3), np.array(flat, np.int32),
            np.array(bounds, F32).reshape(S, 6))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def cloud(M, seed=0, specials=True):
    """hi, nrm f32[M,3]: standard-normal coordinates of both signs; with specials about one coordinate in twelve is one of +0.0, -0.0,
    NaN, +inf, -inf (the bounds' order of the zeros and the points they must leave out)"""
    rng = np.random.default_rng(seed)
    hi = rng.standard_normal((M, 3)).astype(F32)
    nrm = rng.standard_normal((M, 3)).astype(F32)
    if specials:
        vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.0, -0.0], F32)
        where = rng.random((M, 3)) < 1.0 / 12.0
        hi[where] = vals[rng.integers(0, vals.size, int(where.sum()))]
    return hi, nrm


PATTERNS = ("one", "lanes", "runs", "mixed", "empty")


def labels_case(pattern, M, S, seed=0):
    """i32[M]:
      one     every point the same label (S // 2)
      lanes   every lane of a wave its own label: min(S, 64) distinct labels per wave, the wave's labels shifted from wave to wave --
              the rank loop's worst case
      runs    runs of one label, of lengths that straddle the wave (64) and chunk (1024) boundaries, labels not monotone
      mixed   random labels with -1, S, INT32_MAX and INT32_MIN mixed in (about a third of the points in no segment)
      empty   random labels that leave out segments 0, S // 2 and S - 1 (S = 1: every point in no segment)"""
    rng = np.random.default_rng(seed)
    i = np.arange(M)
    if pattern == "one":
        lab = np.full(M, S // 2)
    elif pattern == "lanes":
        lab = ((i % 64) + 7 * (i // 64)) % S
    elif pattern == "runs":
        lab, pos, j = np.zeros(M, np.int64), 0, 0
        lengths = (37, 27, 65, 1, 130, 700, 63, 64, 1100, 5)                  # ends at 37, 64, 129, 130, 260, 960, 1023, 1087, 2187, ...
        while pos < M:
            n = lengths[j % len(lengths)]
            lab[pos:pos + n] = (j * 389 + 3) % S
            pos, j = pos + n, j + 1
    elif pattern == "mixed":
        lab = rng.integers(0, S, M)
        out = rng.random(M) < 1.0 / 3.0
        lab[out] = np.array([-1, S, INT32_MAX, INT32_MIN])[rng.integers(0, 4, int(out.sum()))]
    elif pattern == "empty":
        allowed = np.array([s for s in range(S) if s not in (0, S // 2, S - 1)] or [-1])
        lab = allowed[rng.integers(0, allowed.size, M)]
    else:
        raise ValueError(pattern)
    return lab.astype(np.int32)
