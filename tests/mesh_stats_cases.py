"""Case builders for the edges of csrc/mesh_stats.hip (numpy only, no device): meshes whose end counts E decrease behind a block
boundary, batches that put the face loops, the pair loop and the final kernel on a later trip, strip meshes at the block edges
of the stated summation order, and meshes / point sets for every status leg.  That each case reaches the edge it is named for is
shown with the restatement alone in tests/test_mesh_stats_cases_cpu.py; the device is held to the same cases in
tests/test_gpu_mesh_stats_edges.py."""
import functools

import numpy as np

import mesh_ref as R
import mesh_stats_ref as SR

LANES = SR.LANES
THREADS = 256                       # MS_THREADS
FACE_GRID_CAP = 8192                # workgroups of ms_area_kernel / ms_norm_kernel: 8192 x 256 faces per trip
PAIR_BLOCKS_TARGET = 4096           # MS_PAIR_BLOCKS_TARGET


# ------------------------------------------------------------------------------------------------ strip meshes
def strip_mesh(F, seed, p_face=0.3, p_block=0.0, zero_first=False, zero_last=False):
    """a triangle strip f_t = (t, t+1, t+2) over F + 2 uniform random points.  A face is made degenerate by repeating its second
    vertex (its area is then exactly 0): each face with probability p_face, each whole block of K = ceil(F / 1024) faces of the
    stated order with probability p_block, and the first / last face on request."""
    rng = np.random.default_rng(seed)
    v = rng.random((F + 2, 3))
    t = np.arange(F, dtype=np.int32)
    f = np.stack([t, t + 1, t + 2], 1)
    deg = rng.random(F) < p_face
    if p_block > 0:
        K = -(-F // LANES)
        deg |= np.repeat(rng.random(LANES) < p_block, K)[:F]
    if F > 1:                       # (a one-face mesh keeps its area)
        deg[0], deg[-1] = zero_first or deg[0], zero_last or deg[-1]
        if deg.all():
            deg[F // 2] = False
    else:
        deg[:] = False
    f[deg, 2] = f[deg, 1]
    return v, np.ascontiguousarray(f)


def cumulative(v, f):
    """C of include/cppf.h step 3 for a mesh, by the restatement"""
    a = SR.areas(v, f)
    return SR.blocked_cumsum(a / SR.blocked_total(a))


def kernel_bisection(E, k):
    """ms_points_kernel's search as it stood before E was stored as its running maximum, line by line"""
    lo, hi = 0, len(E) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if E[mid] > k:
            hi = mid
        else:
            lo = mid + 1
    return lo


def first_decrease(C, n_max=1 << 22, chunk=1 << 20):
    """the smallest N < n_max for which E = counts_end(C, N) decreases somewhere, and the first such place: (N, t) with
    E_t > E_t+1, or None.  Only places where C itself decreases can qualify (round and min are monotonic); vectorised over N."""
    dips = np.flatnonzero(C[1:] < C[:-1])
    dips = dips[dips + 1 < C.shape[0] - 1]                # (E_last = N is set, not computed)
    if dips.size == 0:
        return None
    for n0 in range(1, n_max, chunk):
        N = np.arange(n0, min(n_max, n0 + chunk), dtype=np.float64)
        hi = np.minimum(N, SR.round_half_away(C[dips, None] * N))
        lo = np.minimum(N, SR.round_half_away(C[dips + 1, None] * N))
        hit = (hi > lo).any(0)
        if hit.any():
            j = int(np.argmax(hit))
            return int(N[j]), int(dips[np.argmax(hi[:, j] > lo[:, j])])
    return None


PLAIN = dict(p_face=0.3)                         # the issue's strips: 30 % of the faces degenerate
BLOCKY = dict(p_face=0.15, p_block=0.35)         # whole blocks degenerate as well: the lower count stays for several faces


def search_dips(F, seeds, **kw):
    """the search DIP_CASES came from: strip_mesh(F, seed, **kw) for each seed, yielding dict(F, seed, kw, N, t) where an
    N < 2^22 makes the restated E decrease (about 2 s a mesh)"""
    for seed in seeds:
        hit = first_decrease(cumulative(*strip_mesh(F, seed, **kw)))
        if hit is not None:
            yield dict(F=F, seed=seed, kw=kw, N=hit[0], t=hit[1])


# Fixed results of search_dips: E_t = E_t+1 + 1 at the smallest such N.  `late`: the face ms_points_kernel's bisection of E itself
# gave point k = E_t+1 (a probe fell inside the dip), where the first face with E_t > k is `first`; None: it landed on the first.
DIP_CASES = [
    dict(F=3072, seed=21, kw=PLAIN, N=1416377, t=818, first=818, late=None),
    dict(F=2048, seed=465, kw=BLOCKY, N=319276, t=1765, first=1765, late=1770),
    dict(F=2048, seed=454, kw=BLOCKY, N=2842361, t=1717, first=1717, late=1721),
]


@functools.lru_cache(maxsize=None)
def dip_case(i):
    """(vertices, faces, C, E) of DIP_CASES[i]"""
    c = DIP_CASES[i]
    v, f = strip_mesh(c["F"], c["seed"], **c["kw"])
    C = cumulative(v, f)
    return v, f, C, SR.counts_end(C, c["N"])


DIP_SEED = 3


@functools.lru_cache(maxsize=None)
def dip_sample(i):
    """the restatement's (points, face ids) of DIP_CASES[i] at its N, seed DIP_SEED, mesh 0 (computed once: the Philox twin
    takes about a second per million points)"""
    v, f, _, _ = dip_case(i)
    pts, t, _, ok = SR.sample_surface(v, f, DIP_CASES[i]["N"], DIP_SEED, 0)
    assert ok
    return pts, t


def dip_points(E, t):
    """the three points around a decrease E_t > E_t+1: the last before the lower count, the one the dip hides, the last of face t"""
    return [int(E[t + 1]) - 1, int(E[t + 1]), int(E[t]) - 1]


# ------------------------------------------------------------------------------------------------ second trips: faces
@functools.lru_cache(maxsize=None)
def face_trip_batch():
    """two meshes whose 2 101 344 faces are more than one trip of ms_area_kernel / ms_norm_kernel (8192 x 256 lanes): the second
    mesh's faces lie on both sides of global face 2 097 152"""
    return [R.uv_sphere(0.5, 1024, 1024), R.uv_sphere(0.3, 40, 80)]


def face_offsets(meshes):
    return np.concatenate([[0], np.cumsum([f.shape[0] for _, f in meshes])]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ second trips: pairs
def pair_blocks(M, P):
    """ms_pair_blocks: workgroups of ms_pairs_kernel per mesh; one trip of its stride loop is pair_blocks * 256 pairs"""
    return min(-(-P // THREADS), -(-PAIR_BLOCKS_TARGET // M))


# The kernel reduces with fmax, so a dropped trip shows only in a row whose maximum lies in it.  The seeds are the first for which
# the condition of test_mesh_stats_cases_cpu.py holds (seeds 0 .. 14 of four_trips leave no row's maximum among its last 5 pairs;
# seed 5 of grid_cap has both maxima among the first 1 048 576 pairs).
PAIR_CASES = {
    "three_trips": dict(M=512, N=97, P=2 * 8 * 256 + 77, seed=5, nb=8, trips=3),           # the last trip: 77 pairs
    "four_trips": dict(M=300, N=97, P=3 * 14 * 256 + 5, seed=15, nb=14, trips=4),          # the last trip: 5 pairs
    "grid_cap": dict(M=1, N=65536, P=2 * 4096 * 256 + 333, seed=7, nb=4096, trips=3),      # the launch at its cap, 333 pairs left
}


@functools.lru_cache(maxsize=None)
def pair_points(name):
    """the point sets f64[M,N,3] of a pair case: default_rng(1).normal(0, 0.1), drawn mesh by mesh"""
    c = PAIR_CASES[name]
    rng = np.random.default_rng(1)
    return np.stack([rng.normal(0, 0.1, (c["N"], 3)) for _ in range(c["M"])])


@functools.lru_cache(maxsize=None)
def pair_rows(name, seed=None):
    """the restatement's rows f64[M,6] of a pair case over (full) all P pairs, (first) the pairs [0, nb * 256) of the stride loop's
    first trip and (whole) the pairs of its whole trips, without the ragged last one"""
    from cppf_amd import mesh_stats as MS
    c = PAIR_CASES[name]
    seed = c["seed"] if seed is None else seed
    trip = c["nb"] * THREADS
    pts, out = pair_points(name), dict(full=[], first=[], whole=[])
    for m in range(c["M"]):
        idx = MS.stats_pairs(seed, m, c["P"], c["N"])
        out["full"].append(SR.mesh_row(pts[m], idx))
        out["first"].append(SR.mesh_row(pts[m], idx[:trip]))
        out["whole"].append(SR.mesh_row(pts[m], idx[:(c["P"] // trip) * trip]))
    return {k: np.array(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ block edges
EDGE_FS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049)     # K = ceil(F / 1024) goes 1 -> 2 at 1025 and 2 -> 3 at 2049
EDGE_NS = (1, 255, 256, 257)                             # one lane, one workgroup of ms_points_kernel short, full, and one over


@functools.lru_cache(maxsize=None)
def edge_meshes():
    """a strip mesh per face count of EDGE_FS, a fifth of the faces degenerate; a zero-area first face at 2 / 1024 / 2047 / 2049
    faces, a zero-area last face at 1024 / 2048"""
    return [strip_mesh(F, 100 + i, p_face=0.2, zero_first=i % 2 == 1, zero_last=i in (3, 6)) for i, F in enumerate(EDGE_FS)]


# ------------------------------------------------------------------------------------------------ status legs
STATUS_WORDS = [0, 3, 3, 1, 1, 0, 0]


@functools.lru_cache(maxsize=None)
def status_batch():
    """good meshes mixed with: a face index of -1; one equal to nv; a referenced NaN vertex; coordinates of 1e200 (the areas
    overflow); an unreferenced NaN vertex (status 0).  Their status words: STATUS_WORDS."""
    v, f = strip_mesh(1500, 7)
    neg, over = f.copy(), f.copy()
    neg[700, 1] = -1
    over[1499, 2] = v.shape[0]
    v_nan = v.copy()
    v_nan[f[10, 0], 1] = np.nan
    assert SR.areas(v, f)[10] > 0
    v_unref = np.vstack([v, [[np.nan, 0.0, np.inf]]])
    return [R.box()[:2], (v, neg), (v, over), (v_nan, f), (v * 1e200, f), (v_unref, f), R.uv_sphere(0.5, 16, 32)]


BAD_NS = (1, 2, 255, 257, 2048)
BAD_AT = (0, 255, 256, -1)
BAD_VALUES = (np.nan, np.inf, -np.inf)


def bad_point_batch(N):
    """point sets f64[M,N,3] for cppf_mesh_vote_stats_batch and the status each must get: good sets alternating with sets that hold
    ONE non-finite coordinate, at each point index of BAD_AT that exists and with each value of BAD_VALUES"""
    rng = np.random.default_rng(N)
    sets, status = [rng.normal(0, 0.1, (N, 3))], [0]
    for j, at in enumerate(sorted({a % N for a in BAD_AT if -N <= a < N})):
        for i, val in enumerate(BAD_VALUES):
            p = rng.normal(0, 0.1, (N, 3))
            p[at, (i + j) % 3] = val
            sets += [p, rng.normal(0, 0.1, (N, 3))]
            status += [1, 0]
    return np.stack(sets), status


# ------------------------------------------------------------------------------------------------ counter and host edges
FIRST_MESH_TOP = 2 ** 32 - 3        # with three meshes the last one draws as mesh 2^32 - 1, the largest counter word
EINVAL = -1                         # CPPF_EINVAL (include/cppf.h)
