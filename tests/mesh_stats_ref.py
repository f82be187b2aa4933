"""numpy restatement of csrc/mesh_stats.hip (include/cppf.h "Mesh statistics"), operation for operation, and of gen_stats.py's
per-pair arithmetic and reduction:

- areas, the blocked sums of the stated order, the std::round counts, the first-face rule, the status word, the Philox uniforms
  and the barycentric points of cppf_surface_sample_batch;
- the bounding box, the Philox pairs, generate_target's fp64 arithmetic and the maxima of cppf_mesh_vote_stats_batch;
- gen_stats.py's aggregation over meshes (cppf_amd.mesh_stats.aggregate is the product's; this one is typed out again)."""
import numpy as np

from cppf_amd import mesh_stats as MS

LANES = 1024                       # MS_SCAN_THREADS: the block count of the stated summation order


def areas(vertices, faces):
    """a_t = 0.5 sqrt((c0^2 + c1^2) + c2^2), c = (v0 - v1) x (v0 - v2)"""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    x, y = p0 - p1, p0 - p2
    c0 = x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1]
    c1 = x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2]
    c2 = x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]
    return 0.5 * np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)


def _blocks(x):
    """x padded with zeros to LANES * K and split into the LANES blocks of K = ceil(F / LANES) (adding +0.0 to a value >= 0 leaves
    it unchanged, so the padding does not change any sum)"""
    F = x.shape[0]
    K = -(-F // LANES)
    out = np.zeros(LANES * K, np.float64)
    out[:F] = x
    return out.reshape(LANES, K)


def blocked_total(x):
    """((0 + s_0) + s_1) ... + s_1023, s_l = ((0 + x) + x) ... over block l"""
    B = _blocks(x)
    s = np.zeros(LANES, np.float64)
    for j in range(B.shape[1]):
        s = s + B[:, j]
    tot = 0.0
    for l in range(LANES):
        tot = tot + s[l]
    return np.float64(tot)


def blocked_cumsum(q):
    """C_t: within block l, ((B_l + q) + q) ... left to right; B_0 = 0, B_l = B_l-1 + T_l-1"""
    F = q.shape[0]
    Q = _blocks(q)
    T = np.zeros(LANES, np.float64)
    for j in range(Q.shape[1]):
        T = T + Q[:, j]
    B = np.zeros(LANES, np.float64)
    b = 0.0
    for l in range(LANES):
        B[l] = b
        b = b + T[l]
    C = np.empty_like(Q)
    c = B.copy()
    for j in range(Q.shape[1]):
        c = c + Q[:, j]
        C[:, j] = c
    return C.reshape(-1)[:F]


def round_half_away(x):
    """std::round for x >= 0: halves away from zero (np.round would round them to even)"""
    t = np.trunc(x)
    return t + ((x - t) >= 0.5)


def counts_end(C, n):
    """E_t = min(N, round(C_t N)), E_last = N"""
    E = np.minimum(float(n), round_half_away(C * float(n))).astype(np.int64)
    E[-1] = n
    return E


def sample_status(vertices, faces):
    """the status word of cppf_surface_sample_batch for one mesh: bit 2 = a face index outside [0, nv); bit 1 = the blocked total S
    is not in (0, inf).  A face with an index outside has the area NaN, so S is NaN and bit 2 never comes without bit 1."""
    return _areas_total_status(np.asarray(vertices, np.float64), np.asarray(faces, np.int64))[2]


def _areas_total_status(v, f):
    outside = ((f < 0) | (f >= v.shape[0])).any(1)
    with np.errstate(over="ignore", invalid="ignore"):
        a = areas(v, np.where(outside[:, None], 0, f))
        a[outside] = np.nan
        S = blocked_total(a)
    return a, S, (0 if S > 0 and S < np.inf else 1) | (2 if outside.any() else 0)


def sample_surface(vertices, faces, n, seed, mesh=0):
    """cppf_surface_sample_batch for one mesh at batch index `mesh`: (points f64[n,3], face ids i64[n], E i64[F], ok).  ok False:
    the total area is not in (0, inf) and the device writes NaN.  E is returned as step 4 defines it and may decrease by one
    behind a block boundary; the face of point k is the first t with E_t > k, which is the first t whose running maximum exceeds
    k -- a bisection of the running maximum, never of E itself."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    a, S, status = _areas_total_status(v, f)
    if status != 0:
        return np.full((n, 3), np.nan), np.full(n, -1), None, False
    q = a / S
    E = counts_end(blocked_cumsum(q), n)
    k = np.arange(n)
    t = np.searchsorted(np.maximum.accumulate(E), k, side="right")  # the first t with E_t > k
    r1, r2 = MS.surface_uniforms(seed, mesh, n)
    s = np.sqrt(r1)
    wa, wb, wc = 1.0 - s, s * (1.0 - r2), s * r2
    p0, p1, p2 = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
    pts = (wa[:, None] * p0 + wb[:, None] * p1) + wc[:, None] * p2
    return pts, t, E, True


def open3d_counts(C, n):
    """Open3D's loop (SamplePointsUniformlyImpl): point_idx runs up to round(C_t n) on face t -> the count of every face"""
    cnt, idx = np.zeros(C.shape[0], np.int64), 0
    for t, c in enumerate(C):
        e = int(round_half_away(np.float64(c) * n))
        if e > idx:
            cnt[t] = e - idx
            idx = e
    return cnt


def pair_targets(a, b):
    """generate_target's targets_tr in fp64 before its float32 cast: (proj_len, dist2o), in its operation order"""
    d = a - b
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    u = d / (nrm + 1e-7)[:, None]
    proj = (a[:, 0] * u[:, 0] + a[:, 1] * u[:, 1]) + a[:, 2] * u[:, 2]
    o = a - proj[:, None] * u
    return proj, np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])


def centre(pts):
    lo, hi = pts.min(0), pts.max(0)
    return (lo + hi) / 2


def mesh_row(pts, idx):
    """cppf_mesh_vote_stats_batch's row for points f64[N,3] and pairs idx[P,2]: {diag, f32(max|proj|), f32(max dist2o), half}"""
    c = centre(pts)
    pc = pts - c
    hc, lc = pc.max(0), pc.min(0)
    e = hc - lc
    diag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    proj, dist = pair_targets(pc[idx[:, 0]], pc[idx[:, 1]])
    return np.array([diag, np.float32(np.abs(proj).max()), np.float32(dist.max()), *hc], np.float64)


def vote_stats(pts, n_pairs, seed, mesh=0):
    """cppf_mesh_vote_stats_batch for one mesh at batch index `mesh` (Philox pairs)"""
    return mesh_row(pts, MS.stats_pairs(seed, mesh, n_pairs, pts.shape[0]))


def aggregate(rows):
    """gen_stats.py:37-57 over the rows"""
    scale_range, vote_range, scale_mean = [np.inf, -np.inf], [0, 0], []
    for r in rows:
        scale_range = [min(scale_range[0], r[0]), max(scale_range[1], r[0])]
        vote_range = [max(vote_range[0], np.float32(r[1])), max(vote_range[1], np.float32(r[2]))]
        scale_mean.append(r[3:6])
    return dict(scale_range=scale_range, vote_range=vote_range, scale_mean=np.mean(scale_mean, 0))
