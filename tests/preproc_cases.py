"""Clouds and numpy definitions for the pre-processing row f3 (voxel de-duplication, neighbour search, PCA normals), shared by the
oracle's CPU tests (tests/test_oracle_golden.py) and the kernels' device tests (tests/test_gpu_preproc_edges.py).  Nothing here knows
the packed voxel key, the kernels' pruning or their cumulants: the expected values come from int64 index triples, a stable argsort and
np.linalg.eigh of a two-pass fp64 covariance."""
import numpy as np

F32 = np.float32


# ----------------------------------------------------------------------------------------------- voxel de-duplication
def voxel_index(pc, res):
    """v = floor((double)p / res) per axis, as float64 (so that NaN / inf survive)"""
    return np.floor(np.asarray(pc, F32).astype(np.float64) / float(res))


def in_range(pc, res):
    """the range contract of cppf_voxel_dedupe: every point finite and -2^20 <= v < 2^20 on all three axes"""
    v = voxel_index(pc, res)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(v) & (v >= -2.0 ** 20) & (v < 2.0 ** 20)))


def unique_first(pc, res):
    """sorted first occurrences of the int64 voxel index triples (finite clouds): what de-duplication must return"""
    v = voxel_index(pc, res).astype(np.int64)
    _, first = np.unique(v, axis=0, return_index=True)
    return np.sort(first)


def faces_cloud(res, n=4000, seed=0):
    """coordinates ON voxel faces: float32(m * res), a third one float32 step below, a third one step above"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-300, 300, (n, 3))
    p = (m.astype(np.float64) * res).astype(F32)
    step = rng.integers(0, 3, (n, 3))
    p = np.where(step == 1, np.nextafter(p, F32(-np.inf)), p)
    p = np.where(step == 2, np.nextafter(p, F32(np.inf)), p)
    return np.ascontiguousarray(p, F32)


def signs_cloud(res):
    """-0.0, +0.0 and mixed-sign points in the eight voxels around the origin (every combination per axis), each twice"""
    r = F32(res)
    lo = F32(res * (1 - 2.0 ** -20))                        # (just inside the voxel, whichever way float32(res) rounds)
    c = np.array([-0.0, 0.0, -1e-30, 1e-30, -0.5 * r, 0.5 * r, -lo, lo], F32)
    g = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([g, g[::-1]]), F32)


RANGE_RES = 0.5      # indices are exact in float32: 2^20 * 0.5 = 524288, and 524287.5 has 21 significant bits


def range_edge_cloud():
    """res = 0.5: on each axis the extreme indices -2^20 and 2^20 - 1, their inner neighbours, and a second point in each of
    those voxels -- all in range, 12 distinct voxels + the origin's"""
    rows = []
    for a in range(3):
        for v in (-2 ** 20, -2 ** 20 + 1, 2 ** 20 - 2, 2 ** 20 - 1):
            for frac in (0.0, 0.25):
                p = np.full(3, 0.1)
                p[a] = (v + frac * 2) * RANGE_RES         # frac 0.25 -> the middle of the voxel
                rows.append(p)
    rows.append(np.full(3, 0.1))
    return np.ascontiguousarray(np.array(rows), F32)


def refused_clouds():
    """[(name, cloud, res, finite)]: each has exactly one reason to be refused"""
    base = range_edge_cloud()
    out = []
    for a in range(3):
        for name, v in (("hi", 2 ** 20), ("lo", -2 ** 20 - 1)):
            p = np.full((1, 3), 0.1, F32)
            p[0, a] = v * RANGE_RES                        # 524288.0 / -524288.5: exact; masked keys would alias -2^20 / 2^20 - 1
            out.append((f"axis{a}_{name}", np.concatenate([base, p]), RANGE_RES, True))
    w = F32(0.004 * 2 ** 21)
    four = np.array([[0.1, 0.2, 0.3], [F32(0.1) + w, 0.2, 0.3], [5000, 0, 0], [F32(5000) - w, 0, 0]], F32)
    out.append(("four_point_alias", four, 0.004, True))
    rng = np.random.default_rng(5)
    for name, bad in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        p = rng.uniform(-0.2, 0.3, (300, 3)).astype(F32)
        p[257, 1] = bad
        out.append((name, p, 0.004, False))
    return out


SIZES = (1, 255, 256, 257, 1024, 1025)


def size_clouds(n, res=0.004, seed=0):
    """(all n points in one voxel, all n points in distinct voxels), both shuffled"""
    rng = np.random.default_rng(seed + n)
    one = (rng.uniform(0.1, 0.9, (n, 3)) * res + np.array([-3, 7, 175]) * res).astype(F32)
    i = rng.permutation(n)
    distinct = ((np.stack([i % 37 - 18, (i // 37) % 37 - 18, i // 1369], -1) + rng.uniform(0.2, 0.8, (n, 3))) * res).astype(F32)
    return one, distinct


# ----------------------------------------------------------------------------------------------- neighbour search
def knn_numpy(pc, k):
    """float32 keys (dx*dx + dy*dy) + dz*dz, stable argsort (ties -> lower index), first k, in ascending index order"""
    pc = np.asarray(pc, F32)
    d = pc[None, :, :] - pc[:, None, :]                    # d[q, j] = pc[j] - pc[q], float32
    key = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert key.dtype == F32
    return np.sort(np.argsort(key, axis=1, kind="stable")[:, :k], axis=1).astype(np.int32), key


def knn_candidates(key, k):
    """How many keys the search's pruning bound lets through per query (include/cppf.h, cppf_knn): the bound is the k-th smallest of
    the 64 minima over j = lane mod 64.  Used only to show that a case reaches the path it is meant for."""
    n = key.shape[0]
    pad = np.full((n, (-n) % 64), np.inf, F32)
    lane_min = np.concatenate([key, pad], 1).reshape(n, -1, 64).min(1)
    t0 = np.sort(lane_min, axis=1)[:, k - 1]
    return (key <= t0[:, None]).sum(1)


def clusters_cloud():
    """N = 1280 distinct points, point j in cluster j mod 64: every lane of the search sees one cluster, so the pruning bound is the
    distance to the k-th nearest CLUSTER and more than 512 candidates pass it"""
    rng = np.random.default_rng(11)
    centres = rng.uniform(-0.5, 0.5, (64, 3))
    pc = (centres[np.arange(1280) % 64] + rng.normal(0, 0.01, (1280, 3))).astype(F32)
    assert np.unique(pc, axis=0).shape[0] == 1280
    return pc


def lattice_cloud():
    """40 x 64 points at 4 mm pitch in raster order, z = 0.7: the order real masks arrive in; many exact distance ties"""
    r, c = np.mgrid[0:40, 0:64]
    return np.ascontiguousarray(np.stack([c * 0.004 - 0.128, r * 0.004 - 0.08, np.full(r.shape, 0.7)], -1).reshape(-1, 3), F32)


SMALL_NK = ((1, 1), (2, 2), (5, 3), (63, 60), (64, 64), (65, 64), (100, 1))


def small_cloud(n):
    return np.random.default_rng(100 + n).uniform(-0.1, 0.1, (n, 3)).astype(F32)


# ----------------------------------------------------------------------------------------------- normals
def eigh_reference(pc, nbrs):
    """np.linalg.eigh of the two-pass fp64 covariance of every neighbour set -> (e f64[N,3] unit eigenvector of the smallest
    eigenvalue, w f64[N,3] ascending eigenvalues, frob f64[N] = Frobenius norm of the raw second moment E[p p^T])"""
    q = np.asarray(pc, F32)[np.asarray(nbrs)].astype(np.float64)          # [N, k, 3]
    c = q - q.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c) / q.shape[1]
    w, v = np.linalg.eigh(cov)
    frob = np.linalg.norm(np.einsum("nki,nkj->nij", q, q) / q.shape[1], axis=(1, 2))
    return v[:, :, 0], w, frob


def normal_errors(nrm, pc, nbrs):
    """s = |n x e| per point, the per-point bound 2^-23 + (k + 3) 2^-53 ||E[pp^T]||_F / (l1 - l0) -- fp32 rounding of a unit vector
    with a margin of two + first-order perturbation of one-pass fp64 cumulants -- and the mask of points that HAVE a normal
    ((l1 - l0) / l2 > 1e-6)"""
    e, w, frob = eigh_reference(pc, nbrs)
    k = np.asarray(nbrs).shape[1]
    gap = w[:, 1] - w[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        defined = gap / w[:, 2] > 1e-6
        bound = 2.0 ** -23 + (k + 3) * 2.0 ** -53 * frob / gap
    s = np.linalg.norm(np.cross(np.asarray(nrm).astype(np.float64), e), axis=1)
    return s, bound, defined


def check_normals(nrm, pc, nbrs, surface, tag):
    """every point against eigh within its bound + the unconditional properties; -> the worst s among the compared points"""
    nrm = np.asarray(nrm)
    assert nrm.dtype == F32 and np.isfinite(nrm).all(), tag
    n64 = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1.0).max() <= 2.0 ** -23, (tag, "unit length")
    assert (nrm[np.arange(nrm.shape[0]), np.abs(nrm).argmax(1)] > 0).all(), (tag, "largest component positive")
    s, bound, defined = normal_errors(nrm, pc, nbrs)
    if surface:
        assert (~defined).mean() <= 0.01, (tag, "points without a defined normal", int((~defined).sum()))
    worst = float(s[defined].max()) if defined.any() else 0.0
    print(f"normals[{tag}]: worst s = {worst:.3g}, largest bound = {float(bound[defined].max()) if defined.any() else 0:.3g}, "
          f"skipped {int((~defined).sum())} of {nrm.shape[0]}")
    bad = defined & ~(s <= bound)
    assert not bad.any(), (tag, int(bad.sum()), float(s[bad].max()), float(bound[bad].min()))
    return worst


def _plane(n, seed, scale=1.0, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    n0 = np.array([0.3, -0.5, 0.8]); n0 /= np.linalg.norm(n0)
    a = np.cross(n0, [1, 0, 0]); a /= np.linalg.norm(a)
    b = np.cross(n0, a)
    p = rng.uniform(-0.1, 0.1, (n, 1)) * a + rng.uniform(-0.1, 0.1, (n, 1)) * b
    return (p * scale + np.asarray(offset, np.float64)).astype(F32)


def depth_surface_cloud():
    """a sloped surface seen by a camera, depth quantised to whole millimetres (48 x 60 pixels), in metres"""
    r, c = np.mgrid[200:248, 300:360].astype(np.float64)
    z = np.round(700 + 0.8 * (r - 200) + 0.5 * (c - 300))
    x, y = (c - 322.5) * z / 591.0, (r - 242.0) * z / 590.0
    return (np.stack([x, -y, -z], -1).reshape(-1, 3) / 1000.0).astype(F32)


def normal_clouds():
    """[(name, cloud, k, surface)] -- the clouds of the issue's table"""
    rng = np.random.default_rng(21)
    sph = rng.normal(size=(2000, 3))
    sph = (sph / np.linalg.norm(sph, axis=1, keepdims=True) * 0.05 + [0, 0, 1.0]).astype(F32)
    t = rng.uniform(-0.1, 0.1, (2000, 2))
    crease = np.stack([t[:, 0], t[:, 1], np.abs(t[:, 0]) * 0.7 + 0.9], -1).astype(F32)
    cube = rng.uniform(-0.1, 0.1, (2000, 3)).astype(F32)
    base = _plane(1500, 1)
    return [
        ("plane_origin", base, 30, True),
        ("plane_at_0.3_-0.2_1.2", _plane(1500, 1, offset=(0.3, -0.2, 1.2)), 30, True),
        ("plane_millimetres", _plane(1500, 1, scale=1000.0), 30, True),
        ("plane_offset_1000", _plane(1500, 1, offset=(1000, 1000, 1000)), 30, True),
        ("plane_x10_offset_3e4", _plane(1500, 1, scale=10.0, offset=(3e4, 3e4, 3e4)), 30, True),
        ("depth_quantised", depth_surface_cloud(), 30, True),
        ("sphere_5cm_at_1m", sph, 60, True),
        ("crease", crease, 30, True),
        ("solid_cube", cube, 30, False),
        ("k3", base, 3, True),
        ("k4", base, 4, True),
        ("k64", base, 64, True),
    ]


def tie_plane_cloud():
    """the lattice plane x + y = 0 (exact in float32): the two largest components of its normal are equal"""
    i, j = np.mgrid[-15:15, 0:30]
    h = 2.0 ** -8
    return np.ascontiguousarray(np.stack([i * h, -i * h, j * h], -1).reshape(-1, 3), F32)


def line_cloud():
    t = np.arange(200, dtype=np.float64)[:, None]
    return (t * np.array([0.25, 0.5, -0.125]) * 2.0 ** -6).astype(F32)          # exact in float32: a straight line
