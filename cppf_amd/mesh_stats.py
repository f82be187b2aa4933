"""Voting statistics of a category from its meshes: the reference's gen_stats.py on the device, and the config a new category trains
with.

gen_stats.py samples 2048 points on each mesh's surface (Open3D's sample_points_uniformly), centres them on their bounding box,
runs generate_target on 100 000 random pairs and keeps, per mesh, the bbox diagonal, max |proj_len|, max dist2o and the half
extents; over the meshes it prints scale_range = [min diag, max diag], vote_range = [max of the two maxima] and scale_mean = the
mean half extents.  Here the sampling (cppf_surface_sample_batch) and the per-mesh statistics (cppf_mesh_vote_stats_batch) run
for a whole batch of meshes in one launch sequence each (csrc/mesh_stats.hip; the arithmetic: include/cppf.h "Mesh statistics"),
the rows come back in one host read, and the aggregation over meshes is gen_stats.py's, in numpy.

derive_config turns those figures into a CategoryConfig that MeshViewSampler trains on consistently -- a rule of this project, not
of the reference (see its docstring)."""
import os

import numpy as np
import torch

from . import _lib
from ._torch_util import call, canon, require_cuda, scratch, workspace
from .config import CategoryConfig
from .synthetic import philox4x32_10

STREAM_POINTS, STREAM_PAIRS = 2, 3          # Philox counter word 2 of the two draws (include/cppf.h); 0 and 1 are cppf_sample_pairs'
STAT_COLUMNS = ("diag", "max_abs_proj", "max_dist2o", "half_x", "half_y", "half_z")
MAX_FACES_PER_CALL = 1 << 26                 # a batch is split so that one call's faces stay below this (workspace ~ 12 B / face)


class MeshStatsError(ValueError):
    pass


# ----------------------------------------------------------------------------------------------------------------- host twins
def u53(w0, w1):
    """include/cppf.h u53: ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, a double in [0, 1)"""
    m = ((np.asarray(w0, np.uint64) >> np.uint64(5)) << np.uint64(26)) | (np.asarray(w1, np.uint64) >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


def surface_uniforms(seed, mesh, n_points):
    """the (r1, r2) f64[n_points] cppf_surface_sample_batch draws for point k of mesh `mesh` (= first_mesh + batch position):
    Philox({k, mesh, 2, 0}) keyed by seed"""
    k = np.arange(int(n_points), dtype=np.uint64)
    w = philox4x32_10([k, np.uint64(mesh), np.uint64(STREAM_POINTS), np.uint64(0)], seed)
    return u53(w[0], w[1]), u53(w[2], w[3])


def stats_pairs(seed, mesh, n_pairs, n_points):
    """the pairs i64[n_pairs,2] cppf_mesh_vote_stats_batch draws for mesh `mesh`: Philox({p, mesh, 3, 0}), index = (word N) >> 32"""
    p = np.arange(int(n_pairs), dtype=np.uint64)
    w = philox4x32_10([p, np.uint64(mesh), np.uint64(STREAM_PAIRS), np.uint64(0)], seed)
    N, s32 = np.uint64(int(n_points)), np.uint64(32)
    return np.stack([(w[0] * N) >> s32, (w[1] * N) >> s32], -1).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------- device calls
def _pack(meshes):
    """(verts f64[V,3], faces i32[F,3], vert_off i64[M+1], face_off i64[M+1]) of a list of (vertices, faces)"""
    vs = [np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1, 3)) for v, _ in meshes]
    fs = [np.ascontiguousarray(np.asarray(f, np.int32).reshape(-1, 3)) for _, f in meshes]
    voff = np.zeros(len(meshes) + 1, np.int64)
    foff = np.zeros(len(meshes) + 1, np.int64)
    voff[1:] = np.cumsum([v.shape[0] for v in vs])
    foff[1:] = np.cumsum([f.shape[0] for f in fs])
    return np.concatenate(vs), np.concatenate(fs), voff, foff


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", 0)


def upload_meshes(meshes, device=None):
    """a list of (vertices f64[V,3], faces i32[F,3]) host arrays -> (verts, faces) concatenated device tensors and the host offsets
    (vert_off, face_off) i64[M+1] that cppf_surface_sample_batch takes"""
    for k, (v, f) in enumerate(meshes):
        if np.asarray(f).size == 0 or np.asarray(v).size == 0:
            raise MeshStatsError(f"mesh {k}: no faces or no vertices")
    dev = _device(device)
    v, f, voff, foff = _pack(meshes)
    return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), voff, foff


def sample_surface_packed(verts, faces, vert_off, face_off, n_points, seed=0, first_mesh=0):
    """cppf_surface_sample_batch on uploaded meshes (upload_meshes): (points f64[M,n,3], face_ids i32[M,n], status i32[M]) device
    tensors, no host synchronisation"""
    require_cuda()
    dev = verts.device
    verts, faces = canon(verts, torch.float64, dev, "verts", (3,)), canon(faces, (torch.int32,), dev, "faces", (3,))
    M = len(face_off) - 1
    vert_off, face_off = np.ascontiguousarray(vert_off, np.int64), np.ascontiguousarray(face_off, np.int64)
    pts = torch.empty((M, int(n_points), 3), dtype=torch.float64, device=dev)
    fid = torch.empty((M, int(n_points)), dtype=torch.int32, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    ws = workspace(_lib.lib().cppf_surface_sample_workspace_bytes(M, int(face_off[-1])), dev, "surface_sample")
    call("cppf_surface_sample_batch", dev, verts, faces, vert_off, face_off, M, int(n_points), int(seed) & 0xFFFFFFFFFFFFFFFF,
         int(first_mesh), pts, fid, status, scratch(ws))
    return pts, fid, status


def sample_surface_batch(meshes, n_points, seed=0, first_mesh=0, device=None):
    """cppf_surface_sample_batch on a list of (vertices f64[V,3], faces i32[F,3]) host arrays: (points f64[M,n,3], face_ids
    i32[M,n], status i32[M]) device tensors, no host synchronisation.  Mesh m draws as mesh index first_mesh + m.  status bit 1:
    the mesh's total area is zero or not finite, bit 2: a face index outside its vertices (that mesh's points are NaN).  Bit 2
    comes with bit 1 (status 3): the offending face's area is NaN and so is the total."""
    require_cuda()
    return sample_surface_packed(*upload_meshes(meshes, device), n_points, seed, first_mesh)


def _status_text(bits):
    why = []
    if bits & 1:
        why.append("its total surface area is zero or not finite (every face degenerate, or a NaN / inf vertex)")
    if bits & 2:
        why.append("a face index lies outside its vertices")
    return " and ".join(why) or f"status {bits}"


def sample_surface(vertices, faces, n, seed=0, device=None, return_faces=False):
    """n points on the surface of one mesh, area-weighted (Open3D's SamplePointsUniformly; include/cppf.h): device f64[n,3]
    (and the face index i32[n] of each point with return_faces).  A mesh with no area raises MeshStatsError."""
    pts, fid, status = sample_surface_batch([(vertices, faces)], n, seed, 0, device)
    bits = int(status.item())
    if bits:
        raise MeshStatsError(f"mesh: {_status_text(bits)}")
    return (pts[0], fid[0]) if return_faces else pts[0]


def vote_stats_batch(points, n_pairs=100000, seed=0, first_mesh=0):
    """cppf_mesh_vote_stats_batch on device points f64[M,N,3]: (stats f64[M,6] (STAT_COLUMNS), status i32[M]) device tensors"""
    require_cuda()
    points = canon(points, torch.float64, points.device, "points", (3,))
    assert points.dim() == 3
    M, N = int(points.shape[0]), int(points.shape[1])
    dev = points.device
    stats = torch.empty((M, 6), dtype=torch.float64, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    ws = workspace(_lib.lib().cppf_mesh_vote_stats_workspace_bytes(M, N, int(n_pairs)), dev, "mesh_vote_stats")
    call("cppf_mesh_vote_stats_batch", dev, points, M, N, int(n_pairs), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_mesh), stats, status,
         scratch(ws))
    return stats, status


def _chunks(meshes, max_faces):
    out, cur, nf = [], [], 0
    for k, (_, f) in enumerate(meshes):
        n = int(np.asarray(f).reshape(-1, 3).shape[0])
        if cur and nf + n > max_faces:
            out.append(cur)
            cur, nf = [], 0
        cur.append(k)
        nf += n
    if cur:
        out.append(cur)
    return out


# ----------------------------------------------------------------------------------------------------------------- gen_stats.py
def aggregate(rows):
    """gen_stats.py's reduction over meshes, on rows f64[M,6] (STAT_COLUMNS): scale_range = [min diag, max diag] (starting from
    [inf, -inf]), vote_range = [max(0, max|proj|), max(0, max dist2o)] over float32 values, scale_mean = the mean of the half
    extents"""
    scale_range = [np.inf, -np.inf]
    vote_range = [0, 0]
    scale_mean = []
    for r in np.asarray(rows, np.float64):
        diag = np.float64(r[0])
        scale_range[0] = min(scale_range[0], diag)
        scale_range[1] = max(scale_range[1], diag)
        vote_range[0] = max(vote_range[0], np.float32(r[1]))
        vote_range[1] = max(vote_range[1], np.float32(r[2]))
        scale_mean.append(r[3:6])
    return dict(scale_range=scale_range, vote_range=vote_range, scale_mean=np.mean(scale_mean, 0))


def format_stats(agg):
    """the three lines gen_stats.py prints"""
    lst = lambda xs: "[" + ", ".join(str(x) if isinstance(x, (int, np.float32)) else repr(float(x)) for x in xs) + "]"
    return "\n".join([f"scale_range: {lst(agg['scale_range'])}", f"vote_range: {lst(agg['vote_range'])}",
                      f"scale_mean: {agg['scale_mean']}"])


def category_stats(meshes, n_samples=2048, n_pairs=100000, seed=0, device=None, max_faces_per_call=MAX_FACES_PER_CALL):
    """gen_stats.py for one category.  meshes: OBJ paths (read with meshes.load_obj) or (vertices, faces) pairs.  Mesh m draws
    with the Philox counter of mesh index m, so the result does not depend on how the batch is split.  One host read at the end.
    Returns dict(rows f64[M,6] (STAT_COLUMNS), names, scale_range, vote_range, scale_mean).  A mesh with no surface area raises
    MeshStatsError naming it."""
    from .meshes import load_obj
    require_cuda()
    dev = _device(device)
    items = list(meshes)
    if not items:
        raise MeshStatsError("no meshes")
    names = [it if isinstance(it, (str, os.PathLike)) else f"<mesh {k}>" for k, it in enumerate(items)]
    loaded = [load_obj(it) if isinstance(it, (str, os.PathLike)) else it for it in items]
    rows, stat = [], []
    for idx in _chunks(loaded, max_faces_per_call):
        pts, _, st_s = sample_surface_batch([loaded[k] for k in idx], n_samples, seed, idx[0], dev)
        st_v = vote_stats_batch(pts, n_pairs, seed, idx[0])
        rows.append(st_v[0])
        stat.append(torch.stack([st_s, st_v[1]], -1))
    host = torch.cat([torch.cat(rows).flatten(), torch.cat(stat).flatten().double()]).cpu().numpy()   # the one host read
    M = len(items)
    rows, stat = host[:6 * M].reshape(M, 6), host[6 * M:].reshape(M, 2).astype(np.int64)
    for k in range(M):
        if stat[k, 0]:
            raise MeshStatsError(f"{names[k]}: {_status_text(int(stat[k, 0]))}")
        if stat[k, 1]:
            raise MeshStatsError(f"{names[k]}: a sampled point is not finite")
    out = aggregate(rows)
    out.update(rows=rows, names=[str(n) for n in names])
    return out


def derive_config(name, stats, res, scale_range, up_sym=False, right_sym=False, z_right=False, regress_right=False):
    """A CategoryConfig for meshes whose category_stats are `stats`, consistent with how MeshViewSampler uses it: the sampler
    multiplies the raw (centred) mesh by a scale drawn from `scale_range` (meshes.model_matrix) and takes the half extents with x
    and z swapped (meshes.view_half_extents, utils/dataset.py:244-247).  So

        vote_range = raw vote_range * scale_range[1]          (the largest object a view can show)
        scale_mean = raw half extents [z, y, x] * mean(scale_range)

    This derivation is this project's rule, not the reference's: the reference's category files were evidently written by hand
    from gen_stats.py's output and real-world sizes.  The raw gen_stats figures stay in `stats` unchanged."""
    lo, hi = float(scale_range[0]), float(scale_range[1])
    if not 0 < lo <= hi:
        raise ValueError(f"scale_range {scale_range}: need 0 < lo <= hi")
    vr = [float(v) * hi for v in stats["vote_range"]]
    h = np.asarray(stats["scale_mean"], np.float64)
    sm = [float(x) * (lo + hi) / 2 for x in (h[2], h[1], h[0])]
    return CategoryConfig(name, float(res), vr, sm, bool(regress_right), up_sym=bool(up_sym), z_right=bool(z_right),
                          scale_range=[lo, hi], right_sym=bool(right_sym))
