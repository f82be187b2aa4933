"""Device-resident counterpart of the per-instance hot section of the reference's inference script
(nocs/inference.py:177-335; the same lines are duplicated at sunrgbd/inference.py:136-241).

The reference bounces every stage through the host (torch -> numpy -> CuPy and back, :191-231,
:265-284).  Here the whole chain is enqueued on one HIP stream and the host reads back ONE small
record at the end:

  PPF + pair MLP + decode      PPFEncoder.forward_decode            (:182-188)
  second pass on survivors     PPFEncoder.forward_decode_sel        (:236-256)
  centre vote + arg-max        cppf_vote_argmax                     (:191-208)
  T = corner + cand * res      cppf_center_from_argmax              (:209-213)
  back-vote + compaction       cppf_backvote / cppf_compact_mask    (:216-231)
  orientation vote + count     cppf_rot_sphere_count, arg-max       (:259-284)
  axis sign                    cppf_axis_sign                       (:286-303)
  scale                        cppf_scale_sum                       (:335)

Stochastic pieces of the reference are made explicit inputs: `u_tr`/`u_rot` (uniforms replacing
torch.multinomial at :186/:250/:254, indexed by ORIGINAL pair; the second MLP pass of :236 runs on the
surviving pairs only, like the reference's, through cppf_pair_mlp_decode_sel), and the random
10 000-pair subset of :277-280 is the first `max_rot_pairs` survivors in pair order (pairs are
i.i.d. uniform, so a prefix is distributed exactly like a shuffled subset).
"""
import ctypes as C
import gc
import os

import numpy as np
import torch

from . import _lib, chains
from ._torch_util import call, canon, copy_words, fill, release_scope, require_cuda, scratch, workspace, workspace_scope
from .models import voting

F32, I32 = torch.float32, torch.int32


def _canon_inputs(pc, pc_normal, feat, point_idxs, u_tr, u_rot, probs=None):
    """The caller's tensors of estimate_center / estimate_pose in the form every launch of the chain reads ("Input
    forms"): f32 / index dtype, C-contiguous, on pc's device -- converted once, so the centre half and the tail see the same
    tensors; a tensor elsewhere (the CPU included) is refused by name before anything is launched.  A numpy pair list is uploaded
    as PPFEncoder takes it (nocs/inference.py:177,182)."""
    if not isinstance(pc, torch.Tensor) or not pc.is_cuda:
        raise ValueError(f"pc: expected a tensor on a HIP device, got {getattr(pc, 'device', type(pc).__name__)}")
    dev = pc.device
    pc = canon(pc, F32, dev, "pc", (3,))
    P = int(point_idxs.shape[0])
    if isinstance(point_idxs, np.ndarray):
        from .models.model import PPFEncoder
        point_idxs = PPFEncoder._as_index_tensor(point_idxs, dev)
    return (pc, canon(pc_normal, F32, dev, "pc_normal", (3,)), canon(feat, F32, dev, "feat"),
            canon(point_idxs, (torch.int64, I32), dev, "point_idxs", (2,)), canon(u_tr, F32, dev, "u_tr", (P, 2)),
            None if u_rot is None else canon(u_rot, F32, dev, "u_rot", (P, 2)),
            None if probs is None else canon(probs, F32, dev, "probs"))


def grid_shape(pc_host, res):
    """nocs/inference.py:194-195 on the host copy of the cloud: corners, int32((max-min)/res)+1 (cppf_host_grid_shape: one pass
    over the cloud in C; the numpy form below -- same types, same results -- serves anything that is not a C-contiguous f32[N,3])."""
    a = np.asarray(pc_host)
    if a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 and a.shape[0] > 0 and a.flags.c_contiguous:
        corners = np.empty((2, 3), np.float32)
        dims = np.empty(3, np.int32)
        rc = call("cppf_host_grid_shape", None, a, a.shape[0], float(np.float32(res)), corners, dims, ok=(_lib.ENONFINITE,))
        if rc == _lib.ENONFINITE:      # the reference fails at np.zeros(grid_res) with the dims such a cloud gives (:196)
            raise ValueError("the cloud holds NaN / inf coordinates: no vote grid can be laid over it")
        return corners, (int(dims[0]), int(dims[1]), int(dims[2]))
    t = np.ascontiguousarray(np.asarray(pc_host, dtype=np.float32).T)    # [3,N]: numpy reduces the long axis 20x faster than axis 0 of [N,3]
    corners = np.stack([t.min(1), t.max(1)])
    if not np.isfinite(corners).all():
        raise ValueError("the cloud holds NaN / inf coordinates: no vote grid can be laid over it")
    grid_res = ((corners[1] - corners[0]) / np.float32(res)).astype(np.int32) + 1
    return corners, tuple(int(v) for v in grid_res)


class PoseWorkspace:
    """Per-object device buffers, allocated once and reused across calls of the same size."""

    def __init__(self, device, n_pairs, dims, n_sphere, grid=None):
        self.device, self.n_pairs, self.dims, self.n_sphere = device, n_pairs, None if dims is None else tuple(dims), n_sphere
        self.grid = grid if grid is not None else torch.empty(self.dims, dtype=F32, device=device)
        self.out_idx = torch.empty(1, dtype=torch.int64, device=device)
        self.out_val = torch.empty(1, dtype=F32, device=device)
        # the 21-double result record; T64 / best_dir / sign / scale are views into it, so the kernels write the
        # record directly and the read-back is one copy
        # (the record and the sphere-bin counts share one buffer: both start every tail zeroed, with one fill)
        # layout: record 176 B | counts 2 x n_sphere i32 | ticket 16 B | survivors per chunk of 1024 pairs i32[...]; 16 B multiple
        c0 = 176 + ((2 * n_sphere * 4 + 15) & ~15)
        n_chunks = (n_pairs + 1023) // 1024
        self._tail0 = torch.zeros(c0 + 16 + ((4 * n_chunks + 15) & ~15), dtype=torch.uint8, device=device)
        self.ticket = self._tail0[c0:c0 + 16].view(I32)
        self.chunk_counts = self._tail0[c0 + 16:c0 + 16 + 4 * n_chunks].view(I32)
        self.rec = self._tail0[:168].view(torch.float64)
        self.T64 = self.rec[0:3]
        self.T32 = torch.empty(3, dtype=F32, device=device)
        self.mask = torch.empty(n_pairs, dtype=torch.uint8, device=device)
        self.surv = torch.empty(n_pairs, dtype=I32, device=device)
        self.count = torch.empty(1, dtype=I32, device=device)
        self.counts = self._tail0[176:176 + 2 * n_sphere * 4].view(I32).view(2, n_sphere)
        self.best_idx = torch.empty(2, dtype=torch.int64, device=device)
        self.best_dir = self.rec[3:9].view(2, 3)
        self.sign = self.rec[9:15].view(2, 3)
        self.scale = self.rec[15:19]
        # {theta_up, theta_right, aux_up, aux_right, sx, sy, sz, 0} per pair, written by the second MLP pass for the pairs
        # that survive the back-vote (nocs/inference.py:236-256); other rows keep whatever an earlier instance left
        self.heads = torch.zeros((n_pairs, 8), dtype=F32, device=device)
        self.probs = None
        self._sph_key = None

    def sphere(self, sph64):
        """Device copies of the sphere bins (fp32 for the count, fp64 for best_dir) and whether the bins
        are unit vectors with a monotone y column (true for fibonacci_sphere), which lets
        cppf_rot_sphere_count search a band of bins instead of all of them."""
        key = (sph64.shape, sph64.tobytes())
        if self._sph_key != key:
            s32 = sph64.astype(np.float32)
            unit = bool(np.all(np.abs(np.linalg.norm(s32.astype(np.float64), axis=-1) - 1.0) < 1e-4))
            dy = np.diff(s32[:, 1])
            self._sorted_y = (1 if np.all(dy <= 0) else (-1 if np.all(dy >= 0) else 0)) if unit else 0
            self._sph32 = torch.from_numpy(s32).to(self.device)
            self._sph64 = torch.from_numpy(sph64).to(self.device)
            self._sph_key = key
        return self._sph32, self._sph64, self._sorted_y


def estimate_center(encoder, pc, pc_normal, feat, point_idxs, u_tr, cfg, corner, dims, num_rots=72, adaptive=True,
                    u_rot=None, ws=None, idx32=None, probs=None):
    """PPF -> MLP -> decode -> centre vote -> arg-max, all on device (the benchmarked chain).
    Returns (out_idx i64[1], out_val f32[1], outputs f32[P,2], heads f32[P,8] | None, grid)."""
    require_cuda()
    pc, pc_normal, feat, point_idxs, u_tr, u_rot, probs = _canon_inputs(pc, pc_normal, feat, point_idxs, u_tr, u_rot, probs)
    dev = pc.device
    corner = canon(corner, F32, dev, "corner")
    P = point_idxs.shape[0]
    if ws is None:
        ws = PoseWorkspace(dev, P, dims, 1)
    if idx32 is None:
        idx32 = point_idxs.to(I32)
    else:
        idx32 = canon(idx32, (I32,), dev, "idx32", (2,))
    # probs=None: all ones (nocs/inference.py:201) -- the vote then reads no probs at all
    outputs, heads = encoder.forward_decode(pc, pc_normal, feat, point_idxs, u_tr, cfg.vote_range, u_rot,
                                            cfg.tr_num_bins, cfg.rot_num_bins)
    # grid = votes (overwrite mode replaces the zero-initialisation of :196)
    voting.vote_argmax(pc, outputs, probs, idx32, ws.grid, corner, cfg.res, num_rots, adaptive, ws.out_idx,
                       ws.out_val, accumulate=False)
    return ws.out_idx, ws.out_val, outputs, heads, ws.grid


_grid_class_cache = {}


def grid_class(dims):
    """(tiles, tile capacity class, cell capacity) of the shape-polymorphic vote for a grid of `dims`: launches come in three
    classes -- 0: < 4 LDS tiles (the fused vote, <= 3 tiles of cells), 16: up to 16 tiles (bin + vote with queues for 16 tiles: posed
    NOCS objects need 9-12, the C5 grid 16), 1: up to 64 (queues for 64) -- the value is what the *_dyn entry points take as
    `many_tiles` (truthy = a binned class); tiles == 0: the grid needs more than the tiled vote serves -- only the exact-shape
    pipeline runs it."""
    key = (int(dims[0]), int(dims[1]), int(dims[2]))
    hit = _grid_class_cache.get(key)
    if hit is None:
        L = _lib.lib()
        T = int(L.cppf_vote_tiles(*key))
        many = 0 if T < 4 else (16 if T <= 16 and not os.environ.get("CPPF_TILE_CLASS_64") else 1)
        hit = (T, many, _lib.tiles_cap(many) * int(L.cppf_vote_tile_cells()))
        if len(_grid_class_cache) < 4096:
            _grid_class_cache[key] = hit
    return hit


class _GraphCache:
    """The captured hipGraphs of one pipeline or chain and the one way they are captured and replayed.  One entry per FORM (None for
    the classes with one form, `full_first` False / True for PosePipeline and PoseChain) = (graph, the key it was captured under,
    the tensors its launches write): a captured form owns its outputs / heads / feat, so whoever switches the form gets the other
    form's tensors back from run()."""

    def __init__(self, owner, use_graph):
        # scratch requested by a chain belongs to its owner (see workspace_scope): pipelines replay concurrently
        self.scope, self.device, self.use_graph, self.entries = id(owner), owner.device, use_graph, {}

    def graph(self, form=None):
        entry = self.entries.get(form)
        return entry[0] if entry is not None else None

    def clear(self):
        self.entries = {}

    def _images(self, members, check_weights, entry):
        """the weight-image part of the key.  check_weights=True (or nothing captured yet): a changed parameter is re-packed here, on
        this stream, into the buffer the captured launches read, and the images' addresses are returned; None: the caller refreshed
        the images itself (BatchPoseRunner, once per batch), only their addresses are looked at; False: nothing is (a caller that
        runs many instances between parameter updates)"""
        if check_weights or entry is None:
            return tuple(p._weight_images() for p in members)
        return tuple(p._image_ptrs() for p in members) if check_weights is None else entry[1][0]

    def run(self, chain_fn, members, check_weights=True, extra=None, form=None, eager=False):
        """Run `chain_fn` (the launches of `members`, CenterPipelines; returns the tensors it wrote) as the replay of its captured
        graph -> those tensors.  The graph is captured on first use and again when its key = (weight images, `extra`: whatever else
        the launches bake in) changed: a moved / resized image, another vote width, other member buffers.  eager (or use_graph
        False): launch instead.  Either way the run is ordered after a weight image rebuilt in place on another stream, and a later
        rebuild after it."""
        with torch.no_grad(), workspace_scope(self.scope):
            entry = None
            if self.use_graph and not eager:
                entry = self.entries.get(form)
                # the pair and point encoders' precision is part of the key whatever `check_weights` says (another kernel, another image): after
                # a switch the entry is dropped before the images are looked at, so the new key holds the new precision's addresses
                precision = tuple((p.encoder.precision, None if p.point_encoder is None else p.point_encoder.precision)
                                  for p in members)
                if entry is not None and entry[1][2] != precision:
                    self.entries.pop(form, None)
                    entry = None
                key = (self._images(members, check_weights, entry), extra, precision)
                if entry is None or entry[1] != key:
                    self.entries.pop(form, None)
                    entry = None                          # (a stale graph's memory goes before the new one's is taken)
                    # warm up on a side stream (lazy attribute setting, weight packing, scratch allocation), then capture; the
                    # captured launches read the static buffers, so later loads just change the data
                    cur = torch.cuda.current_stream(self.device)
                    s = torch.cuda.Stream(device=self.device)
                    s.wait_stream(cur)
                    with torch.cuda.stream(s):
                        chain_fn()
                        chain_fn()
                    cur.wait_stream(s)
                    graph = torch.cuda.CUDAGraph()
                    # No cycle collection inside the capture: chain_fn allocates enough Python objects to trigger one, and a dead
                    # pipeline or chain that sits in a reference cycle (a runner kept alive by an exception's traceback, say) would
                    # have its __del__ run right here -- release() drops ITS captured graphs, and destroying a graph while this
                    # thread captures aborts the process.  (torch.cuda.graph no longer collects on entry.)  Such garbage goes at
                    # the first collection after the capture instead.
                    gc_was_on = gc.isenabled()
                    gc.disable()
                    try:
                        # thread_local: other threads (the RCCL watchdog of a multi-rank run) may touch the runtime meanwhile
                        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                            tensors = chain_fn()
                    finally:
                        if gc_was_on:
                            gc.enable()
                    entry = self.entries[form] = (graph, key, tensors)
            for p in members:
                p._await_images()
            if entry is None:
                tensors = chain_fn()
            else:
                entry[0].replay()
                tensors = entry[2]
            for p in members:
                p._note_images_read()
        return tensors


class _Captured:
    """what the pipelines and chains share: a _GraphCache in `_cache`, the form the next run uses, and the way out"""

    full_first = None       # None: the class has one captured form

    @property
    def _graph(self):
        """the graph the next replay (of the current form) uses, None before its capture"""
        return self._cache.graph(self.full_first)

    def release(self):
        """drop the captured graphs and this object's scratch buffers (BatchPoseRunner's cache eviction)"""
        self._cache.clear()
        release_scope(id(self))      # scratch is keyed by id(self): it must not outlive the object

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _point_features(p):
    """the per-point features of member `p` (nocs/inference.py:180-181, no N x N matrix): its point encoder's launches, or the
    features it was loaded with"""
    if p.point_encoder is None:
        return p.feat
    if p.dynamic:
        return p.point_encoder.forward_dyn(p.pc, p.nrm, p.shape, out=p._feat_out, nbrs=p._nbrs, nbrs_ready=p.nbrs_ready)
    return p.point_encoder(p.pc[None], p.nrm[None])[0]


def _decode_items(pipes, feats, with_heads):
    """the members as models.model.forward_decode_batch takes them"""
    return [dict(encoder=p.encoder, pc=p.pc, pc_normal=p.nrm, feat=f, idxs=p.idx, u_tr=p.u_tr, vote_range=p.cfg.vote_range,
                 **(dict(u_rot=p.u_rot) if with_heads else {})) for p, f in zip(pipes, feats)]


def _vote_items(pipes, outputs):
    """the members as models.voting.vote_argmax_batch takes them"""
    return [dict(points=p.pc, outputs=o, point_idxs=p.idx, corner=p.corner, res=p.cfg.res, out_idx=p.out_idx, out_val=p.out_val,
                 **(dict(grid=p.grid_flat, shape=p.shape, many_tiles=p.many_tiles) if p.dynamic else dict(grid=p.grid)))
            for p, o in zip(pipes, outputs)]


class CenterPipeline(_Captured):
    """The centre chain (PPF -> MLP -> decode -> vote -> arg-max) for a fixed problem shape, with static
    device buffers and -- by default -- the three kernel launches captured once in a hipGraph, so that a
    replay costs one launch on the host instead of ~0.25 ms of Python per object.

        pipe = CenterPipeline(encoder, cfg, n_points, n_pairs, dims, device)
        pipe.load(pc, normals, feat, point_idxs, u_tr, u_rot, corner)     # host or device arrays
        idx, val = pipe.run()                                             # device i64[1], f32[1]

    `outputs` (mu, nu), `heads` and `grid` of the last run stay available as attributes.  With
    `point_encoder=` (a cppf_amd PointEncoder) the per-point features are computed on device at the head of the
    chain (kNN + SPRIN, nocs/inference.py:180-181) and `load(feat=None)` is enough.

    dynamic=True makes the pipeline SHAPE-POLYMORPHIC: `n_points` is then a capacity and `dims` either a capacity
    class (`many_tiles` bool) or any grid of that class; every instance with N <= n_points points (N >= k of the point
    encoder) and a grid of that class runs on the same captured graph -- its real shape {N, gx, gy, gz} travels in the
    device record `shape` (written by load()) and the *_dyn kernels read it.  Real scenes give every instance its own N
    (voxel de-duplication, nocs/inference.py:140-142) and its own grid (:194-195); the number of pairs is the caller's
    constant (:177).  Results equal the exact-shape pipeline's bit for bit.

    The encoders' weight images are re-checked before every run: a parameter update (optimizer step, load_state_dict)
    is re-packed into the same device buffer, which the captured launches read; a moved / resized image re-captures."""

    def __init__(self, encoder, cfg, n_points, n_pairs, dims, device, num_rots=72, adaptive=True, with_heads=True,
                 use_graph=True, point_encoder=None, dynamic=False, vote_workgroups=0, idx_i32=False):
        """vote_workgroups: 0 = the vote launches one workgroup per CU (fastest for ONE instance on an idle chip); 64..256 = at
        most that many (cppf.h: CPPF_VOTE_WORKGROUPS) -- for callers that keep several pipelines in flight on different streams,
        where fewer, longer-lived vote workgroups leave the rest of the chip to the other streams (bench.py, BatchPoseRunner).
        idx_i32: the pipeline's pair list is int32[P,2] instead of the reference's int64 (nocs/inference.py:177) -- for lists that are
        drawn on the device (a staged chain: cppf_stage_batch) every kernel that streams the list moves half the index bytes, and
        the tail needs no int32 copy; a host list loaded into it is narrowed (indices are < n_points)."""
        require_cuda()
        self.vote_workgroups = int(vote_workgroups or 0)
        self.encoder, self.cfg, self.device = encoder, cfg, device
        self.point_encoder = point_encoder
        self.num_rots, self.adaptive, self.with_heads = num_rots, adaptive, with_heads
        self.n_points, self.n_pairs, self.dynamic = int(n_points), int(n_pairs), bool(dynamic)
        F = (encoder.ppffcs[0] - 4) // 2
        z = lambda *shape, dtype=F32: torch.zeros(shape, dtype=dtype, device=device)
        # the small per-instance inputs live in ONE buffer -- points | normals | corner | shape record -- so that a caller can
        # stage and upload them with a single copy (BatchPoseRunner); pc / nrm / corner / shape are views into it
        n = self.n_points
        self._in = z(6 * n + 8)
        self.pc, self.nrm = self._in[:3 * n].view(n, 3), self._in[3 * n:6 * n].view(n, 3)
        self.feat = z(n_points, F)
        self.idx = z(n_pairs, 2, dtype=I32 if idx_i32 else torch.int64)
        self.idx32 = self.idx if idx_i32 else z(n_pairs, 2, dtype=I32)
        self._u = z(2, n_pairs, 2)                     # one buffer: device-side sampling fills both with one launch
        self.u_tr, self.u_rot = self._u[0], self._u[1]
        self.corner = self._in[6 * n:6 * n + 3]
        self.probs = None       # all ones (nocs/inference.py:201): the vote takes None for that and reads nothing
        if self.dynamic:
            if isinstance(dims, (bool, np.bool_, int, np.integer)):       # a capacity class (_lib.tile_class)
                self.many_tiles = _lib.tile_class(bool(dims) if isinstance(dims, (bool, np.bool_)) else int(dims))
            else:
                T, self.many_tiles, _ = grid_class(dims)
                if T == 0:
                    raise _lib.CppfError(f"grid {tuple(dims)} needs more LDS tiles than the shape-polymorphic vote serves")
            self.grid_flat = z(_lib.tiles_cap(self.many_tiles) * int(_lib.lib().cppf_vote_tile_cells()))
            self.shape = self._in[6 * n + 4:6 * n + 8].view(I32)               # {n_points, gx, gy, gz}, read by the *_dyn kernels
            self.shape_host = (0, 0, 0, 0)
            self.dims = None
            if point_encoder is not None:
                self._nbrs = z(n_points, point_encoder.k, dtype=I32)
                self._feat_out = z(n_points, point_encoder.out_dim + point_encoder.out_dim // 4)
        else:
            self.dims = tuple(int(v) for v in dims)
            self.grid = torch.empty(self.dims, dtype=F32, device=device)
        # arg-max index and value side by side in one 16-byte record, so a caller that logs every step moves them with
        # one small copy: `result` u8[16] = {i64 flat index, f32 peak, 4 bytes unused}
        self.result = torch.zeros(16, dtype=torch.uint8, device=device)
        self.out_idx = self.result[:8].view(torch.int64)
        self.out_val = self.result[8:12].view(F32)
        self.outputs = self.heads = None
        self.nbrs_ready = False      # dynamic + point encoder: `_nbrs` already holds the cloud's neighbour sets (frames.FrameRunner)
        self._image_gens = {}        # the weight-image rebuilds this pipeline has waited for (_await_images)
        self._cache = _GraphCache(self, use_graph)

    def set_shape(self, n_points, dims, shape_src=None, upload=True):
        """dynamic pipelines: the next run's real shape.  `shape_src`: a (pinned) host i32[4] tensor the caller has filled
        with {n_points, gx, gy, gz} -- copied asynchronously; without it a small synchronous upload is made;
        upload=False: the caller writes the record itself (it is part of the `_in` buffer)."""
        if not self.dynamic:
            raise _lib.CppfError("set_shape() is for dynamic pipelines")
        T, many, cap = grid_class(dims)
        k_min = self.point_encoder.k if self.point_encoder is not None else 1
        if not (k_min <= n_points <= self.n_points) or T == 0 or T > _lib.tiles_cap(self.many_tiles) or \
                int(dims[0]) * int(dims[1]) * int(dims[2]) > self.grid_flat.numel():
            raise _lib.CppfError(f"instance shape N={n_points}, grid {tuple(dims)} does not fit this pipeline "
                                 f"(N in {k_min}..{self.n_points}, many_tiles={self.many_tiles})")
        self.shape_host = (int(n_points), int(dims[0]), int(dims[1]), int(dims[2]))
        self.dims = self.shape_host[1:]
        if not upload:
            return
        if shape_src is None:
            shape_src = torch.tensor(self.shape_host, dtype=I32)
        self.shape.copy_(shape_src, non_blocking=True)

    @property
    def grid_view(self):
        """the vote grid of the last run as f32[gx,gy,gz]"""
        if not self.dynamic:
            return self.grid
        gx, gy, gz = self.dims
        return self.grid_flat[:gx * gy * gz].view(gx, gy, gz)

    def load(self, pc, pc_normal, feat, point_idxs, u_tr, u_rot, corner, dims=None):
        """host or device arrays -> the static buffers (None = keep).  Dynamic pipelines take clouds of any N <= capacity
        and need `dims` (grid_shape(pc, res)[1]) together with `pc`."""
        n = None if pc is None else int(pc.shape[0])
        if self.dynamic and pc is not None:
            if dims is None:
                raise ValueError("a dynamic pipeline needs dims with every cloud")
            self.set_shape(n, dims)
        for dst, src, per_point in ((self.pc, pc, True), (self.nrm, pc_normal, True), (self.feat, feat, True),
                                    (self.idx, point_idxs, False), (self.u_tr, u_tr, False), (self.u_rot, u_rot, False),
                                    (self.corner, corner, False)):
            if src is None:
                continue
            src = torch.as_tensor(src)
            if self.dynamic and per_point:
                dst = dst[:src.shape[0]]
            dst.copy_(src, non_blocking=True)

    def _chain(self):
        """enqueue the launches -> (outputs, heads, feat), the tensors they write"""
        feat = _point_features(self)
        outputs, heads = self.encoder.forward_decode(
            self.pc, self.nrm, feat, self.idx, self.u_tr, self.cfg.vote_range,
            self.u_rot if self.with_heads else None, self.cfg.tr_num_bins, self.cfg.rot_num_bins)
        # the vote reads the int64 pair list directly (the reference copies it to int32 first, nocs/inference.py:202)
        if self.dynamic:
            voting.vote_argmax_dyn(self.pc, outputs, None, self.idx, self.grid_flat, self.shape, self.corner,
                                   self.cfg.res, self.num_rots, self.adaptive, self.out_idx, self.out_val,
                                   many_tiles=self.many_tiles, accumulate=False, workgroups=self.vote_workgroups)
        else:
            voting.vote_argmax(self.pc, outputs, None, self.idx, self.grid, self.corner, self.cfg.res,
                               self.num_rots, self.adaptive, self.out_idx, self.out_val, accumulate=False,
                               workgroups=self.vote_workgroups)
        return outputs, heads, feat

    def _weight_images(self):
        """(re)build the encoders' weight images if a parameter changed; returns their identity (addresses)"""
        ids = [self.encoder._packed_weights(self.device).data_ptr()]
        if self.point_encoder is not None:
            ids.append(self.point_encoder._packed_weights(self.device)[0].data_ptr())
        return tuple(ids)

    def _image_ptrs(self):
        """the addresses of the weight images as they are NOW, without looking at the parameters (a caller that has just refreshed
        the images of its encoders -- BatchPoseRunner, once per batch -- only needs to know whether an image MOVED since capture)"""
        enc, penc = self.encoder, self.point_encoder
        image = enc._current_image()               # (of the encoder's current precision: each keeps its own buffer)
        pimage = None if penc is None else penc._current_image()
        if image is None or (penc is not None and pimage is None):
            return self._weight_images()
        return (image.data_ptr(),) if penc is None else (image.data_ptr(), pimage[0].data_ptr())

    def run(self, check_weights=True):
        """check_weights: how far the encoders' weight images are looked at before the run (_GraphCache._images)"""
        self.outputs, self.heads, self.feat = self._cache.run(self._chain, (self,), check_weights, None, self.full_first)
        return self.out_idx, self.out_val

    def _await_images(self):
        """another stream may have rebuilt a weight image in place since this pipeline last replayed: wait for it"""
        seen = self._image_gens                                # per (encoder, stream): a pipeline replayed on a NEW stream must wait too
        sid = torch.cuda.current_stream(self.device).cuda_stream
        for enc in (self.encoder, self.point_encoder):
            if enc is not None:
                seen[(id(enc), sid)] = enc._await_image(self.device, seen.get((id(enc), sid)))

    def _note_images_read(self):
        """... and a later rebuild (on any stream) must wait for this replay"""
        for enc in (self.encoder, self.point_encoder):
            if enc is not None:
                enc._note_image_read(self.device)

    def set_vote_workgroups(self, n):
        """change the vote's launch width (see __init__); the chain is captured again on the next run"""
        n = int(n or 0)
        if n != self.vote_workgroups:
            self.vote_workgroups = n
            self._cache.clear()


def estimate_pose(encoder, pc, pc_normal, feat, point_idxs, u_tr, u_rot, cfg, sphere_pts, pc_host=None, num_rots=72,
                  adaptive=True, angle_tol=1.5, max_rot_pairs=10000, ws=None, rng=None, rot_order=None):
    """Full per-instance pose (nocs/inference.py:177-339 minus dataset I/O and the laptop segmenter).

    encoder: cppf_amd.models.model.PPFEncoder on `pc.device`, eval mode.
    pc, pc_normal f32[N,3], feat f32[N,F], point_idxs i64/i32[P,2], u_tr/u_rot f32[P,2]: device tensors.
    sphere_pts: fp64 array [S,3] (np.array(fibonacci_sphere(S)), :100-102).
    rot_order: optional i32 array / device tensor of positions in the survivor list -- the reference's shuffled subsample for
    the orientation vote (:277-280: `np.random.shuffle(arange(P'))[:10000]`); entries beyond the survivor count are skipped,
    so a caller that does not know P' yet may pass a longer list.  None: the first `max_rot_pairs` survivors.
    Returns a dict of host values: T f64[3], up/right f64[3], R f64[3,3], scale f64[3], scale_norm,
    argmax (flat grid index), peak, n_surv, counts_up/right (i32[S])."""
    require_cuda()
    # once, at the top: the centre half, the second pass and the tail below all read these tensors
    pc, pc_normal, feat, point_idxs, u_tr, u_rot, _ = _canon_inputs(pc, pc_normal, feat, point_idxs, u_tr, u_rot)
    dev = pc.device
    P = point_idxs.shape[0]
    if pc_host is None:
        pc_host = pc.detach().cpu().numpy()
    corners, dims = grid_shape(pc_host, cfg.res)                              # :194-195
    corner = torch.from_numpy(corners[0].copy()).to(dev)
    sph64 = np.asarray(sphere_pts, dtype=np.float64)
    S = sph64.shape[0]
    if ws is None or ws.n_pairs != P or ws.dims != dims or ws.n_sphere != S or ws.device != dev:
        ws = PoseWorkspace(dev, P, dims, S)
    sph32_d, sph64_d, sorted_y = ws.sphere(sph64)                             # :276 (uploaded once per workspace)
    idx32 = point_idxs.to(I32)
    if rot_order is not None:
        rot_order = torch.as_tensor(rot_order).to(device=dev, dtype=I32).contiguous()

    # centre ------------------------------------------------------------------------------------------
    split = encoder.fused_decode_supported(cfg.tr_num_bins, cfg.rot_num_bins)
    _, _, outputs, heads, _ = estimate_center(encoder, pc, pc_normal, feat, point_idxs, u_tr, cfg, corner, dims,
                                              num_rots, adaptive, None if split else u_rot, ws, idx32)
    if split:       # the reference's own order: a second pass for the survivors (:236-256)
        heads = ws.heads
    # (other bin counts / architectures: every head of every pair came from the first pass, through the logits + decode kernels)
    _enqueue_tail(ws, pc, pc_normal, idx32, outputs, heads, corner, cfg, dims, num_rots, angle_tol, max_rot_pairs,
                  sph32_d, sph64_d, sorted_y, second_pass=(encoder, feat, point_idxs, u_rot) if split else None,
                  rot_order=rot_order)
    out = _assemble(ws.rec.cpu().numpy(), cfg, rng)                           # the one read-back
    out.update(dims=dims, corner=corners[0], ws=ws, outputs=outputs, heads=heads)
    return out


def _enqueue_tail(ws, pc, pc_normal, idx32, outputs, heads, corner, cfg, dims, num_rots, angle_tol, max_rot_pairs,
                  sph32_d, sph64_d, sorted_y, shape=None, second_pass=None, idx64=None, rot_order=None):
    """nocs/inference.py:209-303,335 after the centre vote, all on the current stream; leaves the 21-double
    result record in ws.rec (T[3], best_dir[2,3], sign sums[2,3], scale sums[4], argmax, peak).  `shape`: the device
    dims record of a shape-polymorphic pipeline (then `dims` is unused).  `second_pass` = (encoder, feat, point_idxs, u_rot):
    the heads of the surviving pairs are computed here, after the compaction, like the reference's second
    ppf_encoder call (:236-256); without it `heads` must already hold them.  `idx64`: the pair list as int64 -- then `idx32`
    is an OUTPUT, filled by the back-vote launch for the launches after it (no conversion pass).  `rot_order`: device i32[m],
    positions in the survivor list whose pairs feed the orientation vote (the reference's shuffled subsample, :277-280);
    None = the first `max_rot_pairs` survivors."""
    dev = pc.device
    L = _lib.lib()
    P, S = idx32.shape[0], sph32_d.shape[0]
    # the vote's workspace (same scope, same tag as models/voting.py): its rotation table is reused by the back-vote
    vws = workspace(256, dev, "vote_dyn" if shape is not None else "vote")
    vws = vws if vws.numel() >= 32768 else None
    gx, gy, gz = (1, 1, 1) if shape is not None else dims
    # T = corner + unravel(argmax) * res (:209-210); the same launch zeroes the record, the bin counts, the chunk counts
    # and the ticket of the launches below
    call("cppf_pose_tail_begin", dev, ws.out_idx, corner, float(cfg.res), gy, gz, shape, ws.T64, ws.T32, ws.out_val, ws.rec[19:21],
         scratch(ws._tail0))
    # back-vote filter (:216-231) --------------------------------------------------------------
    # mask only: the offsets themselves (:220-228) are consumed nowhere else, so no buffer is zeroed or written
    tol = float(np.float32(3 * cfg.res))
    fused = 0 < P <= 8192 * 1024
    if idx64 is not None and not fused:
        idx32.copy_(idx64)
    if fused:                    # survivors counted per chunk by the back-vote itself: the compaction is one launch
        if idx64 is not None:
            call("cppf_backvote_count64", dev, pc, outputs, idx64, idx32, corner, float(cfg.res), P, num_rots, gx, gy, gz, shape, ws.T32,
                 tol, ws.mask, ws.chunk_counts, vws)
        else:
            call("cppf_backvote_count", dev, pc, outputs, idx32, corner, float(cfg.res), P, num_rots, gx, gy, gz, shape, ws.T32, tol,
                 ws.mask, ws.chunk_counts, vws)
        call("cppf_compact_scatter", dev, ws.mask, P, ws.chunk_counts, ws.surv, ws.count)
    else:
        call("cppf_backvote_ws", dev, pc, outputs, None, idx32, corner, float(cfg.res), P, num_rots, gx, gy, gz, shape, ws.T32, tol,
             ws.mask, vws)
        cws = workspace(L.cppf_compact_workspace_bytes(P), dev, "compact")
        call("cppf_compact_mask", dev, ws.mask, P, ws.surv, ws.count, scratch(cws))
    if second_pass is not None:                                          # :236-256, survivors only
        enc2, feat2, idxs2, u_rot2 = second_pass
        enc2.forward_decode_sel(pc, pc_normal, feat2, idxs2, u_rot2, ws.surv, ws.count, heads, max_sel=P,
                                tr_num_bins=cfg.tr_num_bins, rot_num_bins=cfg.rot_num_bins)
    # orientation (:259-303) and scale (:335) ---------------------------------------------------
    # heads row = {theta_up, theta_right, aux_up, aux_right, sx, sy, sz, 0}: both directions' candidates are counted in
    # one launch; np.argmax(counts), sphere_pts[...] (:283-284), the sign sums (:287-301) and the scale sums in another
    thr = float(np.float32(np.cos(angle_tol / 180 * np.pi)))
    n_dirs = 2 if cfg.regress_right else 1
    if rot_order is None:
        call("cppf_rot_sphere_count_dirs", dev, pc, heads, 8, 1, n_dirs, idx32, ws.surv, ws.count, P, max_rot_pairs, num_rots, sph32_d, S,
             thr, sorted_y, ws.counts, S)
    else:
        call("cppf_rot_sphere_count_dirs_order", dev, pc, heads, 8, 1, n_dirs, idx32, ws.surv, ws.count, P, rot_order, rot_order.numel(),
             max_rot_pairs, num_rots, sph32_d, S, thr, sorted_y, ws.counts, S)
    pws = workspace(L.cppf_pose_sums_workspace_bytes(), dev, "pose_sums")
    call("cppf_pose_sums", dev, pc, pc_normal, idx32, ws.surv, ws.count, P, heads.data_ptr() + 4 * 2, 8, n_dirs, ws.counts, S, S, sph64_d,
         heads.data_ptr() + 4 * 4, 8, ws.best_idx, ws.best_dir, ws.sign, ws.scale, scratch(pws), ws.ticket)
    # (T64, best_dir, sign, scale, arg-max index and value were written into ws.rec by the kernels above)


def _assemble(rec, cfg, rng=None):
    """Host end of nocs/inference.py:299-339 from the 21-double record."""
    T = rec[0:3].copy()
    best = rec[3:9].reshape(2, 3)
    sign = rec[9:15].reshape(2, 3)
    ssum = rec[15:19]
    flat, peak = int(rec[19]), float(rec[20])
    if flat < 0:    # cppf_vote_argmax_dyn: the instance's shape record exceeded the captured launch's capacities
        raise _lib.CppfError("the instance shape did not fit the shape-polymorphic pipeline it ran on (arg-max index -1)")
    n_surv = int(ssum[3])
    n_dirs = 2 if cfg.regress_right else 1

    dirs = []
    for j in range(n_dirs):
        n = max(sign[j, 2], 1.0)
        up_loss, down_loss = sign[j, 0] / n, sign[j, 1] / n
        dirs.append(-best[j] if down_loss < up_loss else best[j].copy())      # :299-302
    up = dirs[0]
    if cfg.regress_right:                                                     # :305-312
        right = dirs[1]
        right = right - np.dot(up, right) * up
        right = right / (np.linalg.norm(right) + 1e-9)
    else:
        right = np.array([0, -up[2], up[1]])
        right = right / (np.linalg.norm(right) + 1e-9)
    if np.linalg.norm(right) < 1e-7:                                          # :325-328
        rng = rng or np.random.default_rng(0)
        right = rng.standard_normal(3)
        right -= right.dot(up) * up
        right /= np.linalg.norm(right)
    if cfg.z_right:                                                           # :330-333
        R = np.stack([np.cross(up, right), up, right], -1)
    else:
        R = np.stack([right, up, np.cross(right, up)], -1)
    mean = (ssum[:3] / max(n_surv, 1)).astype(np.float32)                     # torch mean is fp32
    pred_scale = np.exp(mean).astype(np.float64) * np.asarray(cfg.scale_mean, np.float64) * 2   # :335
    scale_norm = float(np.linalg.norm(pred_scale))
    return dict(T=T, up=up, right=right, R=R, scale=pred_scale, scale_norm=scale_norm, argmax=flat, peak=peak,
                n_surv=n_surv, best_up=best[0].copy(), best_right=best[1].copy() if n_dirs > 1 else None,
                losses=sign.copy())


def nocs_result(poses, res=None):
    """The per-image result record of nocs/inference.py:114-117,213,338-342 from a list of pose dicts (estimate_pose /
    PosePipeline.run / _assemble; a mask-free pose of scene_poses or its `refined` dict, scene_poses.refine_poses: T, R, scale and
    scale_norm are what is read): `pred_RTs` f32[n,4,4] (identity-initialised, translation in the last column, rotation
    scaled by |scale|) and `pred_scales` f32[n,3] (scale / |scale|), written into `res` (the detection dict the script
    pickles, :344-345) or a new dict -- the format nocs/eval.py reads."""
    n = len(poses)
    RTs = np.zeros((n, 4, 4), dtype=np.float32)
    for i in range(n):
        RTs[i] = np.eye(4)
    scales = np.ones((n, 3), dtype=np.float32)
    for i, p in enumerate(poses):
        if p is None:                                   # skipped instance (:121-123): identity pose, unit scale
            continue
        RTs[i][:3, -1] = p["T"]
        assert p["scale_norm"] > 0
        RTs[i][:3, :3] = p["R"] * p["scale_norm"]
        scales[i, :] = p["scale"] / p["scale_norm"]
    res = {} if res is None else res
    res["pred_RTs"] = RTs
    res["pred_scales"] = scales
    return res


class CenterBatchPipeline(_Captured):
    """Several CenterPipelines replayed as ONE captured chain: the pair lists of all members in one launch of the pair kernel
    (models.model.forward_decode_batch: the ~9 us a launch spends before its first MFMA are paid once, 70.9 -> 64.0 us per C2
    list in threes), then the members' votes -- by default in ONE vote launch and ONE reduce launch as well
    (models.voting.vote_argmax_batch: every object on 256 / n workgroups, a quarter of the partial-tile traffic per object in
    fours), `vote_batch=False`: a vote + reduce launch per member at the member's own width.  Members keep their buffers and results
    (`pipes[i].out_idx`, `.result`, `.outputs`, `.grid`): load them as usual, run the batch instead of the members.  Static-shape
    members on one device, no point encoder in front, all with the rotation heads or none, the same num_rots / adaptive; up to 8.
    vote_workgroups: workgroups per object of the batched vote (None / 0: 256 / n, at least 64; 64..256)."""

    def __init__(self, pipes, use_graph=True, vote_batch=True, vote_workgroups=None, own_results=True):
        """own_results=False: the members keep the result records they have (a pipeline that is a member of a second, shorter
        chain -- bench.py's remainder chains -- keeps the views the first chain gave it; `results` is then None)"""
        pipes = list(pipes)
        if not 1 <= len(pipes) <= 8:
            raise ValueError("1 to 8 pipelines per batch")
        if any(p.dynamic or p.point_encoder is not None or p.device != pipes[0].device or p.with_heads != pipes[0].with_heads
               or p.num_rots != pipes[0].num_rots or p.adaptive != pipes[0].adaptive for p in pipes):
            raise _lib.CppfError("CenterBatchPipeline takes static-shape CenterPipelines on one device, without a point encoder, "
                                 "with the same num_rots / adaptive")
        self.pipes, self.device = pipes, pipes[0].device
        self.vote_batch, self.vote_workgroups = bool(vote_batch), int(vote_workgroups or 0)
        self._cache = _GraphCache(self, use_graph)
        # the members' 16-byte result records side by side in ONE block (`results` u8[n,16]): a caller that logs every step moves
        # a chain's results with one small copy; the members' `result` / `out_idx` / `out_val` become views into it (their own
        # captured graphs, which wrote the old records, are dropped)
        self.results = torch.zeros((len(pipes), 16), dtype=torch.uint8, device=self.device) if own_results else None
        for i, p in enumerate(pipes if own_results else []):
            p.result = self.results[i]
            p.out_idx, p.out_val = p.result[:8].view(torch.int64), p.result[8:12].view(F32)
            p._cache.clear()
            if hasattr(p, "ws"):
                p.ws.out_idx, p.ws.out_val = p.out_idx, p.out_val

    def _capture_key(self):
        """what the captured launches bake in besides the weight images: the vote widths and the members' buffers"""
        return (self.vote_batch, self.vote_workgroups) + tuple((p.vote_workgroups, p.idx.data_ptr(), p.grid.data_ptr(), p.result.data_ptr())
                                                               for p in self.pipes)

    def _chain(self):
        """enqueue the launches -> [(outputs, heads)] of the members, the tensors they write"""
        from .models.model import forward_decode_batch
        pipes, p0 = self.pipes, self.pipes[0]
        outs = forward_decode_batch(_decode_items(pipes, [p.feat for p in pipes], p0.with_heads), p0.cfg.tr_num_bins, p0.cfg.rot_num_bins)
        if self.vote_batch:
            voting.vote_argmax_batch(_vote_items(pipes, [o for o, _ in outs]), p0.num_rots, p0.adaptive, accumulate=False,
                                     workgroups=self.vote_workgroups)
        else:
            for p, (o, _) in zip(pipes, outs):
                voting.vote_argmax(p.pc, o, None, p.idx, p.grid, p.corner, p.cfg.res, p.num_rots, p.adaptive, p.out_idx, p.out_val,
                                   accumulate=False, workgroups=p.vote_workgroups)
        return outs

    def run(self, check_weights=True):
        """-> [(out_idx, out_val)] of the members (device tensors, as CenterPipeline.run returns them).  The vote widths / member
        buffers the launches baked in are compared on every run (cheap), the weight images as `check_weights` says: a moved image,
        a member's set_vote_workgroups() or an assigned `vote_workgroups` captures again."""
        for p, (o, h) in zip(self.pipes, self._cache.run(self._chain, self.pipes, check_weights, self._capture_key())):
            p.outputs, p.heads = o, h
        return [(p.out_idx, p.out_val) for p in self.pipes]


class PosePipeline(CenterPipeline):
    """Full per-instance pose for a fixed problem shape (or, with dynamic=True, for every shape up to its capacities, see
    CenterPipeline): the centre chain plus the pose tail, captured together in one hipGraph; `run()` replays it and
    reads back the 21-double record (one sync)."""

    def __init__(self, encoder, cfg, n_points, n_pairs, dims, device, sphere_pts, num_rots=72, adaptive=True,
                 angle_tol=1.5, max_rot_pairs=10000, use_graph=True, point_encoder=None, dynamic=False, rot_order_len=0,
                 vote_workgroups=0, idx_i32=False):
        """rot_order_len > 0: the pipeline owns a static i32[rot_order_len] buffer `rot_order` (positions in the survivor
        list, see estimate_pose) that the captured orientation vote reads -- fill it before run() to reproduce the reference's
        shuffled subsample (nocs/inference.py:277-280); it starts as 0, 1, 2, ... (= the first survivors)."""
        super().__init__(encoder, cfg, n_points, n_pairs, dims, device, num_rots, adaptive, False, use_graph, point_encoder,
                         dynamic, vote_workgroups, idx_i32)
        self.rot_order = (torch.arange(int(rot_order_len), dtype=I32, device=device) if rot_order_len else None)
        sph64 = np.asarray(sphere_pts, dtype=np.float64)
        self.ws = PoseWorkspace(device, n_pairs, self.dims, sph64.shape[0], grid=self.grid_flat if self.dynamic else self.grid)
        self.ws.out_idx, self.ws.out_val = self.out_idx, self.out_val
        self._sph = self.ws.sphere(sph64)
        self.angle_tol, self.max_rot_pairs = angle_tol, max_rot_pairs
        # bin counts / architectures the fused second pass (cppf_pair_mlp_decode_sel) does not serve run the full-first form
        # only: every head of every pair from the first pass, whose logits + decode-kernel fallback serves any configuration
        self._split_ok = encoder.fused_decode_supported(cfg.tr_num_bins, cfg.rot_num_bins)
        self.full_first = not self._split_ok

    # Two captured forms of the same computation.  Split (the reference's own order, nocs/inference.py:182-256): the first MLP
    # pass decodes the two centre heads only, the survivors of the back-vote get a second pass for the orientation / scale heads
    # -- 86 + 8 us at C2 when 0.4 % survive (a network that has not learnt the object), but 86 + 94 us when all do (a trained
    # one).  Full first: the first pass decodes every head of every pair (107 us) and there is no second pass.  Per pair the
    # arithmetic is the same, so the heads rows of the survivors, hence the pose, are identical; the choice follows the share
    # of survivors of the instance that ran last on this pipeline (break-even ~0.15, with hysteresis), seen in the record the
    # host reads back anyway (chains.next_form).
    FULL_FIRST_ON, FULL_FIRST_OFF = chains.FULL_FIRST_ON, chains.FULL_FIRST_OFF

    def adapt(self, n_surv):
        """choose the form for the next instance from the survivors of the last one"""
        # (the next run returns the tensors this form's launches write: outputs / heads / feat)
        self.full_first = chains.next_form(self.full_first, float(n_surv) / max(self.idx.shape[0], 1), self._split_ok)

    def _chain(self):
        self.with_heads = self.full_first
        outputs, heads, feat = super()._chain()   # (full first: heads = every pair's heads row, from the first pass)
        if not self.full_first:
            heads = self.ws.heads
        _enqueue_tail(self.ws, self.pc, self.nrm, self.idx32, outputs, heads, self.corner, self.cfg,
                      self.dims, self.num_rots, self.angle_tol, self.max_rot_pairs, *self._sph,
                      shape=self.shape if self.dynamic else None,
                      second_pass=None if self.full_first else (self.encoder, feat, self.idx, self.u_rot),
                      idx64=self.idx if self.idx.dtype == torch.int64 else None,   # the tail's kernels take int32 indices: written
                                                                                  # by the back-vote launch unless the list is int32 already
                      rot_order=self.rot_order)
        return outputs, heads, feat

    def run(self, rng=None, check_weights=True):
        super().run(check_weights)
        out = _assemble(self.ws.rec.cpu().numpy(), self.cfg, rng)
        out.update(dims=self.dims, ws=self.ws, outputs=self.outputs, heads=self.heads)
        self.adapt(out["n_surv"])
        return out

    def run_async(self, record_out, check_weights=True):
        """Replay the graph and copy the 21-double record into `record_out` (device f64[21]) on the current stream:
        no host synchronisation, so a batch of instances runs back to back (BatchPoseRunner reads all records back at
        once and assembles the poses with `assemble_record`)."""
        super().run(check_weights)
        if record_out is not None:          # (None: the caller collects the records itself, e.g. several pipelines' with one launch)
            record_out.copy_(self.ws.rec, non_blocking=True)

    def sample_inputs(self, seed, n_points=None):
        """Draw the pair list and the bin-sampling uniforms on the device (the reference draws the pairs with np.random.randint on
        the host and the bins with torch.multinomial, nocs/inference.py:177,186): 17 MB per instance at C2 that never cross PCIe.
        One launch (cppf_sample_pairs: Philox keyed by `seed`, counter = pair index; a torch.Generator is accepted for its
        initial_seed()): 6 us where torch's two generator kernels took 38.  Same distribution as the reference's draws, not the
        same stream of numbers -- parity tests pass explicit arrays."""
        if self.idx.dtype != torch.int64:
            raise _lib.CppfError("sample_inputs() draws int64 pair lists (cppf_sample_pairs); an int32 pipeline is filled by a staged chain")
        n = self.shape_host[0] if self.dynamic else self.pc.shape[0]
        n = int(n_points) if n_points is not None else n
        if isinstance(seed, torch.Generator):
            seed = seed.initial_seed()
        call("cppf_sample_pairs", self.device, self.idx, self.u_tr, self.u_rot, self.idx.shape[0], n, None, int(seed) & 0xFFFFFFFFFFFFFFFF,
             None)


class PoseChain(_Captured):
    """Up to 8 PosePipelines -- the instances of a frame on one HIP stream (the reference loops over them, nocs/inference.py:120) --
    replayed as ONE captured chain with the launches SHARED between the members: their point encoders one after the other, then ONE
    launch of the pair kernel for all pair lists (forward_decode_batch), ONE vote + ONE reduce launch (vote_argmax_batch) and the six
    launches of the batched tail (cppf_pose_tail_batch: T, back-vote, compaction, second pass, orientation vote, sums) -- about
    10 + n launches for n instances instead of ~15 each.  At the reference's own size (100 000 pairs, :177) a launch is half prologue,
    so the launches were what an instance cost.  Members keep their buffers (load / stage them as usual) and their result records
    (`pipes[i].ws.rec`); records equal the members' own runs bit for bit (at the chain's vote width).

    Members: pose pipelines of ONE device with the standard fused pair encoder, the same num_rots / adaptive / angle_tol /
    max_rot_pairs / sphere bins, no rot_order, grids of the tiled vote; static or shape-polymorphic, any categories.  Like a
    PosePipeline the chain has two captured forms -- split (second pass on the survivors) and full-first (every head in the first
    pass) -- chosen from the survivor share of its last run (adapt)."""

    FULL_FIRST_ON, FULL_FIRST_OFF = chains.FULL_FIRST_ON, chains.FULL_FIRST_OFF

    @staticmethod
    def takes(p, first):
        """can `p` be a member of a chain whose first member is `first`?  (the class docstring's "Members")"""
        return (isinstance(p, PosePipeline) and p._split_ok and p.rot_order is None and p._sph[2] != 0
                and (p.device, p.num_rots, p.adaptive, p.angle_tol, p.max_rot_pairs, p.ws._sph_key)
                == (first.device, first.num_rots, first.adaptive, first.angle_tol, first.max_rot_pairs, first.ws._sph_key))

    def __init__(self, pipes, use_graph=True, vote_workgroups=0, prestages=None, staged=False):
        """prestages: optional list of callables, one per member (or None): launches enqueued at the head of the chain, in front of
        the member's point encoder -- e.g. the count-driven pre-processing that fills the member's cloud, normals, corner and shape
        record from a depth frame (cppf_amd.frames.FrameRunner).
        staged=True: the chain serves objects that are ALREADY on the device (run_staged): its first launch (cppf_stage_batch) copies
        each member's cloud / normals / features from where the caller keeps them, sets up its grid and draws its pairs and bin
        uniforms -- all read from a 48-byte device descriptor per member, rewritten with one small copy per replay -- and its last
        launch assembles the members' FINISHED records (`records` f64[n, sharding.RECORD], the host end of nocs/inference.py:299-339
        on the device): nothing comes back to the host."""
        pipes = list(pipes)
        if not 1 <= len(pipes) <= 8:
            raise ValueError("1 to 8 pipelines per chain")
        self.prestages = list(prestages) if prestages is not None else [None] * len(pipes)
        if len(self.prestages) != len(pipes):
            raise ValueError("one prestage (or None) per pipeline")
        p0 = pipes[0]
        if not all(self.takes(p, p0) for p in pipes):
            raise _lib.CppfError("PoseChain takes PosePipelines of one device with the standard pair encoder and the same vote / "
                                 "orientation settings (no rot_order)")
        if len({id(p) for p in pipes}) != len(pipes):
            raise ValueError("a pipeline can be a member once")
        self.pipes, self.device = pipes, p0.device
        self.vote_workgroups = int(vote_workgroups or 0)
        self.full_first = False
        self._cache, self.tensors = _GraphCache(self, use_graph), None     # tensors: outputs / heads / feat per member, of the last run
        self.staged = bool(staged)
        if self.staged:
            from .sharding import RECORD
            n, W = len(pipes), _lib.STAGE_DESC_WORDS
            self.desc = torch.zeros((n, W), dtype=torch.int64, device=self.device)       # CppfStageDesc per member
            self.records = torch.zeros((n, RECORD), dtype=torch.float64, device=self.device)
            # a ring of pinned descriptor blocks: a block is rewritten only after the copy that last read it has executed
            self._desc_ring = []
            for _ in range(4):
                h = torch.zeros((n, W), dtype=torch.int64).pin_memory()
                self._desc_ring.append((h, h.numpy().view(np.uint64), torch.cuda.Event()))
            self._ring_pos = 0

    def _stage(self):
        """the chain's first launch (staged chains): clouds in, grids set up, pairs and uniforms drawn (cppf_stage_batch)"""
        pipes = self.pipes
        arr = (_lib.StageItem * len(pipes))()
        for i, p in enumerate(pipes):
            fill(arr[i], self.device, desc=self.desc[i], pc=p.pc, nrm=p.nrm, corner=p.corner, feat=p.feat if p.point_encoder is None else None,
                 shape=p.shape if p.dynamic else None, idx=p.idx, u_tr=p.u_tr, u_rot=p.u_rot, n_pairs=p.idx.shape[0], n_cap=p.pc.shape[0],
                 F=p.feat.shape[1], res=float(np.float32(p.cfg.res)), idx_is_i64=p.idx.dtype == torch.int64)
        call("cppf_stage_batch", self.device, len(pipes), arr)

    def _chain(self):
        from .models.model import forward_decode_batch
        pipes, p0 = self.pipes, self.pipes[0]
        L = _lib.lib()
        if self.staged:                                                          # nocs/inference.py:177,194-196 for resident objects
            self._stage()
        for pre in self.prestages:                                               # nocs/inference.py:131-142 (FrameRunner)
            if pre is not None:
                pre()
        # (the members' own attributes are left alone: a member may also run on its own captured graph)
        # nocs/inference.py:180-181.  The shape-polymorphic members' encoders share three launches (search, convolution,
        # GlobalInfoProp for all of them: a cloud of 700-2000 points fills a quarter of the chip); others run one after the other.
        enc_members = [p for p in pipes if p.point_encoder is not None and p.dynamic]
        batched = len(enc_members) > 1 and not os.environ.get("CPPF_NO_POINT_BATCH")      # (the knob: A/B measurements)
        if batched:
            from .models.model import point_encoder_forward_batch
            point_encoder_forward_batch([dict(encoder=p.point_encoder, pc=p.pc, nrm=p.nrm, n_dev=p.shape, out=p._feat_out,
                                              nbrs=p._nbrs, nbrs_ready=p.nbrs_ready) for p in enc_members])
        feats = [p._feat_out if batched and p in enc_members else _point_features(p) for p in pipes]
        tables = []
        outs = forward_decode_batch(_decode_items(pipes, feats, self.full_first), p0.cfg.tr_num_bins, p0.cfg.rot_num_bins,
                                    tables_out=tables)                                                           # :182-188
        outputs = [o for o, _ in outs]
        heads = [(h if self.full_first else p.ws.heads) for p, (_, h) in zip(pipes, outs)]
        vws = []
        voting.vote_argmax_batch(_vote_items(pipes, outputs), p0.num_rots, p0.adaptive, accumulate=False,
                                 workgroups=self.vote_workgroups, workspaces_out=vws)                            # :191-208
        arr = (_lib.PoseTailItem * len(pipes))()
        keep = []
        sph32, sph64, sorted_y = p0._sph
        for i, p in enumerate(pipes):
            ws = p.ws
            pws = workspace(L.cppf_pose_sums_workspace_bytes(), self.device, f"pose_sums{i}")
            packed = p.encoder._packed_weights(self.device)
            gx, gy, gz = (1, 1, 1) if p.dynamic else p.dims
            # (idx64 None: the list is int32, idx32 is the input)
            fill(arr[i], self.device, pc=p.pc, nrm=p.nrm, feat=feats[i], idx32=p.idx32, idx64=p.idx if p.idx.dtype == torch.int64 else None,
                 outputs=outputs[i], u_rot=p.u_rot, heads=heads[i], corner=p.corner, shape_dev=p.shape if p.dynamic else None,
                 argmax_idx=p.out_idx, peak=p.out_val, packed=packed, mlp_workspace=scratch(tables[i]),
                 vote_workspace=vws[i] if vws[i].numel() >= 32768 else None, rec=ws.rec, T32=ws.T32, tail0=scratch(ws._tail0),
                 mask=ws.mask, chunk_counts=ws.chunk_counts, surv=ws.surv, count=ws.count, counts=ws.counts, best_idx=ws.best_idx,
                 ticket=ws.ticket, sums_workspace=scratch(pws), n_points=p.pc.shape[0], n_pairs=p.idx.shape[0], res64=float(p.cfg.res),
                 res=float(p.cfg.res), tol=float(np.float32(3 * p.cfg.res)), gx=gx, gy=gy, gz=gz, n_dirs=2 if p.cfg.regress_right else 1,
                 second_pass=0 if self.full_first else (2 if p.encoder.precision == "bf16" else 1))
            if self.staged:                      # the finished record, assembled by the last launch (:299-339)
                fill(arr[i], self.device, record_out=self.records[i], object_id_dev=self.desc[i].data_ptr() + 40,
                     scale_mean=(C.c_double * 3)(*[float(v) for v in p.cfg.scale_mean]), regress_right=bool(p.cfg.regress_right))
            keep.append((pws, packed))
        dims = (C.c_int * len(p0.encoder.ppffcs))(*p0.encoder.ppffcs)
        thr = float(np.float32(np.cos(p0.angle_tol / 180 * np.pi)))
        call("cppf_pose_tail_batch", self.device, len(pipes), arr, feats[0].shape[1], dims, len(p0.encoder.ppffcs) - 1, p0.encoder.out_dim,
             p0.cfg.tr_num_bins, p0.cfg.rot_num_bins, p0.num_rots, sph32, sph64, sph32.shape[0], sorted_y, thr,
             p0.max_rot_pairs)                                                                                   # :209-303,335
        return [dict(outputs=o, heads=h, feat=f) for o, h, f in zip(outputs, heads, feats)]

    def _key(self):
        return (self.vote_workgroups,) + tuple((p.idx.data_ptr(), p.pc.data_ptr()) for p in self.pipes)

    def run_staged(self, objs, seeds, ids, rows_out, check_weights=None, capture=True):
        """Staged chains: objs[i] = dict(pc, normals[, feat]) of DEVICE f32 tensors (contiguous; they must stay alive and unchanged
        until the chain has run), seeds[i] the Philox key of member i's pair / uniform draws, ids[i] its object id; rows_out: device
        f64[n, RECORD] that receives the members' finished records (one device copy).  No host synchronisation.
        capture=False: a chain that has no captured graph yet runs its launches eagerly this time (a one-off combination)."""
        n = len(self.pipes)
        host, words, ev = self._desc_ring[self._ring_pos % len(self._desc_ring)]
        self._ring_pos += 1
        ev.synchronize()
        for i, (o, p) in enumerate(zip(objs, self.pipes)):
            feat = o.get("feat") if p.point_encoder is None else None
            if feat is None and p.point_encoder is None:
                raise ValueError(f"member {i}: no `feat` and no point encoder in its pipeline (the chain would reuse the last object's features)")
            if o["pc"].shape[0] > p.pc.shape[0] or (feat is not None and feat.shape != (o["pc"].shape[0], p.feat.shape[1])):
                raise ValueError(f"member {i}: cloud of {o['pc'].shape[0]} points / features {None if feat is None else tuple(feat.shape)} "
                                 f"do not fit a pipeline of {p.pc.shape[0]} x {p.feat.shape[1]}")
            words[i] = (o["pc"].data_ptr(), o["normals"].data_ptr(), 0 if feat is None else feat.data_ptr(), o["pc"].shape[0],
                        int(seeds[i]) & 0xFFFFFFFFFFFFFFFF, int(ids[i]))
        copy_words(self.desc, host, self.device)          # (kernels, not copy engines: see cppf_copy_words)
        ev.record(torch.cuda.current_stream(self.device))
        self.run_async(None, check_weights, eager=not capture and self._graph is None)
        copy_words(rows_out, self.records[:rows_out.shape[0]], self.device)

    def run_async(self, records_out, check_weights=True, eager=False):
        """Replay the chain and copy every member's 21-double record into records_out[i] (device f64[21]) on the current stream
        (records_out None: no copies).  eager: launch instead of capturing / replaying."""
        self.tensors = self._cache.run(self._chain, self.pipes, check_weights, self._key(), self.full_first, eager)
        for p, r in zip(self.pipes, records_out or ()):
            r.copy_(p.ws.rec, non_blocking=True)

    def run(self, check_weights=True):
        """-> the members' pose dicts (one host synchronisation for all of them)"""
        recs = torch.empty((len(self.pipes), 21), dtype=torch.float64, device=self.device)
        self.run_async(list(recs), check_weights)
        host = recs.cpu().numpy()
        out = []
        for p, r in zip(self.pipes, host):
            d = _assemble(r, p.cfg)
            d.update(dims=p.dims, ws=p.ws)
            out.append(d)
        for d, tn in zip(out, self.tensors):
            d.update(outputs=tn["outputs"], heads=tn["heads"])
        self.adapt([d["n_surv"] for d in out])
        return out

    def adapt(self, n_survs):
        """choose the form of the next run from the survivor shares of the last one (see PosePipeline.adapt)"""
        share = float(np.mean([float(n) / max(p.idx.shape[0], 1) for n, p in zip(n_survs, self.pipes)]))
        self.full_first = chains.next_form(self.full_first, share)

    def release(self):
        self.tensors = None
        super().release()


def assemble_batch(recs, cfgs, object_ids, n_cols):
    """_assemble + sharding.pack_record for a whole batch in one numpy pass: recs f64[n,21] (read back from the device),
    cfgs a list of n category configs -> f64[n, n_cols] = {T, up, right, scale, argmax, peak, n_surv, object id}.
    Same arithmetic per row as _assemble (nocs/inference.py:299-339); a row whose `right` degenerates (|right| < 1e-7, :325)
    goes through _assemble itself for its random fallback."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 21)
    n = recs.shape[0]
    out = np.zeros((n, n_cols), np.float64)
    if n == 0:
        return out
    if np.any(recs[:, 19] < 0):
        raise _lib.CppfError("an instance shape did not fit the shape-polymorphic pipeline it ran on (arg-max index -1)")
    rr = np.array([bool(c.regress_right) for c in cfgs])
    sm = np.array([c.scale_mean for c in cfgs], np.float64)
    best = recs[:, 3:9].reshape(n, 2, 3)
    sign = recs[:, 9:15].reshape(n, 2, 3)
    cnt = np.maximum(sign[:, :, 2], 1.0)
    flip = (sign[:, :, 1] / cnt) < (sign[:, :, 0] / cnt)                  # down_loss < up_loss  (:299-302)
    dirs = np.where(flip[:, :, None], -best, best)
    up = dirs[:, 0]
    right_r = dirs[:, 1] - np.sum(up * dirs[:, 1], -1, keepdims=True) * up  # :305-312
    right_n = np.stack([np.zeros(n), -up[:, 2], up[:, 1]], -1)
    right = np.where(rr[:, None], right_r, right_n)
    right = right / (np.linalg.norm(right, axis=-1, keepdims=True) + 1e-9)
    n_surv = recs[:, 18].astype(np.int64)
    mean = (recs[:, 15:18] / np.maximum(n_surv, 1)[:, None]).astype(np.float32)     # torch mean is fp32
    scale = np.exp(mean).astype(np.float64) * sm * 2                                  # :335
    out[:, 0:3], out[:, 3:6], out[:, 6:9], out[:, 9:12] = recs[:, 0:3], up, right, scale
    out[:, 12], out[:, 13], out[:, 14], out[:, 15] = recs[:, 19], recs[:, 20], n_surv, np.asarray(object_ids, np.float64)
    for i in np.nonzero(np.linalg.norm(right, axis=-1) < 1e-7)[0]:                    # :325-328, random fallback
        p = _assemble(recs[i], cfgs[i])
        out[i, 3:6], out[i, 6:9] = p["up"], p["right"]
    return out


def assemble_record(rec, cfg, rng=None):
    """pose dict from one 21-double record read back from a PosePipeline (see PosePipeline.run_async)"""
    return _assemble(np.asarray(rec, dtype=np.float64), cfg, rng)
