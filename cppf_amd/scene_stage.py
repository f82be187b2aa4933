"""The proposal stage of a scene with no instance masks, shared by the notebook's path (zero_shot.py, 9-wide regression head) and
the mask-free path (scene_poses.py, bin head): the callers' input forms, the frame pre-processing of nocs/zero_shot.ipynb cells
3-6, the scene vote with its proposals (cells 8-9) and cell 11's back-vote and segmentation of ALL proposals in one pass over the
pair list (csrc/scene_multi.hip).  What the heads do with each proposal's kept pairs stays in the two modules.  The pre-processing is
scene_cloud (every caller's clouds, labelled or not) and cloud_inputs (features, draw, filter: frame_inputs' and segment_inputs' body)."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._torch_util import call, canon, scratch, workspace
from .models import voting
from .utils.util import fibonacci_sphere, num_sphere_bins

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MAX_CENTERS = 32                          # csrc/scene_multi.hip: BVM_MAX_CENTERS (one bit per proposal in a 32-bit word)
MAX_PAIRS = 1 << 27                       # csrc/scene_multi.hip: BVM_MAX_PAIRS (a queue entry is pair << 5 | k in one word)


def pairs_tensor(idx, dev):
    """the pair list as PPFEncoder takes it: a numpy array is host data and is uploaded (other integer widths widened); a tensor
    must be int32 / int64 on `dev` -- any strides"""
    if not isinstance(idx, torch.Tensor):
        a = np.asarray(idx)
        if a.dtype.kind not in "iu":
            raise TypeError(f"pair list: expected integers, got {a.dtype}")
        idx = torch.from_numpy(np.ascontiguousarray(a if a.dtype in (np.int32, np.int64) else a.astype(np.int64))).to(dev)
    return canon(idx, (torch.int64, torch.int32), dev, "pair list", (2,))


def on_device(x, dev, name, tail=None):
    """f32 data of the caller on `dev`: a numpy array (or list) is uploaded, a tensor is converted where it is or refused"""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(dev)
    return canon(x, F32, dev, name, tail)


def kept_positions(pc, nrm, idx):
    """Cell 6: the positions (i64, in order) of the pairs of `idx` that are not "indistinguishable"; device tensors in"""
    dev = pc.device
    P = idx.shape[0]
    keep = torch.empty(max(P, 1), dtype=U8, device=dev)
    pos = torch.empty(max(P, 1), dtype=I32, device=dev)
    count = torch.zeros(1, dtype=I32, device=dev)
    if P:
        call("cppf_pair_filter_distinct", dev, pc, nrm, idx, idx.dtype == torch.int64, pc.shape[0], P, keep)
        cws = workspace(_lib.lib().cppf_compact_workspace_bytes(P), dev, "compact")
        call("cppf_compact_mask", dev, keep, P, pos, count, scratch(cws))
    return pos[:int(count.item())].long()


def sphere_tables(angle_tol, dev):
    """the orientation bins of nocs/inference.py:100-102: (fp64 host, fp32 device, fp64 device, order of the y column for the banded
    count -- PoseWorkspace.sphere's rule; 1 for the Fibonacci sphere)"""
    sph64 = np.array(fibonacci_sphere(num_sphere_bins(angle_tol)), np.float64)
    s32 = sph64.astype(np.float32)
    unit = bool(np.all(np.abs(np.linalg.norm(s32.astype(np.float64), axis=-1) - 1.0) < 1e-4))
    dy = np.diff(s32[:, 1])
    sorted_y = (1 if np.all(dy <= 0) else (-1 if np.all(dy >= 0) else 0)) if unit else 0
    return sph64, torch.from_numpy(s32).to(dev), torch.from_numpy(sph64).to(dev), sorted_y


class SceneCloud(NamedTuple):
    """scene_cloud's record, device tensors: the dense cloud (res), the sparse cloud (4 res), their labels (None: no label image)"""
    hi: torch.Tensor                      # f32[M,3]
    hi_nrm: torch.Tensor                  # f32[M,3]
    hi_labels: Optional[torch.Tensor]     # i32[M]
    ind: torch.Tensor                     # i64[N]
    pc: torch.Tensor                      # f32[N,3] = hi[ind]
    nrm: torch.Tensor                     # f32[N,3] = hi_nrm[ind]
    labels: Optional[torch.Tensor]        # i32[N] = hi_labels[ind]


def scene_cloud(depth, intrinsics, cfg, jitter=None, labels=None):
    """Cell 3 on the device, a SceneCloud: frames._cloud_and_pixels with every pixel in the mask (jitter: f32[n_pixels,3] standard-normal
    draws, None: none), then sparse_quantize at 4 res.  labels: an integer image [H,W] (tensor; -1 = none), read at each dense point's
    own pixel.  A function of (depth, intrinsics, cfg.res, cfg.knn, jitter, labels) alone: categories whose configs agree in (res, knn)
    can share it (cloud= of frame_inputs, segments.segment_inputs, scene_poses.scene_frame).  No valid pixel: ValueError."""
    from .frames import _cloud_and_pixels
    from .utils.util import sparse_quantize
    d = np.asarray(depth) if not isinstance(depth, torch.Tensor) else depth
    hi, hi_nrm, pix = _cloud_and_pixels(depth, intrinsics, np.ones(tuple(d.shape), bool), cfg, jitter)
    if hi.shape[0] == 0:
        raise ValueError("the depth frame has no valid pixels")
    _, ind = sparse_quantize(hi, return_index=True, quantization_size=4 * cfg.res)
    lab = None if labels is None else labels.to(hi.device).reshape(-1)[pix.long()].to(I32).contiguous()
    return SceneCloud(hi, hi_nrm, lab, ind, hi[ind].contiguous(), hi_nrm[ind].contiguous(), None if lab is None else lab[ind].contiguous())


def frame_cloud(depth, intrinsics, cfg, jitter=None):
    """scene_cloud without labels"""
    return scene_cloud(depth, intrinsics, cfg, jitter)


def cloud_inputs(cloud, point_encoder, n_pairs, seed, pairs=None):
    """Cells 5-7 on a SceneCloud: SPRIN features on the dense cloud (its own kNN) taken at `ind`, frames.draw_pairs(seed, 0, ...) and the
    "indistinguishable" filter.  pairs: an i64[n_pairs,2] list to filter in place of the draw's (the bin uniforms stay the draw's).
    Returns hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot): the filter keeps a subset in order, the uniforms go through its positions."""
    from .frames import draw_pairs
    hi, hi_nrm, _, ind, pc, nrm, _ = cloud
    with torch.no_grad():
        feat = point_encoder(hi[None], hi_nrm[None])[0][ind].contiguous()                        # cell 7
    idx, u = draw_pairs(seed, 0, int(n_pairs), pc.device, pc.shape[0])                            # cell 5
    idx = idx if pairs is None else pairs
    pos = kept_positions(pc, nrm, idx)                                                            # cell 6
    return hi, hi_nrm, ind, pc, nrm, feat, idx[pos].contiguous(), (u[0][pos].contiguous(), u[1][pos].contiguous())


def frame_inputs(depth, intrinsics, point_encoder, cfg, n_pairs, seed, jitter=None, cloud=None):
    """Cells 3-6 on the device: scene_cloud (cloud=: the SceneCloud of this frame instead), then cloud_inputs with its own draw"""
    return cloud_inputs(scene_cloud(depth, intrinsics, cfg, jitter) if cloud is None else cloud, point_encoder, n_pairs, seed)


def vote_proposals(pc, outputs, idx32, cfg, num_rots, sigma, thresh, margin, max_proposals, max_iters):
    """Cells 8-9: the scene vote (adaptive, overwrite mode), the smoothed-grid proposals and their one read-back.  Returns grid (raw
    vote, device), corners, dims (inference.grid_shape's), corner (device f32[3]), loc i32[K,3], val, diff (numpy) and worlds
    f64[K,3] = corners[0] + loc * res in fp64 from the float32 corner."""
    from .inference import grid_shape
    from .zero_shot import scene_proposals_device
    dev = pc.device
    corners, dims = grid_shape(pc.cpu().numpy(), cfg.res)
    corner = torch.from_numpy(corners[0].copy()).to(dev)
    grid = torch.empty(dims, dtype=F32, device=dev)
    voting.vote_argmax(pc, outputs, None, idx32, grid, corner, cfg.res, num_rots, True, accumulate=False)
    loc, val, diff, count = scene_proposals_device(grid, sigma, thresh, margin, max_proposals, max_iters)
    n = int(count.item())
    loc, val, diff = loc[:n].cpu().numpy(), val[:n].cpu().numpy(), diff[:n].cpu().numpy()
    worlds = corners[0].astype(np.float64)[None] + loc.astype(np.int64) * float(cfg.res)
    return grid, corners, dims, corner, loc, val, diff, worlds


def backvote_multi(pc, outputs, idx32, corner, res, dims, centers, num_rots=72, tol=None, vote_ws=None, out=None):
    """cppf_backvote_multi: bit k of the returned u32[P] (an int32 tensor) = pair p survives the back-vote at centers[k] (device
    f32[K,3], K <= 32); tol = float32(3 res) by default.  Everything is enqueued on the current stream."""
    dev = pc.device
    P, K = idx32.shape[0], centers.shape[0]
    tol = float(np.float32(3 * res)) if tol is None else float(np.float32(tol))
    bits = torch.empty(max(P, 1), dtype=I32, device=dev) if out is None else out
    gx, gy, gz = (int(d) for d in dims)
    call("cppf_backvote_multi", dev, pc, outputs, idx32, corner, float(res), P, int(num_rots), gx, gy, gz, centers, K, tol, bits, vote_ws)
    return bits


def segment_instances(idx32, bits, n_points, n_centers, min_contrib=12, capacity=None):
    """cppf_segment_instances: (point_masks u8[K,N], pairs i32[capacity], offsets i32[K+1]) device tensors, all enqueued; the kept
    pairs of proposal k are pairs[offsets[k]:offsets[k+1]] when offsets[K] <= capacity (default: the number of pairs)"""
    dev = idx32.device
    P, K, N = idx32.shape[0], int(n_centers), int(n_points)
    capacity = P if capacity is None else int(capacity)
    masks = torch.empty((K, N), dtype=U8, device=dev)
    pairs = torch.empty(max(capacity, 1), dtype=I32, device=dev)
    offsets = torch.empty(K + 1, dtype=I32, device=dev)
    ws = workspace(_lib.lib().cppf_segment_instances_workspace_bytes(N, P, K), dev, "segment_multi")
    call("cppf_segment_instances", dev, idx32, bits, P, N, K, int(min_contrib), masks, pairs, capacity, offsets, scratch(ws))
    return masks, pairs, offsets


def proposal_group(n_pairs):
    """how many proposals one pass over a list of n_pairs pairs serves: 32 (one bit each), fewer where n_pairs x group would pass
    cppf_segment_instances' int32 offsets"""
    return max(1, min(MAX_CENTERS, (2 ** 31 - 1) // max(int(n_pairs), 1)))


def segment_proposals(pc, outputs, idx32, corner, res, dims, worlds, num_rots, tol, min_contrib, vote_ws=None, capacity=None):
    """Cell 11's back-vote (tol = float32(3 res) when None) and "unsupervised instance segmentation" at every proposal centre
    `worlds` ([K,3], handed on as fp32).  The centres go in groups of at most 32 (one bit each; fewer where P x group would pass
    cppf_segment_instances' int32 offsets): per group one pass over the pair list and one read of its offsets, and where the kept
    (pair, proposal) items outnumber `capacity` (default P) cppf_segment_instances alone once more with the reported size.
    Returns (masks u8[K,N], pairs i32: device; offsets i64[K+1]: host; counts i32[K], bits (each group's survivor words): device);
    the kept pairs of proposal k are pairs[offsets[k]:offsets[k+1]], positions in idx32 in order."""
    dev = pc.device
    N, P = pc.shape[0], idx32.shape[0]
    if P >= MAX_PAIRS:
        raise ValueError(f"the pair list has {P} pairs; one pass over all proposals takes fewer than {MAX_PAIRS} (2^27)")
    centers = torch.from_numpy(np.ascontiguousarray(np.asarray(worlds, np.float64).reshape(-1, 3).astype(np.float32))).to(dev)
    K = centers.shape[0]
    group = proposal_group(P)
    masks, pairs, counts, bits, offsets = [], [], [], [], [0]
    for g in range(0, K, group):
        kg = min(group, K - g)
        b = backvote_multi(pc, outputs, idx32, corner, res, dims, centers[g:g + kg], num_rots, tol, vote_ws)
        m, p, off_d = segment_instances(idx32, b, N, kg, min_contrib, capacity)
        off = off_d.cpu().numpy().astype(np.int64)
        if off[kg] > p.shape[0]:                                              # more kept (pair, proposal) items than room: once more
            m, p, off_d = segment_instances(idx32, b, N, kg, min_contrib, capacity=int(off[kg]))
        masks.append(m), pairs.append(p[:int(off[kg])]), counts.append(off_d[1:] - off_d[:-1]), bits.append(b)
        offsets.extend(offsets[g] + off[1:])
    if len(masks) == 1:                                                       # (the usual case: nothing to join)
        return masks[0], p, np.array(offsets, np.int64), counts[0].contiguous(), bits
    cat = lambda ts, dt, *shape: torch.cat(ts + [torch.empty(shape, dtype=dt, device=dev)])      # (pairs: never an empty buffer)
    return cat(masks, U8, 0, N), cat(pairs, I32, 1), np.array(offsets, np.int64), cat(counts, I32, 0), bits


# ----------------------------------------------------------------------------- proposal masks -> instance clouds (csrc/instances.hip)
GATHER_CHUNK, GATHER_MAX_CHUNKS = 1024, 8192      # include/cppf.h: CPPF_GATHER_CHUNK, CPPF_GATHER_MAX_CHUNKS


def voxel_owner(hi, pc_index, q):
    """i32[M] on hi's device: for every point of the dense cloud hi f32[M,3] the position in the sparse cloud hi[pc_index] of the
    point that represents its voxel of edge q, -1 where no sparse point has that voxel (pc_index: frame_inputs' `ind`, q = 4 cfg.res;
    on sparse_quantize's output every dense point has an owner.  A caller's own subset may leave voxels out, or name one twice: the
    first position then owns it).  The voxel is floor((double)p / q) per axis by TRUE division, sparse_quantize's arithmetic
    (utils/util.py:117-121): a tensor divisor divides, a Python number would be multiplied by as its reciprocal and move points on a
    voxel face into the neighbouring voxel.  Points that are not finite or beyond 2^20 voxels from the origin (the range of
    cppf_voxel_dedupe's key) get -1.  Torch ops on the device (keys, one sort, one searchsorted): it runs once per cloud, and every
    category whose config shares (res, knn) can reuse the result."""
    dev = hi.device
    hi = canon(hi, F32, dev, "hi", (3,))
    pc_index = canon(pc_index, (torch.int64, torch.int32), dev, "pc_index").reshape(-1).long()
    M, n = hi.shape[0], pc_index.shape[0]
    if M == 0 or n == 0:
        return torch.full((M,), -1, dtype=I32, device=dev)
    if int(pc_index.min()) < 0 or int(pc_index.max()) >= M:
        raise ValueError(f"pc_index must index the dense cloud (0..{M - 1})")
    p64 = hi.double()
    v = torch.floor(p64 / torch.full_like(p64, float(q)))
    ok = (torch.isfinite(v) & (v >= -(1 << 20)) & (v < (1 << 20))).all(dim=1)
    c = torch.where(ok[:, None], v, torch.zeros_like(v)).long() + (1 << 20)
    key = torch.where(ok, (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], torch.full((M,), -1, dtype=torch.int64, device=dev))
    sk, order = torch.sort(key[pc_index], stable=True)
    pos = torch.searchsorted(sk, key)                                         # (left: the first of equal keys)
    pos_c = pos.clamp(max=n - 1)
    hit = ok & (pos < n) & (sk[pos_c] == key)
    return torch.where(hit, order[pos_c], torch.full_like(pos_c, -1)).to(I32)


def check_gather_args(n_props, n_sparse, n_dense, capacity):
    """the refusals of cppf_gather_instances that need no device, as ValueError"""
    K, N, M, cap = int(n_props), int(n_sparse), int(n_dense), int(capacity)
    if not 1 <= K <= MAX_CENTERS:
        raise ValueError(f"gather_instances takes 1..{MAX_CENTERS} masks (one bit per proposal), got {K}")
    if N < 0 or M < 0 or cap < 0:
        raise ValueError(f"negative size: n_sparse {N}, n_dense {M}, capacity {cap}")
    if M > 2 ** 31 - 1 or K * M > 2 ** 31 - 1 or N > 2 ** 31 - 1:
        raise ValueError(f"{K} masks over {M} dense points pass the int32 offsets")
    if (M + GATHER_CHUNK - 1) // GATHER_CHUNK > GATHER_MAX_CHUNKS:
        raise ValueError(f"{M} dense points: one pass takes at most {GATHER_CHUNK * GATHER_MAX_CHUNKS}")


def gather_instances_device(hi, hi_nrm, owner, masks, capacity=None, out=None):
    """cppf_gather_instances, enqueued on the current stream with nothing read back: dict(member i32[M] (the u32 words), offsets
    i32[K+1], pts f32[capacity,3], nrm f32[capacity,3], src i32[capacity]) of device tensors; capacity: M by default; out: such a dict
    to write into (the caller's buffers)."""
    dev = hi.device
    (K, N), M = masks.shape, hi.shape[0]
    capacity = M if capacity is None else int(capacity)
    check_gather_args(K, N, M, capacity)
    if out is None:
        out = dict(member=torch.empty(max(M, 1), dtype=I32, device=dev), offsets=torch.empty(K + 1, dtype=I32, device=dev),
                   pts=torch.empty((max(capacity, 1), 3), dtype=F32, device=dev), nrm=torch.empty((max(capacity, 1), 3), dtype=F32, device=dev),
                   src=torch.empty(max(capacity, 1), dtype=I32, device=dev))
    counts = torch.empty(max(K * ((M + GATHER_CHUNK - 1) // GATHER_CHUNK), 1), dtype=I32, device=dev)
    call("cppf_gather_instances", dev, hi, hi_nrm, owner, masks, K, N, M, capacity, out["member"], out["offsets"], out["pts"], out["nrm"],
         out["src"], counts)
    return out


def gather_instances(hi, hi_nrm, owner, masks, capacity=None):
    """Proposal masks -> instance clouds, all proposals of a group in one pass over the dense cloud (cppf_gather_instances).
    hi, hi_nrm f32[M,3]: the dense cloud and its normals; owner i32[M]: voxel_owner's map; masks u8[K,N], K <= 32: the point_masks
    of segment_proposals (over the sparse cloud): device tensors.
    Returns (pts f32[T,3], nrm f32[T,3], src i32[T]: device; offsets i64[K+1]: host; member i32[M] (bit k = dense point i belongs to
    proposal k): device): proposal k's points are rows offsets[k]:offsets[k+1], in increasing dense index -- hi[member_k].  The K + 1
    offsets are read back once; where the members outnumber `capacity` rows (default M) the call runs once more with the reported
    size.  An owner >= N raises ValueError (found on the device, nothing was gathered)."""
    dev = hi.device
    hi, hi_nrm = canon(hi, F32, dev, "hi", (3,)), canon(hi_nrm, F32, dev, "hi_nrm", (3,))
    owner, masks = canon(owner, I32, dev, "owner"), canon(masks, U8, dev, "masks")
    if masks.dim() != 2 or owner.shape != (hi.shape[0],) or hi_nrm.shape != hi.shape:
        raise ValueError(f"gather_instances: hi {tuple(hi.shape)}, hi_nrm {tuple(hi_nrm.shape)}, owner {tuple(owner.shape)}, masks "
                         f"{tuple(masks.shape)}: expected [M,3], [M,3], [M], [K,N]")
    K = masks.shape[0]
    capacity = hi.shape[0] if capacity is None else int(capacity)
    g = gather_instances_device(hi, hi_nrm, owner, masks, capacity)
    off = g["offsets"].cpu().numpy().astype(np.int64)
    if off[K] < 0:
        raise ValueError(f"gather_instances: an owner is >= {masks.shape[1]}, the number of sparse points the masks speak of")
    if off[K] > capacity:
        g = gather_instances_device(hi, hi_nrm, owner, masks, capacity=int(off[K]))
    T = int(off[K])
    return g["pts"][:T], g["nrm"][:T], g["src"][:T], off, g["member"][:hi.shape[0]]


# ----------------------------------------------------------------------------- proposal verification (csrc/verify.hip)
VERIFY_COUNTS = ("within", "agree", "cross", "cross_agree", "mask_pts", "mask_in_box", "box_pts")
VERIFY_RATIOS = (("agreement", "agree", "within"), ("leak", "cross_agree", "cross"), ("fill", "mask_in_box", "mask_pts"),
                 ("purity", "mask_in_box", "box_pts"))


def proposal_support(idx32, bits, masks, out=None):
    """cppf_proposal_support: i32[K,4] (within, agree, cross, cross_agree) on the device for the K <= 32 rows of masks (u8[K,N], as
    segment_instances writes them) and their survivor words `bits`; enqueued on the current stream, nothing is read back"""
    dev = idx32.device
    P, (K, N) = idx32.shape[0], masks.shape
    counts = torch.empty((K, 4), dtype=I32, device=dev) if out is None else out
    ws = workspace(_lib.lib().cppf_proposal_support_workspace_bytes(N), dev, "proposal_support")
    call("cppf_proposal_support", dev, idx32, bits, masks, P, N, K, counts, scratch(ws))
    return counts


def box_support(pc, masks, centers, axes, half, out=None):
    """cppf_box_support: i32[K,3] (mask_pts, mask_in_box, box_pts) on the device for K <= 32 oriented boxes -- centers f32[K,3], axes
    f32[K,9] (row-major R: its columns are the axes), half f32[K,3] -- over the cloud pc f32[N,3] and the rows of masks u8[K,N]"""
    dev = pc.device
    K, N = masks.shape
    counts = torch.empty((K, 3), dtype=I32, device=dev) if out is None else out
    call("cppf_box_support", dev, pc, masks, centers, axes, half, N, K, counts)
    return counts


def verify_boxes(poses, cfg, pad=None):
    """the boxes verify_proposals tests, f32[K,15] per proposal {centre T | axes R row-major | half extents scale / 2 + pad} (scale_3d
    on the zero-shot path; pad = cfg.res by default), computed in fp64 and rounded once.  A pose that is not finite gets half extents
    of -1: a box that holds no point."""
    pad = float(cfg.res) if pad is None else float(pad)
    boxes = np.zeros((len(poses), 15), np.float32)
    for k, p in enumerate(poses):
        row = np.concatenate([np.asarray(p["T"], np.float64).reshape(3), np.asarray(p["R"], np.float64).reshape(9),
                              np.asarray(p["scale_3d"] if "scale_3d" in p else p["scale"], np.float64).reshape(3) / 2 + pad])
        if np.all(np.isfinite(row)):
            boxes[k] = row
        else:
            boxes[k, 12:] = -1
    return boxes


def verify_ratios(counts):
    """one proposal's seven counts (VERIFY_COUNTS' order) -> the dict verify_proposals returns: the counts as ints and agreement =
    agree / within, leak = cross_agree / cross, fill = mask_in_box / mask_pts, purity = mask_in_box / box_pts in fp64, each 0.0 where
    its denominator is 0"""
    d = {name: int(v) for name, v in zip(VERIFY_COUNTS, counts)}
    for name, num, den in VERIFY_RATIOS:
        d[name] = d[num] / d[den] if d[den] else 0.0
    return d


def verify_proposals(pc, idx32, bits, masks, poses, cfg, pad=None):
    """Per-proposal evidence after the proposal stage: how far the pairs inside proposal k's point mask agree with
    centre k, and how far the mask and the pose's box cover each other.
    pc f32[N,3], idx32 i32[P,2], masks u8[K,N]: device tensors; bits: the survivor words of every group of <= 32 proposals, the list
    segment_proposals returns (a single tensor: one group); poses: the K pose dicts (T, R and scale, or scale_3d on the zero-shot
    path).  The box of proposal k has centre T, axes R's columns and half extents scale / 2 + pad (pad = cfg.res by default); a pose
    that is not finite gets mask_in_box = box_pts = 0.  Both kernels run per group, then ONE read-back of the two count tables.
    Returns one dict per proposal: the seven counts of VERIFY_COUNTS (int) and agreement, leak, fill, purity (fp64, verify_ratios)."""
    dev = pc.device
    K, P = len(poses), idx32.shape[0]
    if K == 0:
        return []
    if tuple(masks.shape) != (K, pc.shape[0]):
        raise ValueError(f"masks must be [{K}, {pc.shape[0]}] (one row per pose), got {tuple(masks.shape)}")
    bits = [bits] if isinstance(bits, torch.Tensor) else list(bits)
    group = proposal_group(P)
    if len(bits) != (K + group - 1) // group:
        raise ValueError(f"{len(bits)} survivor-word tensors for {K} proposals in groups of {group}")
    boxes = torch.from_numpy(verify_boxes(poses, cfg, pad)).to(dev)
    centers, axes, half = boxes[:, 0:3].contiguous(), boxes[:, 3:12].contiguous(), boxes[:, 12:15].contiguous()
    table = torch.empty(7 * K, dtype=I32, device=dev)
    sup, box = table[:4 * K].view(K, 4), table[4 * K:].view(K, 3)
    for i, g in enumerate(range(0, K, group)):
        e = min(g + group, K)
        proposal_support(idx32, bits[i], masks[g:e], out=sup[g:e])
        box_support(pc, masks[g:e], centers[g:e], axes[g:e], half[g:e], out=box[g:e])
    t = table.cpu().numpy()                                                   # the one read-back
    sup_h, box_h = t[:4 * K].reshape(K, 4), t[4 * K:].reshape(K, 3)
    return [verify_ratios(np.concatenate([sup_h[k], box_h[k]])) for k in range(K)]
