"""Mask-free scene poses with the networks this package trains (the 141-wide bin head of train.py): one cloud of a whole scene with
NO instance masks in, every object's pose and point mask out.  The scene half is the zero-shot notebook's (nocs/zero_shot.ipynb
cells 8-11: scene vote, smoothed-grid proposals, back-vote, "unsupervised instance segmentation"), the pose half is the instance
path's (nocs/inference.py:259-339 on the proposal's kept pairs):

  1  all-heads first pass over every pair               PPFEncoder.forward_decode (fp32 or bf16, as the encoder is set)
  2  scene vote, proposals                              voting.vote_argmax, zero_shot.scene_proposals_device; one read-back
  3  back-vote at every proposal, segmentation          cppf_backvote_multi, cppf_segment_instances: ONE pass over the pair list for
                                                        all proposals (csrc/scene_multi.hip); the K+1 list offsets are read back
  4  orientation votes, axis signs, scale per proposal  cppf_rot_sphere_count_dirs(_order), cppf_pose_sums on the proposal's list;
                                                        every proposal enqueued, then one read-back of all records and masks

The single-list entry points of step 4 take the list's address from the host, which is why the offsets of step 3 are read before
it (K + 1 integers; the same read decides whether the kept-pair buffer was large enough).  cppf_amd.zero_shot stays the path for
the notebook's 9-wide regression head."""
import numpy as np
import torch

from . import _lib
from ._torch_util import call, canon, require_cuda, scratch, workspace
from .models import voting
from .utils.util import fibonacci_sphere, num_sphere_bins
from .zero_shot import _check_loop_args, _compact, _on_device, _pairs_tensor, scene_proposals_device

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MAX_CENTERS = 32                          # csrc/scene_multi.hip: BVM_MAX_CENTERS (one bit per proposal in a 32-bit word)
STD_PPFFCS = [84, 32, 32, 16]             # train.py:35


def check_encoder(encoder, cfg):
    """the standard architecture with the bin head: out_dim = 2 tr_bins + 2 rot_bins + 5 (train.py:35); anything else raises"""
    want = 2 * int(cfg.tr_num_bins) + 2 * int(cfg.rot_num_bins) + 5
    if list(getattr(encoder, "ppffcs", [])) != STD_PPFFCS or int(getattr(encoder, "out_dim", -1)) != want:
        raise ValueError(f"scene_poses needs the standard pair encoder (ppffcs {STD_PPFFCS}) with the bin head, out_dim = 2 tr_bins + "
                         f"2 rot_bins + 5 = {want}; got ppffcs {getattr(encoder, 'ppffcs', None)}, out_dim "
                         f"{getattr(encoder, 'out_dim', None)} (the 9-wide regression head runs through cppf_amd.zero_shot)")


def check_args(max_proposals, thresh=50, margin=10, max_iters=None):
    """the refusals that need no device"""
    if int(max_proposals) > MAX_CENTERS:
        raise ValueError(f"max_proposals must be <= {MAX_CENTERS} (one bit per proposal), got {max_proposals}")
    return _check_loop_args(thresh, margin, max_proposals, max_iters)


def _sphere_tables(angle_tol, dev):
    """the orientation bins of nocs/inference.py:100-102: (fp64 host, fp32 device, fp64 device, order of the y column for the banded
    count -- PoseWorkspace.sphere's rule)"""
    sph64 = np.array(fibonacci_sphere(num_sphere_bins(angle_tol)), np.float64)
    s32 = sph64.astype(np.float32)
    unit = bool(np.all(np.abs(np.linalg.norm(s32.astype(np.float64), axis=-1) - 1.0) < 1e-4))
    dy = np.diff(s32[:, 1])
    sorted_y = (1 if np.all(dy <= 0) else (-1 if np.all(dy >= 0) else 0)) if unit else 0
    return sph64, torch.from_numpy(s32).to(dev), torch.from_numpy(sph64).to(dev), sorted_y


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


def scene_poses(encoder, pc, nrm, feat, idx, u_tr, u_rot, cfg, *, angle_tol=1.5, max_rot_pairs=10000, rot_order=None, num_rots=72,
                sigma=1.0, thresh=50, margin=10, max_proposals=32, max_iters=None, min_contrib=12, outputs=None, heads=None):
    """The poses of every object of a scene cloud, with no instance masks.
    encoder: PPFEncoder with the standard architecture and the bin head (out_dim = 2 tr_bins + 2 rot_bins + 5), on pc's device, in
    the precision it is set to; pc, nrm f32[N,3], feat f32[N,F], idx [P,2], u_tr / u_rot f32[P,2] (uniforms standing in for
    torch.multinomial; negative = arg-max bin): device tensors.  outputs f32[P,2] AND heads f32[P,8] ({theta_up, theta_right, aux_up,
    aux_right, sx, sy, sz, 0}) given: they replace the first pass (encoder, feat, u_tr, u_rot may then be None).
    thresh / margin / sigma / max_proposals (<= 32) / max_iters: the proposal loop's (zero_shot.scene_proposals_device);
    min_contrib: the segmentation's; angle_tol / max_rot_pairs / rot_order / num_rots: estimate_pose's.
    Returns dict(poses, outputs, heads, grid (raw vote, device), corner f32[3], dims, proposals (loc i32[K,3], value, diff numpy),
    surv_bits (device i32[P], bit k = survivor at proposal k), offsets (numpy i64[K+1]), pairs (device i32: the kept lists));
    poses: one dict per proposal with T f64[3] (the proposal), R, up, right (None unless cfg.regress_right), scale f64[3],
    scale_norm, RT f64[4,4], cnt (smoothed peak), diff, point_mask bool[N], n_pairs -- what inference.nocs_result reads."""
    from .inference import _assemble, grid_shape
    max_iters = check_args(max_proposals, thresh, margin, max_iters)
    given = outputs is not None and heads is not None
    if (outputs is None) != (heads is None):
        raise ValueError("outputs= and heads= replace the first pass together: give both or neither")
    if not given:
        check_encoder(encoder, cfg)
    require_cuda()
    if not isinstance(pc, torch.Tensor) or not pc.is_cuda:
        raise ValueError(f"pc: expected a tensor on a HIP device, got {getattr(pc, 'device', type(pc).__name__)}")
    dev = pc.device
    pc, nrm = canon(pc, F32, dev, "pc", (3,)), canon(nrm, F32, dev, "nrm", (3,))
    idx = _pairs_tensor(idx, dev)
    idx32 = idx.to(I32).contiguous()
    P, N = idx.shape[0], pc.shape[0]
    if given:
        outputs = _on_device(outputs, dev, "outputs", (2,))
        heads = _on_device(heads, dev, "heads", (8,))
        if outputs.shape[0] != P or heads.shape[0] != P:
            raise ValueError(f"outputs / heads must have one row per pair ({P}), got {tuple(outputs.shape)} / {tuple(heads.shape)}")
    elif P:                                                                   # step 1
        feat = canon(feat, F32, dev, "feat")
        u_tr, u_rot = canon(u_tr, F32, dev, "u_tr", (P, 2)), canon(u_rot, F32, dev, "u_rot", (P, 2))
        with torch.no_grad():
            outputs, heads = encoder.forward_decode(pc, nrm, feat, idx, u_tr, cfg.vote_range, u_rot, cfg.tr_num_bins, cfg.rot_num_bins)
    else:
        outputs, heads = torch.empty((0, 2), dtype=F32, device=dev), torch.empty((0, 8), dtype=F32, device=dev)
    if N == 0:
        raise ValueError("the scene cloud is empty")
    corners, dims = grid_shape(pc.cpu().numpy(), cfg.res)                      # step 2
    corner = torch.from_numpy(corners[0].copy()).to(dev)
    out = dict(poses=[], outputs=outputs, heads=heads, grid=None, corner=corners[0], dims=dims,
               proposals=(np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)),
               surv_bits=torch.zeros(P, dtype=I32, device=dev), offsets=np.zeros(1, np.int64), pairs=torch.empty(0, dtype=I32, device=dev))
    if P == 0 or int(max_proposals) == 0:
        return out
    grid = torch.empty(dims, dtype=F32, device=dev)
    voting.vote_argmax(pc, outputs, None, idx32, grid, corner, cfg.res, num_rots, True, accumulate=False)
    loc, val, diff, count = scene_proposals_device(grid, sigma, thresh, margin, max_proposals, max_iters)
    K = int(count.item())                                                     # the read-back of the proposals
    loc, val, diff = loc[:K].cpu().numpy(), val[:K].cpu().numpy(), diff[:K].cpu().numpy()
    out.update(grid=grid, proposals=(loc, val, diff))
    if K == 0:
        return out
    worlds = corners[0].astype(np.float64)[None] + loc.astype(np.int64) * float(cfg.res)          # fp64, as zero_shot_scene
    centers = torch.from_numpy(np.ascontiguousarray(worlds.astype(np.float32))).to(dev)

    vws = workspace(256, dev, "vote")                                         # step 3 (the vote's rotation table, when it left one)
    bits = backvote_multi(pc, outputs, idx32, corner, cfg.res, dims, centers, num_rots, vote_ws=vws if vws.numel() >= 32768 else None)
    masks, pairs, offsets_d = segment_instances(idx32, bits, N, K, min_contrib)
    offsets = offsets_d.cpu().numpy().astype(np.int64)
    if offsets[K] > pairs.shape[0]:                                           # more kept (pair, proposal) items than pairs: once more
        masks, pairs, offsets_d = segment_instances(idx32, bits, N, K, min_contrib, capacity=int(offsets[K]))
    counts_d = (offsets_d[1:] - offsets_d[:-1]).contiguous()

    sph64, sph32_d, sph64_d, sorted_y = _sphere_tables(angle_tol, dev)        # step 4
    S = sph64.shape[0]
    thr = float(np.float32(np.cos(angle_tol / 180 * np.pi)))
    n_dirs = 2 if cfg.regress_right else 1
    if rot_order is not None:
        rot_order = torch.as_tensor(rot_order).to(device=dev, dtype=I32).contiguous()
    recs = torch.zeros((K, 21), dtype=torch.float64, device=dev)              # inference._assemble's record per proposal
    sph_counts = torch.zeros((K, 2, S), dtype=I32, device=dev)
    tickets = torch.zeros((K, 4), dtype=I32, device=dev)
    best_idx = torch.empty((K, 2), dtype=torch.int64, device=dev)
    pws = workspace(_lib.lib().cppf_pose_sums_workspace_bytes(), dev, "pose_sums")
    for k in range(K):
        n_k = int(offsets[k + 1] - offsets[k])
        sel = pairs[int(offsets[k]):int(offsets[k]) + n_k] if n_k else pairs[:1]      # (an empty list: any valid address)
        rec = recs[k]
        if rot_order is None:
            call("cppf_rot_sphere_count_dirs", dev, pc, heads, 8, 1, n_dirs, idx32, sel, counts_d[k:k + 1], n_k, int(max_rot_pairs),
                 int(num_rots), sph32_d, S, thr, sorted_y, sph_counts[k], S)
        else:
            call("cppf_rot_sphere_count_dirs_order", dev, pc, heads, 8, 1, n_dirs, idx32, sel, counts_d[k:k + 1], n_k, rot_order,
                 rot_order.numel(), int(max_rot_pairs), int(num_rots), sph32_d, S, thr, sorted_y, sph_counts[k], S)
        call("cppf_pose_sums", dev, pc, nrm, idx32, sel, counts_d[k:k + 1], n_k, heads.data_ptr() + 4 * 2, 8, n_dirs, sph_counts[k], S, S,
             sph64_d, heads.data_ptr() + 4 * 4, 8, best_idx[k], rec[3:9], rec[9:15], rec[15:19], scratch(pws), tickets[k])
    recs_h, masks_h = recs.cpu().numpy(), masks.cpu().numpy().astype(bool)    # the final read-back
    for k in range(K):
        recs_h[k, 0:3] = worlds[k]
        p = _assemble(recs_h[k], cfg)
        RT = np.eye(4)
        RT[:3, :3] = p["R"] * p["scale_norm"]
        RT[:3, -1] = p["T"]
        poses_k = dict(T=p["T"], R=p["R"], up=p["up"], right=p["right"] if cfg.regress_right else None, scale=p["scale"],
                       scale_norm=p["scale_norm"], RT=RT, cnt=float(val[k]), diff=float(diff[k]), point_mask=masks_h[k],
                       n_pairs=int(offsets[k + 1] - offsets[k]))
        out["poses"].append(poses_k)
    out.update(surv_bits=bits[:P], offsets=offsets, pairs=pairs[:int(offsets[K])])
    return out


def frame_cloud(depth, intrinsics, cfg, jitter=None):
    """the dense cloud of a whole frame and its normals, (hi f32[N,3], hi_nrm f32[N,3]) device tensors: frames.instance_cloud with
    every pixel in the mask.  A function of (depth, intrinsics, cfg.res, cfg.knn, jitter) alone, so categories whose configs agree in
    (res, knn) can share it (scene_frame's cloud=)."""
    from .frames import instance_cloud
    d = np.asarray(depth) if not isinstance(depth, torch.Tensor) else depth
    return instance_cloud(depth, intrinsics, np.ones(tuple(d.shape), bool), cfg, jitter)


def scene_frame(depth, intrinsics, encoder, point_encoder, cfg, n_pairs=5_000_000, seed=0, jitter=None, cloud=None, **kw):
    """One depth frame with NO instance masks -> scene_poses' dict: zero_shot_frame's pre-processing (nocs/zero_shot.ipynb cells 3-6:
    the cloud de-duplicated at res, the sparse cloud at 4 res, SPRIN features on the dense cloud, frames.draw_pairs(seed, 0, ...) --
    whose uniforms feed the bin decode -- and the "indistinguishable" pair filter), then scene_poses with the bin-head encoder.
    depth [H,W] in millimetres (numpy uint16 or device); jitter: f32[n_pixels,3] standard-normal draws (None: none); cloud: the
    (hi, hi_nrm) pair frame_cloud returned for this depth, intrinsics, jitter and a config with the same (res, knn) -- it replaces the
    back-projection, the de-duplication and the normals (None: they are computed here: the same bits); kw: scene_poses' options.
    Adds hi_pc / hi_normals, indices, pc / normals, feat, idx, n_pairs (after the filter)."""
    from .frames import draw_pairs
    from .utils.util import sparse_quantize
    check_encoder(encoder, cfg)
    check_args(kw.get("max_proposals", 32), kw.get("thresh", 50), kw.get("margin", 10), kw.get("max_iters"))
    require_cuda()
    hi, hi_nrm = frame_cloud(depth, intrinsics, cfg, jitter) if cloud is None else cloud
    if hi.shape[0] == 0:
        raise ValueError("the depth frame has no valid pixels")
    _, ind = sparse_quantize(hi, return_index=True, quantization_size=4 * cfg.res)
    pc, nrm = hi[ind].contiguous(), hi_nrm[ind].contiguous()
    with torch.no_grad():
        feat = point_encoder(hi[None], hi_nrm[None])[0][ind].contiguous()
    idx, u = draw_pairs(seed, 0, int(n_pairs), pc.device, pc.shape[0])
    # the filter keeps a subset in order: the uniforms of the kept pairs are found by running the draw's positions through it too
    keep_pos = _kept_positions(pc, nrm, idx)
    idx, u_tr, u_rot = idx[keep_pos].contiguous(), u[0][keep_pos].contiguous(), u[1][keep_pos].contiguous()
    out = scene_poses(encoder, pc, nrm, feat, idx, u_tr, u_rot, cfg, **kw)
    out.update(hi_pc=hi, hi_normals=hi_nrm, indices=ind, pc=pc, normals=nrm, feat=feat, idx=idx, n_pairs=int(idx.shape[0]))
    return out


def _kept_positions(pc, nrm, idx):
    """zero_shot.distinct_pairs as positions (i64, in order) instead of the pairs themselves"""
    dev = pc.device
    P = idx.shape[0]
    keep = torch.empty(max(P, 1), dtype=U8, device=dev)
    if P:
        call("cppf_pair_filter_distinct", dev, pc, nrm, idx, idx.dtype == torch.int64, pc.shape[0], P, keep)
    pos, _ = _compact(keep[:P], dev)
    return pos.long()


__all__ = ["scene_poses", "scene_frame", "frame_cloud", "backvote_multi", "segment_instances", "check_encoder", "check_args"]
