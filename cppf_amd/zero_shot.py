"""Zero-shot instance segmentation and pose estimation (the reference README's "Zero-Shot Instance Segmentation and Pose
Estimation", nocs/zero_shot.ipynb): one depth frame with NO instance masks in, every object's pose and point mask out.

  cell 3   whole-frame cloud, two-level de-duplication, SPRIN features   zero_shot_frame (scene_stage.frame_inputs)
  cell 5   5 M uniform pairs over the sparse cloud                       frames.draw_pairs (cppf_sample_pairs)
  cell 6   drop "indistinguishable" pairs                                distinct_pairs (cppf_pair_filter_distinct + compaction)
  cell 7-8 9-wide regression head, scene vote                            PPFEncoder.forward_with_idx, cppf_vote_argmax
  cell 9   Gaussian smoothing + iterative peak proposals                 smooth_grid / scene_proposals (cppf_scene_proposals)
  cell 11  back-vote, segmentation, orientation, axis sign, scale        segment_instance / zero_shot_poses

Cells 3-6, the vote with its proposals and cell 11's back-vote and segmentation (all proposals in one pass over the pair list, which
therefore holds fewer than 2^27 pairs) are scene_stage.py's, shared with the bin head's scene_poses.py.  The notebook does cells 9
and 11 in scipy / numpy on the host after copying the grid off the device; here everything runs on the device and the host reads
back the proposals (to size the per-proposal work), the K + 1 offsets of the proposals' kept-pair lists (the pose step takes each
list's address from the host) and at the end one small record and one point mask per proposal.  The
semantics where the notebook has none (thin grids, a peak on a last plane, a first diff equal to the threshold) are documented at
cppf_scene_proposals in include/cppf.h.  The notebook's "fine-grained centre vote" of cell 11 is computed and discarded there (T
stays the proposal); it is not run here."""
import numpy as np
import torch

from . import _lib
from ._torch_util import call, canon, require_cuda, scratch, workspace
from .scene_stage import (frame_inputs, kept_positions, on_device, pairs_tensor, segment_proposals, sphere_tables, verify_proposals,
                          vote_proposals)
from .utils.util import num_sphere_bins  # noqa: F401  (zero_shot.num_sphere_bins: the bins of the default angle_tol)

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MAX_RADIUS, MAX_MARGIN = 32, 64          # csrc/scene.hip: SCN_MAX_RADIUS, SCN_MAX_MARGIN


def gaussian_weights(sigma=1.0, truncate=4.0):
    """The 1-D kernel of scipy.ndimage.gaussian_filter (order 0): fp64 [2r+1], r = int(truncate * sigma + 0.5)"""
    sigma, truncate = float(sigma), float(truncate)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be a positive number, got {sigma}")
    if not (np.isfinite(truncate) and truncate >= 0):
        raise ValueError(f"truncate must be >= 0, got {truncate}")
    r = int(truncate * sigma + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"the filter radius int(truncate * sigma + 0.5) = {r} exceeds {MAX_RADIUS}")
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return np.ascontiguousarray(phi / phi.sum())


def _grid_tensor(grid):
    """numpy or torch f32[gx,gy,gz] -> (contiguous device tensor, whether numpy came in)"""
    require_cuda()
    was_np = isinstance(grid, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float32)) if was_np else grid
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"grid must be a 3-D array, got {getattr(t, 'shape', type(t).__name__)}")
    if t.dtype != F32:
        raise TypeError(f"grid must be float32, got {t.dtype}")
    if not t.is_cuda:
        t = t.cuda()
    return t.contiguous(), was_np


def smooth_grid(grid, sigma=1.0, truncate=4.0):
    """scipy.ndimage.gaussian_filter(grid, sigma) (cell 9), bit for bit, on the device.  numpy in -> numpy out."""
    g, was_np = _grid_tensor(grid)
    w = gaussian_weights(sigma, truncate)
    gx, gy, gz = g.shape
    out = torch.empty_like(g)
    ws = workspace(_lib.lib().cppf_gaussian_filter3d_workspace_bytes(gx, gy, gz), g.device, "gauss")
    call("cppf_gaussian_filter3d", g.device, g, out, gx, gy, gz, w, (w.shape[0] - 1) // 2, scratch(ws))
    return out.cpu().numpy() if was_np else out


def check_loop_args(thresh, margin, max_proposals, max_iters):
    if not 1 <= int(margin) <= MAX_MARGIN:
        raise ValueError(f"margin must be in 1..{MAX_MARGIN}, got {margin}")
    if int(max_proposals) < 0:
        raise ValueError(f"max_proposals must be >= 0, got {max_proposals}")
    max_iters = 4 * int(max_proposals) if max_iters is None else int(max_iters)
    if max_iters < 0:
        raise ValueError(f"max_iters must be >= 0, got {max_iters}")
    if not np.isfinite(float(thresh)):
        raise ValueError(f"thresh must be finite, got {thresh}")
    return max_iters


_check_loop_args = check_loop_args          # (the name it had while only this module used it)


def proposals_workspace(dims, device):
    """device scratch for scene_proposals_device on a grid of `dims` (allocate it before a graph capture)"""
    return torch.empty(max(int(_lib.lib().cppf_scene_proposals_workspace_bytes(*[int(d) for d in dims])), 256), dtype=U8,
                       device=device)


def scene_proposals_device(grid, sigma=1.0, thresh=50, margin=10, max_proposals=32, max_iters=None, truncate=4.0,
                           smoothed_out=None, out=None, ws=None):
    """Cell 9 on a device grid with no host round trip (graph-capturable): the raw scene vote in, the device tensors
    (loc i32[K,3], value f32[K], diff f32[K], count i32[1]) out, K = max_proposals; rows >= count are unspecified.
    smoothed_out: optional device f32 grid that receives the smoothed grid (before any suppression); out: a previous result
    tuple to write into; ws: proposals_workspace(dims) (a fresh one otherwise)."""
    g, _ = _grid_tensor(grid)
    max_iters = check_loop_args(thresh, margin, max_proposals, max_iters)
    w = gaussian_weights(sigma, truncate)
    dev, (gx, gy, gz) = g.device, g.shape
    K = int(max_proposals)
    if out is None:
        out = (torch.empty((max(K, 1), 3), dtype=I32, device=dev), torch.empty(max(K, 1), dtype=F32, device=dev),
               torch.empty(max(K, 1), dtype=F32, device=dev), torch.empty(1, dtype=I32, device=dev))
    loc, val, diff, count = out
    if smoothed_out is not None and (tuple(smoothed_out.shape) != tuple(g.shape) or smoothed_out.dtype != F32
                                     or not smoothed_out.is_contiguous()):
        raise ValueError("smoothed_out must be a contiguous float32 tensor shaped like the grid")
    if ws is None:
        ws = proposals_workspace(g.shape, dev)
    call("cppf_scene_proposals", dev, g, gx, gy, gz, w, (w.shape[0] - 1) // 2, float(np.float32(thresh)), int(margin), K, max_iters,
         loc, val, diff, count, smoothed_out, scratch(ws))
    return loc, val, diff, count


def scene_proposals(grid, corner, res, sigma=1, thresh=50, margin=10, max_proposals=32, max_iters=None, truncate=4.0):
    """The notebook's `scene_locs` (cell 9): a list of (world f64[3], cnt = smoothed peak f32, diff f32), world =
    corners[0] + loc * res in fp64 from the float32 corner."""
    loc, val, diff, count = scene_proposals_device(grid, sigma, thresh, margin, max_proposals, max_iters, truncate)
    n = int(count.item())
    loc, val, diff = loc[:n].cpu().numpy(), val[:n].cpu().numpy(), diff[:n].cpu().numpy()
    c = np.asarray(corner, np.float32).astype(np.float64)
    return [(c + loc[k].astype(np.int64) * float(res), val[k], diff[k]) for k in range(n)]


def distinct_pairs(pc, nrm, idx):
    """Cell 6: the pairs of `idx` that are not "indistinguishable", in their order (same dtype as idx, on pc's device)."""
    require_cuda()
    dev = pc.device
    pc, nrm = canon(pc, F32, dev, "pc", (3,)), canon(nrm, F32, dev, "nrm", (3,))
    idx = pairs_tensor(idx, dev)
    return idx[kept_positions(pc, nrm, idx)]


def segment_instance(pc, outputs, idx, center, corner, res, dims, num_rots=72, tol=None, min_contrib=12):
    """Cell 11's back-vote and "unsupervised instance segmentation" for one proposal centre: the survivors of the back-vote at
    `center` (tol = 3 res by default), the points that are endpoints of more than `min_contrib` of them, and the survivors with an
    endpoint among those points.  outputs: [P,2+] device (columns 0-1 = (mu, nu)); corner / dims: the scene grid's.
    Returns dict(point_mask bool[N] device, pairs i64[M] device = positions in idx, n_pairs M)."""
    require_cuda()
    dev = pc.device
    pc = canon(pc, F32, dev, "pc", (3,))
    idx32 = pairs_tensor(idx, dev).to(I32).contiguous()
    outputs = on_device(outputs, dev, "outputs")[:, :2].contiguous()
    corner = on_device(corner, dev, "corner")
    masks, pairs, offsets, _, _ = segment_proposals(pc, outputs, idx32, corner, res, dims, [center], num_rots, tol, min_contrib)
    n = int(offsets[1])
    return dict(point_mask=masks[0].bool(), pairs=pairs[:n].long(), n_pairs=n)


def zero_shot_poses(encoder9, pc, nrm, feat, idx, cfg, angle_tol=2, max_rot_pairs=10000, rot_order=None, preds=None, num_rots=72,
                    sigma=1.0, thresh=50, margin=10, max_proposals=32, max_iters=None, min_contrib=12, verify=False):
    """Cells 7-11 on a scene: the 9-wide regression head (out_dim = 2+2+2+3: mu nu | up right | aux up, aux right | log-scales)
    on every pair, the scene vote, the proposals, then per proposal the back-vote, the segmentation, the orientation vote on
    column 2 of the kept pairs (the first `max_rot_pairs`, or the positions `rot_order` in their list), the axis sign from column
    4, right = (0, -up_z, up_y) and scale_3d = mean(exp(columns 6..8)) scale_mean 2.
    pc, nrm f32[N,3], feat f32[N,F], idx [P,2] device tensors; preds: precomputed [P,9] head outputs (then encoder9 is unused).
    Returns one dict per proposal: T (the proposal, f64[3]), R f64[3,3], up, scale_3d f64[3], scale (its norm), RT f64[4,4],
    cnt (smoothed peak), diff, point_mask bool[N] (numpy), n_pairs (kept pairs).  zero_shot_scene also returns the grid and
    the proposals.  verify=True: every dict gains verify, scene_stage.verify_proposals' dict (the box: T, R, scale_3d / 2 + res)."""
    return zero_shot_scene(encoder9, pc, nrm, feat, idx, cfg, angle_tol, max_rot_pairs, rot_order, preds, num_rots, sigma, thresh,
                           margin, max_proposals, max_iters, min_contrib, verify)["poses"]


def zero_shot_scene(encoder9, pc, nrm, feat, idx, cfg, angle_tol=2, max_rot_pairs=10000, rot_order=None, preds=None, num_rots=72,
                    sigma=1.0, thresh=50, margin=10, max_proposals=32, max_iters=None, min_contrib=12, verify=False):
    """zero_shot_poses with the intermediate results: dict(poses, preds [P,9] device, grid (raw vote, device), corner f32[3],
    dims, proposals (loc i32[K,3], value, diff numpy))"""
    require_cuda()
    dev = pc.device
    pc, nrm = canon(pc, F32, dev, "pc", (3,)), canon(nrm, F32, dev, "nrm", (3,))     # (detached: the host copy below is of a leaf too)
    idx = pairs_tensor(idx, dev)
    idx32 = idx.to(I32).contiguous()
    P = idx.shape[0]
    if preds is None:
        if encoder9.out_dim != 9:
            raise ValueError(f"the zero-shot path needs the 9-wide regression head, the encoder has out_dim {encoder9.out_dim}")
        with torch.no_grad():
            preds = encoder9.forward_with_idx(pc, nrm, feat, idx)                             # cell 7
    preds = on_device(preds, dev, "preds")
    if tuple(preds.shape) != (P, 9):
        raise ValueError(f"preds must be [{P}, 9], got {tuple(preds.shape)}")
    outputs = preds[:, :2].contiguous()
    grid, corners, dims, corner, loc, val, diff, worlds = vote_proposals(pc, outputs, idx32, cfg, num_rots, sigma, thresh, margin,
                                                                         max_proposals, max_iters)                  # cells 8-9
    # cell 11: all proposals segmented at once, then each one's pose step (its buffers first: after the offsets read the device waits)
    n = worlds.shape[0]
    sph64, sph32_d, sph64_d, sorted_y = sphere_tables(angle_tol, dev)
    S = sph64.shape[0]
    thr = float(np.float32(np.cos(angle_tol / 180 * np.pi)))
    if rot_order is not None:
        rot_order = torch.as_tensor(rot_order).to(device=dev, dtype=I32).contiguous()
    rws = workspace(_lib.lib().cppf_reduce_workspace_bytes(), dev, "zs_reduce")
    recs = torch.zeros((n, 10), dtype=torch.float64, device=dev)        # best_dir[3] | sign sums[3] | exp-scale sums[4]
    counts = torch.zeros((n, S), dtype=I32, device=dev)
    best_idx = torch.empty(n, dtype=torch.int64, device=dev)
    masks, pairs, offsets, counts_d, bits = segment_proposals(pc, outputs, idx32, corner, cfg.res, dims, worlds, num_rots, None, min_contrib)
    rot = preds.data_ptr() + 4 * 2
    for k in range(n):
        sel = pairs[int(offsets[k]):int(offsets[k + 1])] if offsets[k + 1] > offsets[k] else pairs[:1]    # (empty: any valid address)
        cnt, rec = counts_d[k:k + 1], recs[k]
        if rot_order is None:
            call("cppf_rot_sphere_count", dev, pc, rot, 9, idx32, sel, cnt, P, int(max_rot_pairs), int(num_rots), sph32_d, S, thr,
                 sorted_y, counts[k])
        else:
            call("cppf_rot_sphere_count_dirs_order", dev, pc, rot, 9, 1, 1, idx32, sel, cnt, P, rot_order, rot_order.numel(),
                 int(max_rot_pairs), int(num_rots), sph32_d, S, thr, sorted_y, counts[k], S)
        call("cppf_counts_argmax_select", dev, counts[k], S, sph64_d, best_idx[k:k + 1], rec[0:3])
        call("cppf_axis_sign", dev, pc, nrm, idx32, sel, cnt, P, preds.data_ptr() + 4 * 4, 9, rec[0:3], rec[3:6], scratch(rws))
        call("cppf_scale_exp_sum", dev, preds.data_ptr() + 4 * 6, 9, sel, cnt, P, rec[6:10], scratch(rws))
    recs_h, masks_h = recs.cpu().numpy(), masks.cpu().numpy().astype(bool)
    poses = [_assemble(recs_h[k], worlds[k], cfg, val[k], diff[k], masks_h[k]) for k in range(n)]
    if verify:
        for p, v in zip(poses, verify_proposals(pc, idx32, bits, masks, poses, cfg)):
            p["verify"] = v
    return dict(poses=poses, preds=preds, grid=grid, corner=corners[0], dims=dims, proposals=(loc, val, diff))


def _assemble(rec, T, cfg, cnt, diff, point_mask):
    """host end of cell 11 from one proposal's record"""
    best = rec[0:3].copy()
    n_sign = max(rec[5], 1.0)
    up = -best if rec[4] / n_sign < rec[3] / n_sign else best                   # down_loss < up_loss
    right = np.array([0, -up[2], up[1]])
    right = right / np.linalg.norm(right)
    R = np.stack([right, up, np.cross(right, up)], -1)
    n = int(rec[9])
    scale_3d = rec[6:9] / max(n, 1) * np.asarray(cfg.scale_mean, np.float64) * 2
    scale = float(np.linalg.norm(scale_3d))
    RT = np.eye(4)
    RT[:3, :3] = R * scale
    RT[:3, -1] = T
    return dict(T=np.asarray(T, np.float64), R=R, up=up, scale_3d=scale_3d, scale=scale, RT=RT, cnt=float(cnt), diff=float(diff),
                point_mask=point_mask, n_pairs=n)


def zero_shot_frame(depth, intrinsics, encoder9, point_encoder, cfg, n_pairs=5_000_000, seed=0, jitter=None, **kw):
    """Cells 3-11 end to end on the device: depth [H,W] (millimetres, numpy uint16 or device) with no instance masks ->
    dict(poses (zero_shot_poses' list), hi_pc / hi_normals (the cloud de-duplicated at res), indices (its de-duplication at
    4 res), pc / normals (the sparse cloud), n_pairs (after the cell 6 filter), and zero_shot_scene's other entries).
    jitter: f32[n_pixels,3] standard-normal draws for cell 3's augmentation (None: none).  Pairs: frames.draw_pairs(seed, 0, ...)
    (the notebook's np.random.randint).  kw: zero_shot_poses' options."""
    require_cuda()
    hi, hi_nrm, ind, pc, nrm, feat, idx, _ = frame_inputs(depth, intrinsics, point_encoder, cfg, n_pairs, seed, jitter)    # cells 3-6
    out = zero_shot_scene(encoder9, pc, nrm, feat, idx, cfg, **kw)
    out.update(hi_pc=hi, hi_normals=hi_nrm, indices=ind, pc=pc, normals=nrm, feat=feat, idx=idx, n_pairs=int(idx.shape[0]))
    return out
