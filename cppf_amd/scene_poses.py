"""Mask-free scene poses with the networks this package trains (the 141-wide bin head of train.py): one cloud of a whole scene with
NO instance masks in, every object's pose and point mask out.  The scene half is the zero-shot notebook's (nocs/zero_shot.ipynb
cells 8-11: scene vote, smoothed-grid proposals, back-vote, "unsupervised instance segmentation"), the pose half is the instance
path's (nocs/inference.py:259-339 on the proposal's kept pairs):

  1  all-heads first pass over every pair               PPFEncoder.forward_decode (fp32 or bf16, as the encoder is set)
  2  scene vote, proposals                              scene_stage.vote_proposals; one read-back
  3  back-vote at every proposal, segmentation          scene_stage.segment_proposals (cppf_backvote_multi, cppf_segment_instances):
                                                        ONE pass over the pair list for all proposals (csrc/scene_multi.hip); the
                                                        K+1 list offsets are read back
  4  orientation votes, axis signs, scale per proposal  cppf_rot_sphere_count_dirs(_order), cppf_pose_sums on the proposal's list;
                                                        every proposal enqueued, then one read-back of all records and masks

The single-list entry points of step 4 take the list's address from the host, which is why the offsets of step 3 are read before
it (K + 1 integers; the same read decides whether the kept-pair buffer was large enough).  Steps 2 and 3 and scene_frame's
pre-processing are scene_stage.py's, shared with cppf_amd.zero_shot, which stays the path for the notebook's 9-wide regression head."""
import numpy as np
import torch

from . import _lib
from ._torch_util import call, canon, require_cuda, scratch, workspace
from .scene_stage import (MAX_CENTERS, backvote_multi, frame_cloud, frame_inputs, gather_instances, on_device, pairs_tensor,
                          segment_instances, segment_proposals, sphere_tables, verify_proposals, vote_proposals, voxel_owner)
from .zero_shot import check_loop_args

F32, I32 = torch.float32, torch.int32
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
    return check_loop_args(thresh, margin, max_proposals, max_iters)


def scene_poses(encoder, pc, nrm, feat, idx, u_tr, u_rot, cfg, *, angle_tol=1.5, max_rot_pairs=10000, rot_order=None, num_rots=72,
                sigma=1.0, thresh=50, margin=10, max_proposals=32, max_iters=None, min_contrib=12, outputs=None, heads=None, verify=False,
                keep_masks=False):
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
    scale_norm, RT f64[4,4], cnt (smoothed peak), diff, point_mask bool[N], n_pairs -- what inference.nocs_result reads.
    verify=True: every pose dict gains verify, scene_stage.verify_proposals' dict for that proposal (two more launches per group of 32
    proposals and one more read-back after the poses; everything else is computed and launched as without it).
    keep_masks=True: the dict gains point_masks, the device u8[K,N] rows segment_proposals wrote (what refine_poses gathers from);
    nothing else changes."""
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
    idx = pairs_tensor(idx, dev)
    idx32 = idx.to(I32).contiguous()
    P, N = idx.shape[0], pc.shape[0]
    if given:
        outputs = on_device(outputs, dev, "outputs", (2,))
        heads = on_device(heads, dev, "heads", (8,))
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
    out = dict(poses=[], outputs=outputs, heads=heads, grid=None,
               proposals=(np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)),
               surv_bits=torch.zeros(P, dtype=I32, device=dev), offsets=np.zeros(1, np.int64), pairs=torch.empty(0, dtype=I32, device=dev))
    if P == 0 or int(max_proposals) == 0:
        corners, dims = grid_shape(pc.cpu().numpy(), cfg.res)
        out.update(corner=corners[0], dims=dims)
        return out
    grid, corners, dims, corner, loc, val, diff, worlds = vote_proposals(pc, outputs, idx32, cfg, num_rots, sigma, thresh, margin,
                                                                         max_proposals, max_iters)                  # step 2
    K = loc.shape[0]
    out.update(grid=grid, corner=corners[0], dims=dims, proposals=(loc, val, diff))
    if K == 0:
        return out
    vws = workspace(256, dev, "vote")                                         # step 3 (the vote's rotation table, when it left one)
    masks, pairs, offsets, counts_d, bits = segment_proposals(pc, outputs, idx32, corner, cfg.res, dims, worlds, num_rots, None, min_contrib,
                                                              vote_ws=vws if vws.numel() >= 32768 else None)
    sph64, sph32_d, sph64_d, sorted_y = sphere_tables(angle_tol, dev)         # step 4
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
    if verify:
        for p, v in zip(out["poses"], verify_proposals(pc, idx32, bits, masks, out["poses"], cfg)):
            p["verify"] = v
    out.update(surv_bits=bits[0][:P], offsets=offsets, pairs=pairs[:int(offsets[K])])
    if keep_masks:
        out["point_masks"] = masks
    return out


REFINED_KEYS = ("T", "R", "up", "right", "scale", "scale_norm", "RT", "n_points", "peak", "argmax")


def refined_pose(rec, cfg, n_points):
    """one finished record of BatchPoseRunner (sharding.pack_record's layout: T, up, right, scale, arg-max, peak) -> a dict with the
    first pass's keys T, R, up, right (None unless cfg.regress_right), scale, scale_norm, RT, plus n_points, peak and argmax"""
    rec = np.asarray(rec, np.float64)
    T, up, right, scale = rec[0:3].copy(), rec[3:6].copy(), rec[6:9].copy(), rec[9:12].copy()
    R = np.stack([np.cross(up, right), up, right], -1) if cfg.z_right else np.stack([right, up, np.cross(right, up)], -1)
    scale_norm = float(np.linalg.norm(scale))
    RT = np.eye(4)
    RT[:3, :3] = R * scale_norm
    RT[:3, -1] = T
    return dict(T=T, R=R, up=up, right=right if cfg.regress_right else None, scale=scale, scale_norm=scale_norm, RT=RT,
                n_points=int(n_points), peak=float(rec[13]), argmax=int(rec[12]))


def refine_poses(out, runner, cfg, n_pairs=100_000, seed=0, min_points=None, owner=None):
    """Every proposal of a mask-free frame once more as an INSTANCE: its point mask (over the sparse cloud at 4 res) selects its
    points of the dense cloud (res) on the device -- scene_stage.gather_instances, one pass for all proposals -- and the packed clouds
    go through the instance path (SPRIN on the instance's own cloud, n_pairs pairs inside it, the whole pose) as ONE resident batch of
    `runner`, a BatchPoseRunner that holds the pair encoder and the point encoder of cfg.category.
    out: scene_frame's dict (hi_pc, hi_normals, indices, poses; point_masks, the device masks, when it was computed with
    keep_masks=True -- else the poses' host masks are uploaded again).  owner: scene_stage.voxel_owner(hi_pc, indices, 4 cfg.res) when
    the caller has it already (it depends on the cloud alone: categories that share a cloud share it).
    Sets, for every pose p of out["poses"], p["refined"] = dict(T, R, up, right, scale, scale_norm, RT, n_points, peak, argmax)
    (refined_pose), or p["refined"] = None with p["refine_skipped"] = "points" (fewer than min_points gathered points; default: the
    smallest cloud the point encoder takes, its k) or "refused" (the runner's mark record[:, 12] < 0: the instance did not fit the
    pipeline it ran on).  A refusal is settled here -- the runner's late check of THIS batch is taken and not raised; an earlier
    batch's still raises.  Object j of the batch is the j-th proposal that has enough points: its pairs are drawn from (seed, j).
    The first-pass fields of every pose stay as they were.  Returns the list of refined dicts / None, one per proposal."""
    from ._lib import CppfError
    poses = out["poses"]
    K = len(poses)
    if K == 0:
        return []
    cat = cfg.category
    if cat not in runner.encoders or cat not in runner.point_encoders:
        raise ValueError(f"refine_poses: the runner needs the pair encoder and the point encoder of {cat!r}")
    hi, hi_nrm = out["hi_pc"], out["hi_normals"]
    dev = hi.device
    min_points = int(runner.point_encoders[cat].k) if min_points is None else int(min_points)
    if owner is None:
        owner = voxel_owner(hi, out["indices"], 4 * cfg.res)
    masks = out.get("point_masks")
    if masks is None:
        masks = torch.from_numpy(np.ascontiguousarray(np.stack([p["point_mask"] for p in poses]).astype(np.uint8))).to(dev)
    clouds = []                                                               # (pts, nrm) row ranges of the packed buffers, per proposal
    for g in range(0, K, MAX_CENTERS):
        pts, nrm, _, off, _ = gather_instances(hi, hi_nrm, owner, masks[g:g + MAX_CENTERS])
        clouds += [(pts[int(a):int(b)], nrm[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]
    take = [k for k in range(K) if clouds[k][0].shape[0] >= max(min_points, 1)]
    refined = [None] * K
    for p in poses:
        p["refined"] = None
        p["refine_skipped"] = "points"
    if take:
        objs = runner.put([dict(pc=clouds[k][0], normals=clouds[k][1], cfg=cfg, n_pairs=int(n_pairs)) for k in take])
        recs = runner.run(objs, seed=seed)
        batch = runner._batch_no - 1
        recs = recs.cpu().numpy() if torch.is_tensor(recs) else np.asarray(recs)
        try:
            runner.check()
        except CppfError as e:
            if getattr(e, "batch", None) != batch:
                raise
        for j, k in enumerate(take):
            if recs[j, 12] < 0:
                poses[k]["refine_skipped"] = "refused"
                continue
            refined[k] = poses[k]["refined"] = refined_pose(recs[j], cfg, clouds[k][0].shape[0])
            del poses[k]["refine_skipped"]
    return refined


def scene_frame(depth, intrinsics, encoder, point_encoder, cfg, n_pairs=5_000_000, seed=0, jitter=None, cloud=None, refine=None,
                refine_kw=None, segments=None, intra_frac=1.0, **kw):
    """One depth frame with NO instance masks -> scene_poses' dict: scene_stage.frame_inputs (nocs/zero_shot.ipynb cells 3-6: the cloud
    de-duplicated at res, the sparse cloud at 4 res, SPRIN features on the dense cloud, frames.draw_pairs(seed, 0, ...) -- whose
    uniforms feed the bin decode -- and the "indistinguishable" pair filter), then scene_poses with the bin-head encoder.
    depth [H,W] in millimetres (numpy uint16 or device); jitter: f32[n_pixels,3] standard-normal draws (None: none); cloud: the
    SceneCloud frame_cloud (with segments=: segments.labelled_frame_cloud) returned for this depth, intrinsics, jitter and a config
    with the same (res, knn) (None: it is computed here: the same bits); kw: scene_poses' options.
    Adds hi_pc / hi_normals, indices, pc / normals, feat, idx, n_pairs (after the filter).
    refine (opt-in; None: nothing below runs and the dict has the keys and the bits it always had): a BatchPoseRunner with both
    encoders of cfg.category.  Every pose then gains `refined` (refine_poses: the proposal's dense points through the instance path)
    and the dict gains point_masks (device) and owner (scene_stage.voxel_owner's map of the dense cloud); refine_kw: refine_poses'
    options (n_pairs, seed -- default: this frame's seed --, min_points, owner).
    segments (opt-in; None: the uniform draw above, the same launches and the same bits as ever): segments.frame_segments' dict for
    this frame.  The pairs are then drawn INSIDE segments (segments.segment_inputs replaces frame_inputs: the same clouds, features
    and bin uniforms; the first round(intra_frac n_pairs) pairs join two points of one segment, the rest are uniform) and the dict
    gains segment_ids, the segment of every point of pc (-1: none).  A `cloud` without labels is then refused (ValueError)."""
    check_encoder(encoder, cfg)
    check_args(kw.get("max_proposals", 32), kw.get("thresh", 50), kw.get("margin", 10), kw.get("max_iters"))
    require_cuda()
    seg_ids = None
    if segments is None:
        hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot) = frame_inputs(depth, intrinsics, point_encoder, cfg, n_pairs, seed, jitter, cloud)
    else:
        from .segments import segment_inputs
        hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot), seg_ids = segment_inputs(depth, intrinsics, point_encoder, cfg, n_pairs, seed, segments,
                                                                                     intra_frac, jitter=jitter, cloud=cloud)
    if refine is not None:
        kw = dict(kw, keep_masks=True)
    out = scene_poses(encoder, pc, nrm, feat, idx, u_tr, u_rot, cfg, **kw)
    out.update(hi_pc=hi, hi_normals=hi_nrm, indices=ind, pc=pc, normals=nrm, feat=feat, idx=idx, n_pairs=int(idx.shape[0]))
    if seg_ids is not None:
        out["segment_ids"] = seg_ids
    if refine is not None:
        rkw = dict(refine_kw or {})
        rkw.setdefault("seed", seed)
        if rkw.get("owner") is None:
            rkw["owner"] = voxel_owner(hi, ind, 4 * cfg.res)
        out["owner"] = rkw["owner"]
        refine_poses(out, refine, cfg, **rkw)
    return out


__all__ = ["scene_poses", "scene_frame", "refine_poses", "refined_pose", "frame_cloud", "backvote_multi", "segment_instances", "check_encoder",
           "check_args"]
