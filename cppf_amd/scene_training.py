"""Training on whole frames: the networks of train.py:34-35 fed the distribution the mask-free paths run them on.
training.train and train_on_meshes show the networks one object at a time; scene_poses / frame_detections then run them on a
whole-frame cloud whose SPRIN neighbourhoods cross object boundaries and whose pairs mostly join two different objects.  Here a step
is one rendered multi-object frame (mesh_frames.MeshFrameSampler):

  labelled_cloud       scene_stage.scene_cloud with the frame's label image: the clouds and the instance label of every point
  sample_scene_pairs   cppf_sample_scene_pairs: a stratified draw -- the first n_pos_pairs pairs join two points of ONE instance of
                       the target category, the rest are uniform over the cloud
  scene_pair_targets   cppf_scene_pair_targets: training.targets for every instance of a frame in one pass, in compact form (the
                       lower bin and its weight per head), positives / negatives marked
  scene_loss_fn        train.py:68-87 over the positives, straight from the compact form; optionally the negatives' nu head pulled to
                       the farthest bin
  train_on_frames      the loop around them, with train_on_meshes' optimiser and schedule

The bin head (2 tr_bins + 2 rot_bins + 5 wide) and the loss stay the reference's; the loss runs in torch."""
import numpy as np
import torch
import torch.nn.functional as F

from ._torch_util import call, canon, require_cuda
from .scene_stage import kept_positions, on_device, pairs_tensor, scene_cloud

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MAX_INSTANCES = 32                        # include/cppf.h: CPPF_SCENE_TRAIN_MAX_INSTANCES
FLAG_TARGET, FLAG_UP_SYM, FLAG_RIGHT_SYM = 1, 2, 4
HEADS = ("mu", "nu", "up", "right")       # the order of low / w_low's columns


def labelled_cloud(frame, cfg, jitter=None):
    """A MeshFrame's clouds with labels: scene_stage.scene_cloud(frame.depth_mm, frame.intrinsics, cfg, jitter, frame.labels), the
    SceneCloud (hi f32[N_hi,3], hi_nrm, hi_inst i32[N_hi], ind i64[N], pc f32[N,3], nrm, inst i32[N]) on the device; hi_inst is the
    label image read at each kept point's own pixel (-1 = background), inst = hi_inst[ind]."""
    return scene_cloud(frame.depth_mm, frame.intrinsics, cfg, jitter, labels=frame.labels)


def instance_table(centers, Rs, half_extents, is_target, cfg):
    """The instance table cppf_scene_pair_targets reads, on the host: (table f32[K,12] = {centre, up axis, right axis, scale target},
    flags i32[K]).  Rs: rotation matrices whose columns are the object's axes (up = column 1, right = column 2 with cfg.z_right, else
    column 0); the scale target log(half) - log(scale_mean) is computed in fp64; flags: bit 0 = is_target[k], bit 1 = cfg.up_sym, bit
    2 = cfg.right_sym."""
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    K = centers.shape[0]
    Rs, half = np.asarray(Rs, np.float64).reshape(K, 3, 3), np.asarray(half_extents, np.float64).reshape(K, 3)
    table = np.empty((K, 12), np.float64)
    table[:, 0:3] = centers
    table[:, 3:6] = Rs[:, :, 1]
    table[:, 6:9] = Rs[:, :, 2 if cfg.z_right else 0]
    table[:, 9:12] = np.log(half) - np.log(np.asarray(cfg.scale_mean, np.float64))[None]
    sym = (FLAG_UP_SYM if cfg.up_sym else 0) | (FLAG_RIGHT_SYM if getattr(cfg, "right_sym", False) else 0)
    flags = np.array([(FLAG_TARGET if t else 0) | sym for t in is_target], np.int32).reshape(K)
    return table.astype(np.float32), flags


def frame_table(frame, category, cfg):
    """instance_table of a MeshFrame's ground truth for the networks of `category`"""
    return instance_table(frame.centers, frame.Rs, frame.half_extents, [c == category for c in frame.categories], cfg)


def target_members(inst, flags):
    """(members i32[M], seg_off i32[K+1]) on inst's device: the points whose label is an instance with bit 0 of `flags` (host i32[K])
    set, grouped by instance, ascending within a group -- what the stratified draw takes"""
    dev = inst.device
    flags = np.asarray(flags, np.int32).reshape(-1)
    K = flags.shape[0]
    is_t = torch.from_numpy((flags & FLAG_TARGET) != 0).to(dev)
    lab = inst.long()
    ok = (lab >= 0) & (lab < K)
    ok &= is_t[lab.clamp(0, K - 1)]
    pts = torch.nonzero(ok).reshape(-1)
    order = torch.sort(lab[pts], stable=True)[1]
    counts = torch.bincount(lab[pts], minlength=K)[:K]
    seg_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)]).to(I32)
    return pts[order].to(I32).contiguous(), seg_off.contiguous()


def _i32(x, dev, name):
    """an integer table of the caller as i32 on `dev`: numpy / lists are uploaded, tensors converted where they are or refused"""
    if not isinstance(x, torch.Tensor):
        a = np.asarray(x)
        if a.dtype.kind not in "iu":
            raise TypeError(f"{name}: expected integers, got {a.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(dev)
    if x.dtype.is_floating_point or x.dtype == torch.bool:
        raise TypeError(f"{name}: expected an integer tensor, got {x.dtype}")
    return canon(x, I32, dev, name).reshape(-1)


def sample_scene_pairs(members, seg_off, inst, n_pairs, n_pos_pairs, seed):
    """cppf_sample_scene_pairs: idx i32[n_pairs,2] on inst's device.  members / seg_off: target_members' lists (integer tensors on
    the device or host arrays); inst i32[N]: the labelled cloud's labels.  Pairs [0, n_pos_pairs) join two points of one instance
    of the target category (uniform when there is none), the rest are uniform over the N points; a function of (seed, pair index)."""
    require_cuda()
    if not isinstance(inst, torch.Tensor) or not inst.is_cuda:
        raise ValueError(f"inst: expected a tensor on a HIP device, got {getattr(inst, 'device', type(inst).__name__)}")
    dev = inst.device
    inst, members, seg_off = _i32(inst, dev, "inst"), _i32(members, dev, "members"), _i32(seg_off, dev, "seg_off")
    P, P_pos, K = int(n_pairs), int(n_pos_pairs), seg_off.shape[0] - 1
    if K < 1 or not 0 <= P_pos <= P or inst.shape[0] < 1:
        raise ValueError(f"sample_scene_pairs: {K} instances, {inst.shape[0]} points, {P_pos} of {P} pairs in the positive stratum")
    idx = torch.empty((P, 2), dtype=I32, device=dev)
    call("cppf_sample_scene_pairs", dev, members if members.shape[0] else None, members.shape[0], seg_off, K, inst, inst.shape[0], P, P_pos, int(seed) & 0xFFFFFFFFFFFFFFFF, idx)
    return idx


def scene_pair_targets(pc, nrm, inst, idx, table, flags, cfg):
    """cppf_scene_pair_targets: dict(kind u8[P], pair_inst i32[P], low u8[P,4], w_low f32[P,4], aux u8[P,2]) on pc's device; heads in
    HEADS' order.  pc, nrm f32[N,3], inst [N] integers: device tensors; idx [P,2]: as PPFEncoder takes it; table [K,12] / flags [K]:
    instance_table's (host arrays or device tensors), K <= 32."""
    require_cuda()
    if not isinstance(pc, torch.Tensor) or not pc.is_cuda:
        raise ValueError(f"pc: expected a tensor on a HIP device, got {getattr(pc, 'device', type(pc).__name__)}")
    dev = pc.device
    pc, nrm = canon(pc, F32, dev, "pc", (3,)), canon(nrm, F32, dev, "nrm", (3,))
    inst = _i32(inst, dev, "inst")
    idx = pairs_tensor(idx, dev).to(I32).contiguous()
    table, flags = on_device(table, dev, "table", (12,)), _i32(flags, dev, "flags")
    N, P, K = pc.shape[0], idx.shape[0], flags.shape[0]
    if not 1 <= K <= MAX_INSTANCES:
        raise ValueError(f"scene_pair_targets takes 1..{MAX_INSTANCES} instances, got {K}")
    if tuple(table.shape) != (K, 12) or tuple(nrm.shape) != (N, 3) or inst.shape[0] != N or N < 1:
        raise ValueError(f"scene_pair_targets: pc {tuple(pc.shape)}, nrm {tuple(nrm.shape)}, inst {tuple(inst.shape)}, table "
                         f"{tuple(table.shape)}, flags {tuple(flags.shape)}: expected [N,3], [N,3], [N], [K,12], [K]")
    t = dict(kind=torch.empty(P, dtype=U8, device=dev), pair_inst=torch.empty(P, dtype=I32, device=dev),
             low=torch.empty((P, 4), dtype=U8, device=dev), w_low=torch.empty((P, 4), dtype=F32, device=dev),
             aux=torch.empty((P, 2), dtype=U8, device=dev))
    call("cppf_scene_pair_targets", dev, pc, nrm, inst, N, idx, P, table, flags, K, float(cfg.vote_range[0]), float(cfg.vote_range[1]),
         int(cfg.tr_num_bins), int(cfg.rot_num_bins), t["kind"], t["pair_inst"], t["low"], t["w_low"], t["aux"])
    return t


def dense_targets(t, cfg, table=None):
    """The compact targets expanded to training.targets' dense tensors, for checking: (tr f32[P,2,tr_bins], rot f32[P,2,rot_bins], aux
    f32[P,2], scale); scale = table[pair_inst][:, 9:12] (f32[P,3], row 0 for the negatives) when the instance table is given, else
    None.  Torch ops on the targets' device (the CPU works)."""
    low, w = t["low"].long(), t["w_low"]

    def expand(h, bins):
        out = torch.zeros((low.shape[0], bins), dtype=w.dtype, device=w.device)
        out.scatter_(-1, low[:, h, None], w[:, h, None])
        out.scatter_(-1, low[:, h, None] + 1, 1.0 - w[:, h, None])
        return out

    tb, rb = int(cfg.tr_num_bins), int(cfg.rot_num_bins)
    tr = torch.stack([expand(0, tb), expand(1, tb)], 1)
    rot = torch.stack([expand(2, rb), expand(3, rb)], 1)
    scale = None
    if table is not None:
        table = torch.as_tensor(table, dtype=w.dtype, device=w.device)
        scale = table[t["pair_inst"].long().clamp(min=0)][:, 9:12]
    return tr, rot, t["aux"].to(w.dtype), scale


def scene_loss_fn(preds, t, table, cfg, neg_weight=0.0):
    """train.py:68-87 over the POSITIVE pairs of the compact targets `t`, divided by their count (training.loss_fn's value when every
    pair is positive and of one instance).  preds [1,P,out_dim] or [P,out_dim]; table f32[K,12] on preds' device.
    A KL term is w log w + (1 - w) log(1 - w) - w logp[low] - (1 - w) logp[low + 1] from two gathers of log_softmax: no dense target
    is built.  The scale MSE is against each pair's own instance row.  The right head and the second aux term are gated by
    cfg.regress_right.  neg_weight > 0 adds neg_weight * KL(one-hot farthest bin || nu head), averaged over the NEGATIVE pairs (the
    same formula: their compact nu target is all weight on the last bin).  Pairs of kind 255 take no part.  No host synchronisation."""
    tb, rb = int(cfg.tr_num_bins), int(cfg.rot_num_bins)
    pr = preds.reshape(-1, preds.shape[-1])
    low, w = t["low"].long(), t["w_low"].to(pr.dtype)
    pos = (t["kind"] == 1).to(pr.dtype)
    n_pos = pos.sum().clamp(min=1.0)
    ent = torch.xlogy(w, w) + torch.xlogy(1.0 - w, 1.0 - w)

    def kl(h, logits):
        lp = F.log_softmax(logits, -1)
        l0 = low[:, h, None]
        return ent[:, h] - w[:, h] * lp.gather(-1, l0)[:, 0] - (1.0 - w[:, h]) * lp.gather(-1, l0 + 1)[:, 0]

    aux = t["aux"].to(pr.dtype)
    bce = lambda col, h: F.binary_cross_entropy_with_logits(pr[:, col], aux[:, h], reduction="none")
    over_pos = lambda term: (term * pos).sum() / n_pos
    kl_nu = kl(1, pr[:, tb:2 * tb])
    loss = over_pos(kl(0, pr[:, :tb])) + over_pos(kl_nu)
    loss = loss + over_pos(kl(2, pr[:, 2 * tb:2 * tb + rb]))
    loss = loss + over_pos(bce(-5, 0))
    scale = table.to(pr.dtype)[t["pair_inst"].long().clamp(min=0)][:, 9:12]
    loss = loss + over_pos(((pr[:, -3:] - scale) ** 2).sum(-1)) / 3.0
    if cfg.regress_right:
        loss = loss + over_pos(kl(3, pr[:, 2 * tb + rb:2 * tb + 2 * rb]))
        loss = loss + over_pos(bce(-4, 1))
    if neg_weight:
        neg = (t["kind"] == 0).to(pr.dtype)
        loss = loss + float(neg_weight) * (kl_nu * neg).sum() / neg.sum().clamp(min=1.0)
    return loss


def step_seed(seed, it):
    """the Philox key of step `it`'s pair draw"""
    return (int(seed) * 1000003 + int(it)) & 0x7FFFFFFFFFFFFFFF


def step_inputs(frame, category, cfg, n_pairs, pos_frac, seed, it):
    """What step `it` trains on besides the features: dict(hi, hi_nrm, ind, pc, nrm, inst, table, flags (device), idx i32[P',2] (the
    stratified draw behind the "indistinguishable" filter), targets (scene_pair_targets' dict for idx), n_members (points of the
    category's instances in the sparse cloud)).  A function of (frame, cfg, n_pairs, pos_frac, seed, it) alone."""
    hi, hi_nrm, _, ind, pc, nrm, inst = labelled_cloud(frame, cfg)
    table, flags = frame_table(frame, category, cfg)
    if flags.shape[0] > MAX_INSTANCES:
        raise ValueError(f"a frame of {flags.shape[0]} instances: the targets take at most {MAX_INSTANCES}")
    members, seg_off = target_members(inst, flags)
    idx = sample_scene_pairs(members, seg_off, inst, n_pairs, int(round(float(pos_frac) * int(n_pairs))), step_seed(seed, it))
    idx = idx[kept_positions(pc, nrm, idx)].contiguous()
    table_d, flags_d = torch.from_numpy(table).to(pc.device), torch.from_numpy(flags).to(pc.device)
    return dict(hi=hi, hi_nrm=hi_nrm, ind=ind, pc=pc, nrm=nrm, inst=inst, table=table_d, flags=flags_d, idx=idx,
                targets=scene_pair_targets(pc, nrm, inst, idx, table_d, flags_d, cfg), n_members=int(members.shape[0]))


def train_on_frames(category, sampler, dev, steps=400, n_pairs=200000, pos_frac=0.5, neg_weight=0.0, lr=2e-3, seed=0, encoders=None,
                    cfg=None, log=None):
    """train_on_meshes' optimiser and schedule fed by whole frames (sampler: a mesh_frames.MeshFrameSampler, or anything whose
    sample() returns MeshFrames).  A step: sampler.sample(); labelled_cloud; SPRIN on the DENSE cloud with gradients (its own kNN, as
    scene_stage.frame_inputs runs it), features of the sparse cloud's points; the stratified draw (pos_frac of the pairs in the
    positive stratum); the "indistinguishable" filter the scene paths apply; targets; the pair encoder; scene_loss_fn; Adam.
    A frame with no point of an instance of `category` in its sparse cloud is skipped and counted when neg_weight == 0 (there is
    nothing to learn from it); with neg_weight > 0 it trains on negatives alone.  Returns (point_encoder, ppf_encoder, losses (one per
    trained step; every 20th goes to `log`), skipped)."""
    from . import synthetic as syn
    from .training import new_encoders
    cfg = cfg or syn.CATEGORIES[category]
    penc, enc = encoders or new_encoders(cfg, dev, seed)
    penc.train()
    enc.train()
    opt = torch.optim.Adam([*penc.parameters(), *enc.parameters()], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, eta_min=lr * 0.05)
    losses, skipped = [], 0
    for it in range(steps):
        s = step_inputs(sampler.sample(), category, cfg, n_pairs, pos_frac, seed, it)
        if s["n_members"] == 0 and not neg_weight:
            skipped += 1
            continue
        opt.zero_grad()
        feat = penc(s["hi"][None], s["hi_nrm"][None])[0][s["ind"]]
        preds = enc(s["pc"][None], s["nrm"][None], feat[None], idxs=s["idx"])
        loss = scene_loss_fn(preds, s["targets"], s["table"], cfg, neg_weight)
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.item()))
        if log and (it % 20 == 0 or it == steps - 1):
            log(f"{category} step {it:4d} loss {losses[-1]:.4f} points {s['pc'].shape[0]} pairs {s['idx'].shape[0]}")
    penc.eval()
    enc.eval()
    return penc, enc, losses, skipped
