"""numpy restatement of csrc/scene_train.hip (include/cppf.h "Scene training") and the scenes its tests share.
- draw_ref: the stratified pair draw, bit for bit (cppf_amd.synthetic's host Philox, stream 4);
- targets_ref: the per-pair targets of many instances in fp64 -- training.targets' arithmetic per instance, the compact bin form,
  positives / negatives / out-of-range pairs -- with the quantities a test needs to set hard pairs aside;
- dense_ref: the compact form expanded to real2prob's two-bin distributions;
- posed_scene: posed analytic objects (synthetic.make_posed_object) about 1 m from the origin with background points, as one
  labelled cloud with its instance table."""
import numpy as np

from cppf_amd import synthetic as syn
from cppf_amd.config import CATEGORIES

STREAM = 4
_s32 = np.uint64(32)


def draw_ref(members, seg_off, inst, n_points, n_pairs, n_pos_pairs, seed):
    """cppf_sample_scene_pairs on well-formed lists: idx i32[n_pairs,2]"""
    members, seg_off, inst = (np.asarray(x, np.int64) for x in (members, seg_off, inst))
    p = np.arange(int(n_pairs), dtype=np.uint64)
    w = syn.philox4x32_10([p, np.zeros_like(p), np.full_like(p, STREAM), np.zeros_like(p)], seed)
    N, M = np.uint64(int(n_points)), int(seg_off[-1])
    a = ((w[0] * N) >> _s32).astype(np.int64)
    b = ((w[1] * N) >> _s32).astype(np.int64)
    n_pos = int(n_pos_pairs) if M > 0 else 0
    if n_pos:
        am = members[((w[0][:n_pos] * np.uint64(M)) >> _s32).astype(np.int64)]
        k = inst[am]
        s0, L = seg_off[k], seg_off[k + 1] - seg_off[k]
        a[:n_pos] = am
        b[:n_pos] = members[s0 + ((w[1][:n_pos] * L.astype(np.uint64)) >> _s32).astype(np.int64)]
    return np.stack([a, b], -1).astype(np.int32)


def draw_ref_lenient(members, members_cap, seg_off, inst, n_points, n_pairs, n_pos_pairs, seed):
    """cppf_sample_scene_pairs on lists that need not keep their promises: (idx i32[n_pairs,2], kept bool[n_pairs]: the pairs of the
    positive stratum that keep the UNIFORM draw because a lookup failed one of st_draw_kernel's guards).  members: the entries the
    list claims (at least seg_off[K] of them where that does not pass members_cap); the guards, in the kernel's order: 0 < M =
    seg_off[K] <= members_cap; the member drawn for a lies in [0, n_points); its label k lies in [0, K); 0 <= seg_off[k] < seg_off[k+1]
    <= M.  b is whatever the list holds at the drawn position: it is not looked at."""
    members, seg_off, inst = (np.asarray(x, np.int64) for x in (members, seg_off, inst))
    K = seg_off.shape[0] - 1
    p = np.arange(int(n_pairs), dtype=np.uint64)
    w = syn.philox4x32_10([p, np.zeros_like(p), np.full_like(p, STREAM), np.zeros_like(p)], seed)
    N, M = np.uint64(int(n_points)), int(seg_off[K])
    a = ((w[0] * N) >> _s32).astype(np.int64)
    b = ((w[1] * N) >> _s32).astype(np.int64)
    kept = np.zeros(int(n_pairs), bool)
    n_pos = int(n_pos_pairs)
    if n_pos and not (0 < M <= int(members_cap)):
        kept[:n_pos] = True
    elif n_pos:
        am = members[((w[0][:n_pos] * np.uint64(M)) >> _s32).astype(np.int64)]
        ok = (am >= 0) & (am < int(n_points))
        k = np.where(ok, inst[np.where(ok, am, 0)], -1)
        ok &= (k >= 0) & (k < K)
        kc = np.where(ok, k, 0)
        s0, s1 = seg_off[kc], seg_off[kc + 1]
        ok &= (s0 >= 0) & (s1 > s0) & (s1 <= M)
        L = np.where(ok, s1 - s0, 1).astype(np.uint64)
        pos = np.where(ok, s0, 0) + ((w[1][:n_pos] * L) >> _s32).astype(np.int64)
        a[:n_pos] = np.where(ok, am, a[:n_pos])
        b[:n_pos] = np.where(ok, members[pos], b[:n_pos])
        kept[:n_pos] = ~ok
    return np.stack([a, b], -1).astype(np.int32), kept


def members_ref(inst, flags):
    """(members, seg_off) of the instances with bit 0 of flags set: grouped by instance, ascending within a group"""
    inst, flags = np.asarray(inst), np.asarray(flags)
    groups = [np.nonzero(inst == k)[0] if flags[k] & 1 else np.zeros(0, np.int64) for k in range(flags.shape[0])]
    return (np.concatenate(groups).astype(np.int32) if groups else np.zeros(0, np.int32),
            np.concatenate([[0], np.cumsum([g.shape[0] for g in groups])]).astype(np.int32))


def _bin(v, interval, bins):
    x = v / interval
    low = np.minimum(np.floor(x), bins - 2)
    return low.astype(np.int64), 1.0 - (x - low)


def targets_ref(pc, nrm, inst, idx, table, flags, vote_range, tr_bins, rot_bins, dtype=np.float64):
    """cppf_scene_pair_targets in fp64 (the inputs are the float32 values the device reads; dtype=np.float32: every operation in fp32
    with the kernel's constants -- for scenes of exact coordinates, where |a - b| + 1e-7 must round as it does on the device).  dict: kind u8[P], pair_inst i32[P], low
    i64[P,4], w_low f64[P,4], aux u8[P,2] as the kernel writes them, and for the positives (0 elsewhere) d_len = |a - b|, cos f64[P,2] =
    (u.up, u.right), aux_margin f64[P,2] = (|n.up|, |n.right|)."""
    pc, nrm, table = np.asarray(pc, dtype), np.asarray(nrm, dtype), np.asarray(table, dtype)
    inst, idx, flags = np.asarray(inst, np.int64), np.asarray(idx, np.int64), np.asarray(flags, np.int64)
    N, P, K = pc.shape[0], idx.shape[0], flags.shape[0]
    v0, v1 = float(vote_range[0]), float(vote_range[1])
    kind = np.zeros(P, np.uint8)
    pair_inst = np.full(P, -1, np.int32)
    low = np.tile(np.array([0, tr_bins - 2, 0, 0], np.int64), (P, 1))
    w_low = np.tile(np.array([1.0, 0.0, 1.0, 1.0]), (P, 1))
    aux = np.zeros((P, 2), np.uint8)
    d_len, cos, margin = np.zeros(P), np.zeros((P, 2)), np.zeros((P, 2))
    inside = ((idx >= 0) & (idx < N)).all(-1)
    kind[~inside] = 255
    ia, ib = np.where(inside, idx[:, 0], 0), np.where(inside, idx[:, 1], 0)
    k = inst[ia]
    kc = np.clip(k, 0, K - 1)
    pos = inside & (k >= 0) & (k < K) & (inst[ib] == k) & ((flags[kc] & 1) != 0)
    q = np.nonzero(pos)[0]
    # (a coordinate that is not finite makes a quantity below NaN / inf; such a pair is set aside by `fin`: kind 0, the fill values)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if q.size:
            r = table[kc[q]]
            c, up, right = r[:, 0:3], r[:, 3:6], r[:, 6:9]
            a, b = pc[ia[q]] - c, pc[ib[q]] - c
            d = a - b
            L = np.linalg.norm(d, axis=-1)
            u = d / (L[:, None] + dtype(1e-7))
            proj = (a * u).sum(-1)
            dist2o = np.linalg.norm(a - proj[:, None] * u, axis=-1)
            cu, cr = (u * up).sum(-1), (u * right).sum(-1)
            th_up = np.arccos(np.clip(cu, -1, 1))
            th_up = np.where(flags[kc[q]] & 2, np.minimum(th_up, np.arccos(np.clip(-cu, -1, 1))), th_up)
            th_r = np.arccos(np.clip(cr, -1, 1))
            th_r = np.where(flags[kc[q]] & 4, np.minimum(th_r, np.arccos(np.clip(-cr, -1, 1))), th_r)
            n = nrm[ia[q]].copy()
            n[(n * u).sum(-1) < 0] *= -1
            n_up, n_r = (n * up).sum(-1), (n * right).sum(-1)
            vals = [np.clip(proj + dtype(v0), 0, dtype(2 * v0)), np.clip(dist2o, 0, dtype(v1)), th_up, th_r]
            spans = [(2 * v0, tr_bins), (v1, tr_bins), (np.pi, rot_bins), (np.pi, rot_bins)]
            fin = np.isfinite(proj) & np.isfinite(dist2o) & np.isfinite(cu) & np.isfinite(cr) & np.isfinite(n_up) & np.isfinite(n_r)
            q, sel = q[fin], fin
            for h, (v, (mx, bins)) in enumerate(zip(vals, spans)):
                low[q, h], w_low[q, h] = _bin(v[sel], dtype(mx / (bins - 1)), bins)       # (the width: fp64, then rounded once)
            aux[q, 0], aux[q, 1] = n_up[sel] > 0, n_r[sel] > 0
            kind[q], pair_inst[q] = 1, kc[q]
            d_len[q], cos[q, 0], cos[q, 1] = L[sel], cu[sel], cr[sel]
            margin[q, 0], margin[q, 1] = np.abs(n_up[sel]), np.abs(n_r[sel])
    return dict(kind=kind, pair_inst=pair_inst, low=low, w_low=w_low, aux=aux, d_len=d_len, cos=cos, aux_margin=margin)


def dense_ref(low, w_low, bins):
    """[P] lower bins and weights -> f64[P,bins]: w_low on bin low, 1 - w_low on bin low + 1"""
    low, w_low = np.asarray(low, np.int64), np.asarray(w_low, np.float64)
    out = np.zeros((low.shape[0], bins))
    r = np.arange(low.shape[0])
    out[r, low] = w_low
    out[r, low + 1] = 1.0 - w_low
    return out


def dense_all(t, tr_bins, rot_bins):
    """a targets dict (numpy) -> (tr f64[P,2,tr_bins], rot f64[P,2,rot_bins])"""
    low, w = np.asarray(t["low"], np.int64), np.asarray(t["w_low"], np.float64)
    return (np.stack([dense_ref(low[:, 0], w[:, 0], tr_bins), dense_ref(low[:, 1], w[:, 1], tr_bins)], 1),
            np.stack([dense_ref(low[:, 2], w[:, 2], rot_bins), dense_ref(low[:, 3], w[:, 3], rot_bins)], 1))


def hard_pairs(t, res):
    """bool[P]: positives whose angle targets are ill-conditioned -- the two points closer than res (u is a quotient of two small
    numbers) or u within acos(0.999) of an axis (acos' slope is above 22 there)"""
    return (t["kind"] == 1) & ((t["d_len"] < res) | (np.abs(t["cos"]) > 0.999).any(-1))


def table_of(obs, is_target, cfg):
    """cppf_amd.scene_training.instance_table of make_posed_object dicts"""
    from cppf_amd.scene_training import instance_table
    return instance_table([o["center"] for o in obs], [o["R"] for o in obs], [o["half_extents"] for o in obs], is_target, cfg)


def posed_scene(categories, cfg_category, n_points, seed, n_background=0, shift=(0.25, -0.2, 0.3), up_sym=None, normal_noise=0.02):
    """Posed analytic objects of `categories` 0.3 m apart and about 1 m from the origin, then n_background points of a far plane, as ONE
    labelled cloud in shuffled order.  Targets are those of cfg_category's networks: instance k is of the target category when
    categories[k] == cfg_category.  up_sym: override of the config's flag.  normal_noise: the analytic normals are turned by Gaussian noise of
    that size and renormalised, as fitted normals are (an analytic side normal is EXACTLY perpendicular to the axis, which leaves the sign
    targets to the last bit of a sum).  -> dict(cfg, obs, pc f32[N,3], nrm f32[N,3], inst
    i32[N] (-1 = background), table f32[K,12], flags i32[K])"""
    import dataclasses
    cfg = CATEGORIES[cfg_category]
    if up_sym is not None:
        cfg = dataclasses.replace(cfg, up_sym=bool(up_sym))
    rng = np.random.default_rng(seed)
    n_each = int(n_points) // len(categories)
    obs, pcs, nrms, labs = [], [], [], []
    for k, cat in enumerate(categories):
        ob = syn.make_posed_object(cat, n_each, seed * 10 + k)
        c = np.array([0.3 * k, 0.05 * (k % 2), 0.8 + 0.1 * k]) + np.asarray(shift)
        ob["pc"] = (ob["pc"].astype(np.float64) - ob["center"] + c).astype(np.float32)
        ob["center"] = c
        obs.append(ob)
        pcs.append(ob["pc"]), nrms.append(ob["normals"]), labs.append(np.full(n_each, k, np.int32))
    if n_background:
        bg = np.stack([rng.uniform(-0.3, 1.0, n_background), rng.uniform(-0.4, 0.4, n_background), np.full(n_background, 1.6)], -1)
        pcs.append(bg.astype(np.float32)), nrms.append(np.tile(np.array([0, 0, -1], np.float32), (n_background, 1)))
        labs.append(np.full(n_background, -1, np.int32))
    pc, nrm, inst = np.concatenate(pcs), np.concatenate(nrms).astype(np.float64), np.concatenate(labs)
    if normal_noise:
        nrm = nrm + normal_noise * rng.standard_normal(nrm.shape)
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm = nrm.astype(np.float32)
    perm = rng.permutation(pc.shape[0])
    table, flags = table_of(obs, [c == cfg_category for c in categories], cfg)
    return dict(cfg=cfg, obs=obs, pc=np.ascontiguousarray(pc[perm]), nrm=np.ascontiguousarray(nrm[perm]),
                inst=np.ascontiguousarray(inst[perm]), table=table, flags=flags)


def torch_targets(pc, nrm, idx, ob, cfg):
    """training.targets (torch fp32 on the CPU) for one object: (tr [P,2,tb], rot [P,2,rb], aux [P,2]) as numpy"""
    import torch
    from cppf_amd import training
    tr, rot, aux, _ = training.targets(torch.from_numpy(np.ascontiguousarray(pc, np.float32)), torch.from_numpy(np.ascontiguousarray(nrm, np.float32)),
                                       torch.from_numpy(np.asarray(idx, np.int64)), ob["center"], ob["R"], ob["half_extents"], cfg)
    return tr.numpy(), rot.numpy(), aux.numpy()
