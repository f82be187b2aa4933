"""What cppf_amd.scene_poses is held to: the scenes of its tests, and the pose of ONE proposal composed on the host from the oracle's
single-object pieces (rot_voting, sphere_count, axis_sign, scale -- the tail of nocs/inference.py:259-339 as oracle.estimate_pose
chains it) on the proposal's kept-pair list, plus the assembly of :299-339 restated in numpy.  The scene half (vote, smoothing,
proposals, back-vote, segmentation) is tests/zero_shot_ref.py's and the oracle's."""
import numpy as np

import cppf_amd.synthetic as syn
from cppf_amd.config import CATEGORIES

_f = np.float32


def assemble(up_dir, right_dir, scale, cfg, rng=None):
    """nocs/inference.py:305-339 from the signed axis directions: right orthogonalised against up (or the fixed (0, -up_z, up_y)
    for a category without a right axis), a random tangent when that degenerates, the z_right frame, RT = [R |scale|, T]"""
    up = np.asarray(up_dir, np.float64)
    if cfg.regress_right:
        right = np.asarray(right_dir, np.float64)
        right = right - np.dot(up, right) * up
    else:
        right = np.array([0.0, -up[2], up[1]])
    right = right / (np.linalg.norm(right) + 1e-9)
    if np.linalg.norm(right) < 1e-7:
        rng = rng or np.random.default_rng(0)
        right = rng.standard_normal(3)
        right -= right.dot(up) * up
        right /= np.linalg.norm(right)
    if cfg.z_right:
        R = np.stack([np.cross(up, right), up, right], -1)
    else:
        R = np.stack([right, up, np.cross(right, up)], -1)
    scale = np.asarray(scale, np.float64)
    return dict(up=up, right=right, R=R, scale=scale, scale_norm=float(np.linalg.norm(scale)))


def pose_ref(O, pc, nrm, idx, heads, sel, T, sphere_pts, cfg, angle_tol=1.5, max_rot_pairs=10000, n_rots=72, rot_order=None):
    """the pose of one proposal from its kept pairs `sel` (positions in idx, in pair order); heads f32[P,8] = {theta_up, theta_right,
    aux_up, aux_right, sx, sy, sz, 0}"""
    idx32 = np.ascontiguousarray(np.asarray(idx, np.int32))
    heads = np.asarray(heads, _f)
    sel = np.asarray(sel, np.int64)
    if rot_order is None:
        sub = sel[:max_rot_pairs]
    else:
        ro = np.asarray(rot_order)[:max_rot_pairs]
        sub = sel[ro[(ro >= 0) & (ro < sel.size)]]
    dirs = []
    for j in range(2 if cfg.regress_right else 1):
        cands = O.rot_voting(pc, np.ascontiguousarray(heads[sub, j]), np.ascontiguousarray(idx32[sub]), n_rots)
        counts = O.sphere_count(cands, sphere_pts, angle_tol)
        best = np.asarray(sphere_pts[int(np.argmax(counts))], np.float64)
        flip, _ = O.axis_sign(pc, nrm, np.ascontiguousarray(idx32[sel]), np.ascontiguousarray(heads[sel, 2 + j]), best)
        dirs.append(-best if flip else best)
    scale = O.scale(np.ascontiguousarray(heads[sel, 4:7]).reshape(-1, 3), cfg.scale_mean)     # (no pairs: exp(0) scale_mean 2)
    out = assemble(dirs[0], dirs[1] if len(dirs) > 1 else None, scale, cfg)
    out["T"] = np.asarray(T, np.float64)
    RT = np.eye(4)
    RT[:3, :3] = out["R"] * out["scale_norm"]
    RT[:3, -1] = out["T"]
    out["RT"] = RT
    return out


def object_centers(n_obj):
    """where the scenes put their objects: 0.3 m apart along x, staggered in y and z (tests/test_gpu_zero_shot.py:_scene)"""
    return [np.array([0.3 * k - 0.15 * (n_obj - 1), 0.05 * (k % 2), 0.8 + 0.1 * k]) for k in range(n_obj)]


def perfect_scene(cat, n_obj, seed, pairs_per_object=150000, n_points=2048):
    """n_obj objects of one category with the world's axes, a uniform pair list over all of them and the heads a perfectly trained
    bin-head network would emit: closed-form (mu, nu) and heads for within-object pairs, random values for cross-object pairs.
    -> dict(cfg, obs, pc, nrm, owner, idx i64[P,2], outputs f32[P,2], heads f32[P,8])"""
    cfg = CATEGORIES[cat]
    n_pairs = pairs_per_object * n_obj
    rng = np.random.default_rng(seed)
    obs, pcs, nrms = [], [], []
    for k, c in enumerate(object_centers(n_obj)):
        ob = syn.make_posed_object(cat, n_points, seed * 10 + k, rotate=False)
        ob["pc"] = (ob["pc"] - ob["center"] + c).astype(_f)
        ob["center"] = c
        obs.append(ob)
        pcs.append(ob["pc"])
        nrms.append(ob["normals"])
    pc, nrm = np.concatenate(pcs), np.concatenate(nrms)
    owner = np.repeat(np.arange(n_obj), n_points)
    idx = rng.integers(0, pc.shape[0], (n_pairs, 2))
    vr = cfg.vote_range
    outputs = np.empty((n_pairs, 2), _f)
    outputs[:, 0] = rng.uniform(-vr[0], vr[0], n_pairs)
    outputs[:, 1] = rng.uniform(0, vr[1], n_pairs)
    heads = np.zeros((n_pairs, 8), _f)
    heads[:, 0:2] = rng.uniform(0, np.pi, (n_pairs, 2))
    heads[:, 2:4] = rng.standard_normal((n_pairs, 2))
    heads[:, 4:7] = rng.standard_normal((n_pairs, 3))
    for k, ob in enumerate(obs):
        w = (owner[idx[:, 0]] == k) & (owner[idx[:, 1]] == k)
        outputs[w] = syn.closed_form_outputs(pc, ob["center"], idx[w], cfg, quantise=False)
        heads[w] = syn.closed_form_heads(pc, nrm, idx[w], cfg, quantise=False, seed=k)
    return dict(cfg=cfg, obs=obs, pc=pc, nrm=nrm, owner=owner, idx=idx, outputs=outputs, heads=heads)


PERFECT_SCENES = [("mug", 2, 1), ("mug", 3, 2), ("mug", 4, 3), ("bowl", 2, 1), ("bowl", 3, 2), ("bowl", 4, 3)]


def match_objects(locs, corner, res, centers, tol_cells=1.0):
    """every centre matched by a DISTINCT proposal within tol_cells cells (per axis): the matched proposal index per object, or None
    where there is none.  locs i32[K,3]; greedy in object order on the nearest unused proposal."""
    worlds = np.asarray(corner, _f).astype(np.float64)[None] + np.asarray(locs, np.int64).reshape(-1, 3) * float(res)
    used, out = set(), []
    for c in centers:
        best, best_d = None, None
        for k, w in enumerate(worlds):
            d = float(np.abs(w - c).max())
            if k not in used and d <= tol_cells * res * (1 + 1e-9) and (best is None or d < best_d):
                best, best_d = k, d
        if best is not None:
            used.add(best)
        out.append(best)
    return out
