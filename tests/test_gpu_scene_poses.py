"""cppf_amd.scene_poses on the device.  Perfect heads (outputs= / heads=): proposals bit for bit the numpy restatement on the device's
own grid, every object found within the proposal cap, masks and kept lists equal to the oracle composition (oracle.backvote ->
zero_shot_ref.segment), every proposal's pose equal to tests/scene_poses_ref.py's composition of the oracle's single-object pieces.
Committed trained networks: scenes of held-out bottles / mugs against the per-object maxima of tests/test_gpu_trained.py, with the
instance path's errors on the same objects printed beside them.  bf16, a depth frame, the refusals.

Measured on one MI355X (centre in cells / up in degrees modulo sign / right in degrees modulo sign / largest relative scale error;
scene path | instance path on the same object; printed by test_trained_networks_find_every_object under -s, tabulated in DESIGN.md
3.7e):
  bottle 900000   0.58 / 1.79 / - / 0.063   |   1.13 / 1.79 / - / 0.043
  bottle 900001   0.42 / 4.66 / - / 0.052   |   0.43 / 4.96 / - / 0.047
  bottle 900002   0.83 / 3.63 / - / 0.085   |   0.33 / 3.63 / - / 0.069
  mug 900000      1.04 / 5.28 / 6.60 / 0.037   |   0.92 / 3.20 / 4.10 / 0.036
  mug 900001      1.42 / 2.09 / 4.06 / 0.024   |   1.42 / 2.09 / 4.06 / 0.024"""
import os
import sys

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
from conftest import GOLDEN
from cppf_amd import scene_poses, training
from cppf_amd.config import CATEGORIES
from cppf_amd.utils.util import fibonacci_sphere, num_sphere_bins

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_poses_ref as S  # noqa: E402
import zero_shot_ref as Z  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# `thresh` of the trained scenes, from their measured smoothed peaks: the objects' peaks stand 517..585 (bottles) and
# 1539..1541 (mugs) above their box edges, the next peak of either scene 206 / 245 -- 300 lies between
TRAINED_THRESH = 300


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _d(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("cat,n_obj,seed", S.PERFECT_SCENES)
def test_perfect_heads_proposals_segmentation_poses(oracle, dev, cat, n_obj, seed):
    sc = S.perfect_scene(cat, n_obj, seed)
    cfg, pc, nrm, idx, outputs, heads = sc["cfg"], sc["pc"], sc["nrm"], sc["idx"], sc["outputs"], sc["heads"]
    d = _d(dev)
    out = scene_poses.scene_poses(None, d(pc), d(nrm), None, d(idx), None, None, cfg, outputs=d(outputs), heads=d(heads),
                                  max_proposals=2 * n_obj)
    # proposals: bit for bit the restatement on the device's own vote grid, under the same cap
    el, ev, ed, _ = Z.proposals(Z.smooth(out["grid"].cpu().numpy()), max_proposals=2 * n_obj)
    loc, val, diff = out["proposals"]
    assert np.array_equal(loc, el) and np.array_equal(_bits(val), _bits(ev)) and np.array_equal(_bits(diff), _bits(ed))
    poses = out["poses"]
    assert len(poses) == loc.shape[0] <= 2 * n_obj
    # every object by its own proposal, within one cell
    m = S.match_objects(loc, out["corner"], cfg.res, [o["center"] for o in sc["obs"]])
    assert None not in m and len(set(m)) == n_obj, (m, [p["T"] for p in poses])
    sph = np.array(fibonacci_sphere(num_sphere_bins(1.5)))
    idx32 = idx.astype(np.int32)
    bits = out["surv_bits"].cpu().numpy().view(np.uint32)
    pairs, offsets = out["pairs"].cpu().numpy(), out["offsets"]
    assert offsets.shape == (len(poses) + 1,) and offsets[-1] == pairs.shape[0] and (bits >> np.uint32(len(poses)) == 0).all()
    for k, p in enumerate(poses):
        assert np.array_equal(p["T"], Z.world(loc[k], out["corner"], cfg.res))
        # masks and kept lists: the oracle composition at this proposal
        _, surv = oracle.backvote(pc, outputs, idx32, out["corner"], cfg.res, 72, out["dims"], p["T"].astype(np.float32),
                                  np.float32(3 * cfg.res))
        assert np.array_equal(((bits >> np.uint32(k)) & 1).astype(bool), surv)
        pm, pos = Z.segment(idx, surv, pc.shape[0])
        assert np.array_equal(p["point_mask"], pm) and p["point_mask"].dtype == bool
        assert np.array_equal(pairs[offsets[k]:offsets[k + 1]], pos) and p["n_pairs"] == pos.size
        if k in m:
            truth = sc["owner"] == m.index(k)
            assert (pm & truth).sum() / (pm | truth).sum() > 0.9
        # the pose: the oracle's single-object pieces on the same kept list
        r = S.pose_ref(oracle, pc, nrm, idx, heads, pos, p["T"], sph, cfg)
        assert np.abs(p["R"] - r["R"]).max() < 1e-6 and np.abs(p["up"] - r["up"]).max() < 1e-6
        assert np.abs(p["scale"] - r["scale"]).max() < 1e-6 and abs(p["scale_norm"] - r["scale_norm"]) < 1e-6
        assert (p["right"] is None) == (not cfg.regress_right)
        if cfg.regress_right:
            assert np.abs(p["right"] - r["right"]).max() < 1e-6
        assert np.abs(p["RT"] - r["RT"]).max() < 1e-6 and np.array_equal(p["RT"][:3, 3], p["T"])
    from cppf_amd.inference import nocs_result
    rec = nocs_result(poses)
    assert rec["pred_RTs"].shape == (len(poses), 4, 4) and np.isfinite(rec["pred_RTs"]).all()


def trained_scene(cat, n_obj, dev, seed=0):
    """n_obj held-out objects (seeds 900000 + j, 1536 points: those of tests/test_gpu_trained.py) 0.5 m apart, 100 000 n_obj^2 uniform
    pairs over the whole scene (about 100 000 per object: the instance path's count), features from the point encoder on the scene"""
    cfg = CATEGORIES[cat]
    penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
    obs = []
    for j in range(n_obj):
        ob = syn.make_posed_object(cat, 1536, 900000 + j)
        c = np.array([0.5 * j - 0.25 * (n_obj - 1), 0.0, 0.9])
        ob["pc"] = (ob["pc"] - ob["center"] + c).astype(np.float32)
        ob["center"] = c
        obs.append(ob)
    pc, nrm = np.concatenate([o["pc"] for o in obs]), np.concatenate([o["normals"] for o in obs])
    rng = np.random.default_rng(seed)
    P = 100000 * n_obj * n_obj
    idx = rng.integers(0, pc.shape[0], (P, 2)).astype(np.int64)
    u_tr, u_rot = rng.random((P, 2), dtype=np.float32), rng.random((P, 2), dtype=np.float32)
    d = _d(dev)
    with torch.no_grad():
        feat = penc(d(pc)[None], d(nrm)[None])[0]
    return dict(cfg=cfg, penc=penc, enc=enc, obs=obs, pc=d(pc), nrm=d(nrm), feat=feat, idx=d(idx), u_tr=d(u_tr), u_rot=d(u_rot))


def _match_within(poses, obs, cfg, cells):
    loc_like = [p["T"] for p in poses]
    used, out = set(), []
    for ob in obs:
        ds = [np.abs(t - ob["center"]).max() / cfg.res if k not in used else np.inf for k, t in enumerate(loc_like)]
        k = int(np.argmin(ds)) if ds else -1
        if k >= 0 and ds[k] <= cells:
            used.add(k)
            out.append(k)
        else:
            out.append(None)
    return out


@pytest.mark.parametrize("cat,n_obj", [("bottle", 3), ("mug", 2)])
def test_trained_networks_find_every_object(dev, cat, n_obj):
    """the per-object maxima of tests/test_gpu_trained.py (centre <= 4 cells, up <= 12 degrees modulo sign, scale <= 0.2; the mug's right
    axis <= 10 degrees modulo sign, that test's bound on it) on every object of a scene, with no masks"""
    sc = trained_scene(cat, n_obj, dev)
    cfg = sc["cfg"]
    out = scene_poses.scene_poses(sc["enc"], sc["pc"], sc["nrm"], sc["feat"], sc["idx"], sc["u_tr"], sc["u_rot"], cfg,
                                  thresh=TRAINED_THRESH)
    poses = out["poses"]
    print(f"\n{cat} x {n_obj}: smoothed peaks {np.round(out['proposals'][1], 1).tolist()} diffs {np.round(out['proposals'][2], 1).tolist()}")
    m = _match_within(poses, sc["obs"], cfg, 4.0)
    rows = []
    for j, ob in enumerate(sc["obs"]):
        inst = training.pose_errors(training.infer(sc["penc"], sc["enc"], ob, dev, seed=j), ob)
        scene = training.pose_errors(poses[m[j]], ob) if m[j] is not None else None
        rows.append((scene, inst))
        fmt = lambda e: "not found" if e is None else (f"{e['t_cells']:.2f} cells, up {e['up_deg_mod_sign']:.2f}, right "
                                                       f"{e['right_deg_mod_sign'] if e['right_deg_mod_sign'] is None else round(e['right_deg_mod_sign'], 2)}, "
                                                       f"scale {e['scale_rel']:.3f}")
        print(f"  object {900000 + j}: scene path {fmt(scene)} | instance path {fmt(inst)} | kept pairs "
              f"{poses[m[j]]['n_pairs'] if m[j] is not None else 0}")
    assert None not in m and len(set(m)) == n_obj, m
    assert len(poses) == n_obj                              # (what TRAINED_THRESH was chosen for: the objects and nothing else)
    for scene, _ in rows:
        assert scene["t_cells"] <= 4.0 and scene["up_deg_mod_sign"] <= 12.0 and scene["scale_rel"] <= 0.2, rows
        if cfg.regress_right:
            assert scene["right_deg_mod_sign"] <= 10.0, rows


def test_bf16_encoder_finds_the_same_objects(dev):
    sc = trained_scene("bottle", 3, dev)
    cfg = sc["cfg"]
    run = lambda: scene_poses.scene_poses(sc["enc"], sc["pc"], sc["nrm"], sc["feat"], sc["idx"], sc["u_tr"], sc["u_rot"], cfg,
                                          thresh=TRAINED_THRESH)
    m32 = _match_within(run()["poses"], sc["obs"], cfg, 4.0)
    sc["enc"].set_precision("bf16")
    out = run()
    assert sc["enc"].precision == "bf16"
    m16 = _match_within(out["poses"], sc["obs"], cfg, 4.0)
    assert None not in m32 and None not in m16 and len(set(m16)) == 3, (m32, m16)


def test_scene_frame_demo_depth(dev):
    """runs and returns consistent shapes on a real depth frame (no accuracy claim: the network never saw such a scene)"""
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    cfg = CATEGORIES["bottle"]
    penc, enc = training.load_weights(os.path.join(GOLDEN, "trained_bottle.npz"), cfg, dev)
    out = scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, n_pairs=1_000_000, seed=0, thresh=5.0, max_proposals=4)
    N, P = out["pc"].shape[0], out["n_pairs"]
    assert 0 < P <= 1_000_000 and out["idx"].shape == (P, 2)
    assert out["outputs"].shape == (P, 2) and out["heads"].shape == (P, 8) and out["surv_bits"].shape == (P,)
    assert tuple(out["grid"].shape) == tuple(out["dims"]) and out["feat"].shape[0] == N
    K = len(out["poses"])
    assert K == out["proposals"][0].shape[0] <= 4 and out["offsets"].shape == (K + 1,)
    for p in out["poses"]:
        for k in ("T", "R", "scale", "RT"):
            assert np.isfinite(p[k]).all(), k
        assert p["point_mask"].shape == (N,) and 0 <= p["n_pairs"] <= P
    with pytest.raises(ValueError, match="no valid pixels"):
        scene_poses.scene_frame(np.zeros((48, 64), np.uint16), NOCS_INTRINSICS, enc, penc, cfg, n_pairs=1000)


def test_refusals_and_the_empty_pair_list(dev):
    from cppf_amd.models.model import PPFEncoder
    cfg = CATEGORIES["bowl"]
    ob = syn.make_posed_object("bowl", 256, 3)
    d = _d(dev)
    pc, nrm = d(ob["pc"]), d(ob["normals"])
    feat = torch.zeros((256, 32), device=dev)
    idx = torch.zeros((10, 2), dtype=torch.int64, device=dev)
    u = torch.zeros((10, 2), device=dev)
    with pytest.raises(ValueError, match="out_dim"):
        scene_poses.scene_poses(PPFEncoder([84, 32, 32, 16], 9).to(dev), pc, nrm, feat, idx, u, u, cfg)
    with pytest.raises(ValueError, match="max_proposals"):
        scene_poses.scene_poses(PPFEncoder([84, 32, 32, 16], 141).to(dev), pc, nrm, feat, idx, u, u, cfg, max_proposals=33)
    with pytest.raises(ValueError, match="pc"):
        scene_poses.scene_poses(None, ob["pc"], nrm, None, idx, None, None, cfg, outputs=torch.zeros((10, 2), device=dev),
                                heads=torch.zeros((10, 8), device=dev))
    with pytest.raises(ValueError, match="one row per pair"):
        scene_poses.scene_poses(None, pc, nrm, None, idx, None, None, cfg, outputs=torch.zeros((9, 2), device=dev),
                                heads=torch.zeros((10, 8), device=dev))
    empty = scene_poses.scene_poses(None, pc, nrm, None, idx[:0], None, None, cfg, outputs=torch.zeros((0, 2), device=dev),
                                    heads=torch.zeros((0, 8), device=dev))
    assert empty["poses"] == [] and empty["offsets"].tolist() == [0] and empty["proposals"][0].shape == (0, 3)
    enc = PPFEncoder([84, 32, 32, 16], 141).to(dev).eval()
    assert scene_poses.scene_poses(enc, pc, nrm, feat, idx[:0], u[:0], u[:0], cfg)["poses"] == []
