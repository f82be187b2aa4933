"""cppf_amd.scene_training on the device: csrc/scene_train.hip against its numpy restatement (tests/scene_training_ref.py) -- the draw
bit for bit, the targets within 4 x what torch-fp32 training.targets itself deviates from the fp64 restatement --, a known-answer
scene whose decoded targets vote the target instances' centres, labelled_cloud against frame_inputs, and train_on_frames on rendered
frames of procedural meshes."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as MR  # noqa: E402
import scene_cloud_ref as C  # noqa: E402
import scene_poses_ref as SP  # noqa: E402
import scene_training_ref as R  # noqa: E402
from cppf_amd import mesh_frames as MF  # noqa: E402
from cppf_amd import scene_stage, training  # noqa: E402
from cppf_amd import scene_training as ST  # noqa: E402
from cppf_amd._torch_util import call  # noqa: E402
from cppf_amd.config import CATEGORIES  # noqa: E402

pytestmark = pytest.mark.gpu
N = 300
SIZES = [1, 257, 1000]
UP, TARGET = ST.FLAG_UP_SYM, ST.FLAG_TARGET


def _np(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


# ------------------------------------------------------------------------------------------------------------------- the draw
def _labels(seed):
    inst = np.random.default_rng(seed).integers(-1, 3, N).astype(np.int32)
    return inst, np.array([1, 0, 1], np.int32)                           # K = 3, instance 1 of another category: an empty segment


@pytest.mark.parametrize("P", SIZES)
def test_draw_equals_the_restatement(dev, P):
    inst, flags = _labels(3)
    members, seg_off = R.members_ref(inst, flags)
    assert seg_off[1] == seg_off[2] and members.shape[0] > 0
    inst_d = torch.from_numpy(inst).to(dev)
    m_d, off_d = ST.target_members(inst_d, flags)
    assert np.array_equal(m_d.cpu().numpy(), members) and np.array_equal(off_d.cpu().numpy(), seg_off)
    seed = 0x5EED0000 + P
    for n_pos in sorted({0, P // 2, P}):
        got = ST.sample_scene_pairs(m_d, off_d, inst_d, P, n_pos, seed)
        assert got.dtype == torch.int32 and tuple(got.shape) == (P, 2)
        want = R.draw_ref(members, seg_off, inst, N, P, n_pos, seed)
        assert np.array_equal(got.cpu().numpy(), want), n_pos
        a, b = want[:n_pos, 0], want[:n_pos, 1]
        assert np.all(inst[a] == inst[b]) and np.all(flags[inst[a]] & 1 == 1)
        assert torch.equal(ST.sample_scene_pairs(m_d, off_d, inst_d, P, n_pos, seed), got)             # the same seed twice
    # host arrays and int64 tensors are converted, a float table is refused
    again = ST.sample_scene_pairs(members.astype(np.int64), off_d.long(), inst_d.long(), P, P, seed)
    assert np.array_equal(again.cpu().numpy(), R.draw_ref(members, seg_off, inst, N, P, P, seed))
    with pytest.raises(TypeError):
        ST.sample_scene_pairs(m_d.float(), off_d, inst_d, P, P, seed)
    # M = 0: every pair is uniform
    m0, off0 = ST.target_members(inst_d, np.zeros(3, np.int32))
    assert m0.shape[0] == 0 and int(off0[-1]) == 0
    got = ST.sample_scene_pairs(m0, off0, inst_d, P, P, seed).cpu().numpy()
    assert np.array_equal(got, R.draw_ref(np.zeros(0, np.int32), np.zeros(4, np.int32), inst, N, P, P, seed))
    assert np.array_equal(got, R.draw_ref(members, seg_off, inst, N, P, 0, seed))


# ---------------------------------------------------------------------------------------------------------------- the targets
def scene3_case(**bins):
    """bottle, can, bottle and 60 background points: instances 0 and 2 are of the target category, instance 0 alone is up_sym; one list
    of 1000 pairs (half from the positive stratum) with its fp64 restatement and what torch fp32 deviates from it.  bins: tr_num_bins
    / rot_num_bins other than the config's (tests/test_gpu_scene_limits.py: the ends of the accepted range)"""
    s = R.posed_scene(["bottle", "can", "bottle"], "bottle", N, seed=21, n_background=60, up_sym=False)
    s["flags"] = np.array([TARGET | UP, 0, TARGET], np.int32)
    s["cfg"] = dataclasses.replace(s["cfg"], **bins)
    cfg, n = s["cfg"], s["pc"].shape[0]
    members, seg_off = R.members_ref(s["inst"], s["flags"])
    idx = R.draw_ref(members, seg_off, s["inst"], n, 1000, 500, seed=22)
    t64 = R.targets_ref(s["pc"], s["nrm"], s["inst"], idx, s["table"], s["flags"], cfg.vote_range, cfg.tr_num_bins, cfg.rot_num_bins)
    tr64, rot64 = R.dense_all(t64, cfg.tr_num_bins, cfg.rot_num_bins)
    tr32, rot32 = np.zeros_like(tr64), np.zeros_like(rot64)
    for k in (0, 2):                                                     # training.targets per instance, on that instance's pairs
        w = t64["pair_inst"] == k
        a, b, _ = R.torch_targets(s["pc"], s["nrm"], idx[w], s["obs"][k], dataclasses.replace(cfg, up_sym=bool(s["flags"][k] & UP)))
        tr32[w], rot32[w] = a, b
    pos, hard = t64["kind"] == 1, R.hard_pairs(t64, cfg.res)
    s.update(idx=idx, t64=t64, tr64=tr64, rot64=rot64, pos=pos, hard=hard,
             dev_tr=float(np.abs(tr32 - tr64)[pos].max()), dev_rot=float(np.abs(rot32 - rot64)[pos & ~hard].max()))
    print(f"torch fp32 against fp64 on {int(pos.sum())} positives: mu/nu {s['dev_tr']:.3g}, angles {s['dev_rot']:.3g}, "
          f"{100 * hard.mean():.2f} % of the pairs set aside")
    return s


@pytest.fixture(scope="module")
def scene3():
    """scene3_case at the config's bins, computed once: the cases below are slices of its list"""
    return scene3_case()


def _device_targets(s, dev, idx, inst=None, table=None, flags=None):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ST.scene_pair_targets(d(s["pc"]), d(s["nrm"]), d(s["inst"] if inst is None else inst), d(idx),
                                 s["table"] if table is None else table, s["flags"] if flags is None else flags, s["cfg"])


def _check_against(s, t, t64, tr64, rot64, hard, what=""):
    """the kernel's targets `t` (numpy) against the restatement's: kind and pair_inst exactly, aux where the sign is clear, the dense
    bins within 4 x the yardstick, the hard pairs in range"""
    cfg = s["cfg"]
    P = t64["kind"].shape[0]
    assert np.array_equal(t["kind"], t64["kind"]) and np.array_equal(t["pair_inst"], t64["pair_inst"]), what
    pos = t64["kind"] == 1
    unclear = pos & (t64["aux_margin"] < 1e-6).any(-1)
    assert unclear.sum() <= 0.01 * P and np.array_equal(t["aux"][~unclear], t64["aux"][~unclear]), what
    top = np.array([cfg.tr_num_bins - 2] * 2 + [cfg.rot_num_bins - 2] * 2)
    assert np.all(np.isfinite(t["w_low"])) and np.all(t["low"] <= top) and np.all((t["w_low"] >= 0) & (t["w_low"] <= 1)), what
    assert hard.sum() <= 0.03 * P, what
    tr, rot = R.dense_all(t, cfg.tr_num_bins, cfg.rot_num_bins)
    d_tr = float(np.abs(tr - tr64)[pos].max()) if pos.any() else 0.0
    d_rot = float(np.abs(rot - rot64)[pos & ~hard].max()) if (pos & ~hard).any() else 0.0
    print(f"{what}: kernel against fp64: mu/nu {d_tr:.3g} (yardstick {s['dev_tr']:.3g}), angles {d_rot:.3g} (yardstick {s['dev_rot']:.3g})")
    assert d_tr <= 4 * s["dev_tr"] and d_rot <= 4 * s["dev_rot"], what
    neg = t64["kind"] != 1                                               # negatives and kind 255: the fill values, exactly
    assert np.array_equal(t["low"][neg], t64["low"][neg]) and np.array_equal(t["w_low"][neg], t64["w_low"][neg].astype(np.float32))
    assert not t["aux"][neg].any()


@pytest.mark.parametrize("P", SIZES)
def test_targets_on_three_instances_with_background(dev, scene3, P):
    """The cases are slices of scene3's one list that straddle the end of its positive stratum (pair 499 is a positive); the yardstick
    is the one computed on the whole list, shared"""
    s = scene3
    lo = {1: 499, 257: 372, 1000: 0}[P]
    w = slice(lo, lo + P)
    t64 = {k: v[w] for k, v in s["t64"].items()}
    assert (t64["kind"] == 1).any() and (P == 1 or (t64["kind"] == 0).any())
    assert P < 1000 or ({0, 2} == set(np.unique(t64["pair_inst"][t64["kind"] == 1])) and (t64["kind"] == 0).sum() > 100)
    t = _np(_device_targets(s, dev, s["idx"][w]))
    assert t["kind"].dtype == np.uint8 and t["low"].shape == (P, 4) and t["w_low"].shape == (P, 4) and t["aux"].shape == (P, 2)
    _check_against(s, t, t64, s["tr64"][w], s["rot64"][w], s["hard"][w], f"P={P}")
    if P == 1000:                                                        # up_sym acts on instance 0 alone
        up = t["low"][:, 2].astype(np.float64) + 1 - t["w_low"][:, 2]
        half = (s["cfg"].rot_num_bins - 1) / 2
        assert up[t["pair_inst"] == 0].max() <= half + 1e-3 < up[t["pair_inst"] == 2].max()


def test_targets_edge_cases(dev, scene3):
    s = scene3
    cfg, n, idx = s["cfg"], s["pc"].shape[0], s["idx"]
    base = _np(_device_targets(s, dev, idx))
    # an index equal to N (and a negative one): kind 255, every other pair unchanged
    bad = idx.copy()
    bad[7, 1], bad[500, 0], bad[999, 0] = n, -1, 2 ** 31 - 1
    t = _np(_device_targets(s, dev, bad))
    rows = np.array([7, 500, 999])
    assert np.all(t["kind"][rows] == 255) and np.all(t["pair_inst"][rows] == -1) and (t["kind"] == 255).sum() == 3
    keep = np.ones(1000, bool)
    keep[rows] = False
    assert all(np.array_equal(t[k][keep], base[k][keep]) for k in base)
    assert np.array_equal(t["low"][rows], np.tile([0, cfg.tr_num_bins - 2, 0, 0], (3, 1))) and np.array_equal(t["w_low"][rows], np.tile([1, 0, 1, 1], (3, 1)))
    # a label equal to K and a label of -7 are background
    inst = s["inst"].copy()
    moved = np.nonzero(inst == 0)[0][::2]
    inst[moved[::2]], inst[moved[1::2]] = 3, -7
    t = _np(_device_targets(s, dev, idx, inst=inst))
    t64 = R.targets_ref(s["pc"], s["nrm"], inst, idx, s["table"], s["flags"], cfg.vote_range, cfg.tr_num_bins, cfg.rot_num_bins)
    touched = np.isin(idx, moved).any(-1)
    assert touched.sum() > 20 and np.all(t["kind"][touched] == 0) and np.all(t["pair_inst"][touched] == -1)
    assert np.array_equal(t["kind"], t64["kind"]) and np.array_equal(t["pair_inst"], t64["pair_inst"])
    # int64 pairs / labels and a device table are converted; K = 32 runs; K = 33 is refused by the wrapper and by the entry point
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = _np(ST.scene_pair_targets(d(s["pc"]).double(), d(s["nrm"]), d(s["inst"]).long(), d(idx).long(), d(s["table"]), d(s["flags"]), cfg))
    assert all(np.array_equal(t[k], base[k]) for k in base)
    reps = 11
    table32, flags32 = np.tile(s["table"], (reps, 1))[:32], np.tile(s["flags"], reps)[:32]
    inst32 = np.where(s["inst"] >= 0, s["inst"] + 3 * (np.arange(n) % 10), -1).astype(np.int32)         # labels up to 29, same rows' values
    inst32[np.nonzero(s["inst"] == 0)[0][:5]] = 30                        # ... and rows 30 (a target, as row 0) and 31 (as row 1)
    t = _np(_device_targets(s, dev, idx, inst=inst32, table=table32, flags=flags32))
    t64 = R.targets_ref(s["pc"], s["nrm"], inst32, idx, table32, flags32, cfg.vote_range, cfg.tr_num_bins, cfg.rot_num_bins)
    assert np.array_equal(t["kind"], t64["kind"]) and np.array_equal(t["pair_inst"], t64["pair_inst"]) and t["pair_inst"].max() >= 20
    with pytest.raises(ValueError):
        _device_targets(s, dev, idx, table=np.tile(s["table"], (reps, 1)), flags=np.tile(s["flags"], reps))
    out = ST.scene_pair_targets(d(s["pc"]), d(s["nrm"]), d(s["inst"]), d(idx), s["table"], s["flags"], cfg)
    rc = call("cppf_scene_pair_targets", dev, d(s["pc"]), d(s["nrm"]), d(s["inst"]), n, d(idx), 1000, d(np.tile(s["table"], (reps, 1))),
              d(np.tile(s["flags"], reps)), 33, float(cfg.vote_range[0]), float(cfg.vote_range[1]), cfg.tr_num_bins, cfg.rot_num_bins,
              out["kind"], out["pair_inst"], out["low"], out["w_low"], out["aux"], ok=(-1,))
    assert rc == -1 and all(np.array_equal(v.cpu().numpy(), base[k]) for k, v in out.items())          # refused: nothing was written
    with pytest.raises(ValueError):
        ST.scene_pair_targets(d(s["pc"]).cpu(), d(s["nrm"]), d(s["inst"]), d(idx), s["table"], s["flags"], cfg)


@pytest.mark.parametrize("cat", ["bottle", "mug"])
def test_single_instance_scene_agrees_with_training_targets(dev, cat):
    s = R.posed_scene([cat], cat, N, seed=31)
    cfg = s["cfg"]
    idx = np.random.default_rng(32).integers(0, N, (1000, 2)).astype(np.int32)
    t64 = R.targets_ref(s["pc"], s["nrm"], s["inst"], idx, s["table"], s["flags"], cfg.vote_range, cfg.tr_num_bins, cfg.rot_num_bins)
    tr64, rot64 = R.dense_all(t64, cfg.tr_num_bins, cfg.rot_num_bins)
    tr32, rot32, aux32 = R.torch_targets(s["pc"], s["nrm"], idx, s["obs"][0], cfg)
    hard = R.hard_pairs(t64, cfg.res)
    assert np.all(t64["kind"] == 1) and hard.mean() <= 0.03
    s.update(dev_tr=float(np.abs(tr32 - tr64).max()), dev_rot=float(np.abs(rot32 - rot64)[~hard].max()))
    t = _device_targets(s, dev, idx)
    _check_against(s, _np(t), t64, tr64, rot64, hard, cat)
    tr, rot, aux, scale = ST.dense_targets(t, cfg, torch.from_numpy(s["table"]).to(dev))
    tr, rot, aux = tr.cpu().numpy(), rot.cpu().numpy(), aux.cpu().numpy()
    d_tr, d_rot = float(np.abs(tr - tr32).max()), float(np.abs(rot - rot32)[~hard].max())
    print(f"{cat}: kernel against torch fp32: mu/nu {d_tr:.3g} (yardstick {s['dev_tr']:.3g}), angles {d_rot:.3g} (yardstick {s['dev_rot']:.3g})")
    assert d_tr <= 4 * s["dev_tr"] and d_rot <= 4 * s["dev_rot"]
    clear = (t64["aux_margin"] >= 1e-6).all(-1)
    assert np.array_equal(aux[clear], aux32[clear])
    want = np.log(s["obs"][0]["half_extents"]) - np.log(np.asarray(cfg.scale_mean))
    assert np.allclose(scale.cpu().numpy(), want[None], rtol=0, atol=1e-6)


def test_known_answer_scene_votes_the_target_centres(dev):
    """three analytic objects, two of the target category; positives only, 20 000 pairs per object; the expected (mu, nu) of the targets
    voted into the scene grid must put one proposal on each target instance and none on the third object"""
    s = R.posed_scene(["bottle", "can", "bottle"], "bottle", 3 * 1024, seed=41)
    cfg = s["cfg"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pc, inst = d(s["pc"]), d(s["inst"])
    members, seg_off = ST.target_members(inst, s["flags"])
    P = 3 * 20000
    idx = ST.sample_scene_pairs(members, seg_off, inst, P, P, seed=42)
    t = ST.scene_pair_targets(pc, d(s["nrm"]), inst, idx, s["table"], s["flags"], cfg)
    assert bool((t["kind"] == 1).all()) and set(torch.unique(t["pair_inst"]).tolist()) == {0, 2}
    x = t["low"][:, :2].float() + (1.0 - t["w_low"][:, :2])                  # the expectation of the two-bin target, in bins
    v0, v1 = cfg.vote_range
    outputs = torch.stack([x[:, 0] * (2 * v0 / (cfg.tr_num_bins - 1)) - v0, x[:, 1] * (v1 / (cfg.tr_num_bins - 1))], -1).contiguous()
    _, corners, _, _, loc, val, diff, worlds = scene_stage.vote_proposals(pc, outputs, idx, cfg, 72, 1.0, 50, 10, 2, None)
    centers = [s["obs"][0]["center"], s["obs"][2]["center"]]
    assert loc.shape[0] == 2
    m = SP.match_objects(loc, corners[0], cfg.res, centers, tol_cells=1.0)
    assert None not in m and len(set(m)) == 2, (worlds, centers)
    assert np.abs(worlds - s["obs"][1]["center"][None]).max(-1).min() > 10 * cfg.res


# ------------------------------------------------------------------------------------------------------- frames of procedural meshes
def _unit(v):
    return v / np.linalg.norm(v.max(0) - v.min(0))


def _meshes():
    b, c = MR.necked_cylinder(0.15, 0.45, neck=0.4, n_lon=32), MR.necked_cylinder(0.2, 0.3, neck=0.95, n_lon=32)
    return {"bottle": [(_unit(b[0]), b[1])], "can": [(_unit(c[0]), c[1])]}


def test_labelled_cloud_equals_frame_inputs(dev):
    cfg = CATEGORIES["bottle"]
    fr = MF.MeshFrameSampler(_meshes(), 2, device=dev, seed=3, z_range=(0.6, 1.0)).sample()
    assert len(fr.visible(200)) == 2
    hi, hi_nrm, hi_inst, ind, pc, nrm, inst = got = ST.labelled_cloud(fr, cfg)
    # the independent side: the single public calls composed in tests/scene_cloud_ref.py (labelled_cloud and frame_inputs share code)
    C.assert_same_cloud(got, C.hand_scene_cloud(fr.depth_mm, fr.intrinsics, cfg, labels=fr.labels))
    penc, _ = training.new_encoders(cfg, dev, seed=0)
    want = scene_stage.frame_inputs(fr.depth_mm, fr.intrinsics, penc.eval(), cfg, 16, 0)
    for got, ref in zip((hi, hi_nrm, ind, pc, nrm), want[:5]):
        assert got.dtype == ref.dtype and torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, ref.view(torch.int32) if ref.dtype == torch.float32 else ref)
    K = len(fr.categories)
    assert hi_inst.dtype == torch.int32 and int(hi_inst.min()) >= -1 and int(hi_inst.max()) < K and torch.equal(inst, hi_inst[ind])
    assert set(torch.unique(hi_inst).tolist()) == {0, 1}                # (a rendered frame has no background depth)
    # every label is the label image at the point's own pixel: the point projects back into that pixel (mesh_frames: the frame path
    # returns ((c - cx) z / fx, (r - cy) z / fy, z))
    K_ = fr.intrinsics
    p = hi.double().cpu().numpy()
    col = np.rint(p[:, 0] / p[:, 2] * K_[0, 0] + K_[0, 2]).astype(np.int64)
    row = np.rint(p[:, 1] / p[:, 2] * K_[1, 1] + K_[1, 2]).astype(np.int64)
    assert np.array_equal(fr.labels.cpu().numpy()[row, col], hi_inst.cpu().numpy())
    jit = np.random.default_rng(0).standard_normal((fr.depth_mm.size, 3)).astype(np.float32)
    hj = ST.labelled_cloud(fr, cfg, jitter=jit)
    wj = scene_stage.frame_cloud(fr.depth_mm, fr.intrinsics, cfg, jit)
    assert torch.equal(hj[0], wj[0]) and torch.equal(hj[1], wj[1]) and hj[2].shape[0] == hj[0].shape[0]
    C.assert_same_cloud(hj, C.hand_scene_cloud(fr.depth_mm, fr.intrinsics, cfg, jit, fr.labels))


STEPS = 40


def _params(penc, enc):
    return [p.detach().clone() for p in [*penc.parameters(), *enc.parameters()]]


def test_train_on_frames(dev):
    """two categories, two objects, 40 steps of 4 000 pairs: finite falling losses, both encoders moved, a step's draws and targets
    repeat under one seed, a frame without the category is skipped and counted"""
    cfg = CATEGORIES["bottle"]
    sampler = lambda seed, meshes=None: MF.MeshFrameSampler(meshes or _meshes(), 2, device=dev, seed=seed)
    encoders = training.new_encoders(cfg, dev, seed=0)
    before = _params(*encoders)
    lines = []
    penc, enc, losses, skipped = ST.train_on_frames("bottle", sampler(100), dev, steps=STEPS, n_pairs=4000, seed=0, encoders=encoders,
                                                    log=lines.append)
    assert penc is encoders[0] and enc is encoders[1] and not penc.training and not enc.training
    assert len(losses) == STEPS - skipped > 0 and np.all(np.isfinite(losses)) and lines and "loss" in lines[0]
    after = _params(penc, enc)
    n_p = len(list(penc.parameters()))
    assert any(not torch.equal(a, b) for a, b in zip(before[:n_p], after[:n_p])) and any(not torch.equal(a, b) for a, b in zip(before[n_p:], after[n_p:]))
    # the draws and the targets of a step repeat: two samplers with one seed, the same step
    fa, fb = sampler(100).sample(), sampler(100).sample()
    sa, sb = (ST.step_inputs(f, fa.categories[0], cfg, 4000, 0.5, 0, 7) for f in (fa, fb))
    assert torch.equal(sa["idx"], sb["idx"]) and all(torch.equal(sa["targets"][k], sb["targets"][k]) for k in sa["targets"])
    assert not torch.equal(sa["idx"], ST.step_inputs(fa, fa.categories[0], cfg, 4000, 0.5, 0, 8)["idx"][:sa["idx"].shape[0]])
    # a frame without the category is skipped and counted; nothing is trained
    fresh = training.new_encoders(cfg, dev, seed=1)
    b2 = _params(*fresh)
    _, _, l2, s2 = ST.train_on_frames("bottle", sampler(5, {"can": _meshes()["can"]}), dev, steps=3, n_pairs=4000, encoders=fresh)
    assert l2 == [] and s2 == 3 and all(torch.equal(a, b) for a, b in zip(b2, _params(*fresh)))
    # ... and trains on negatives alone when they carry weight
    _, _, l3, s3 = ST.train_on_frames("bottle", sampler(5, {"can": _meshes()["can"]}), dev, steps=2, n_pairs=4000, neg_weight=0.5, encoders=fresh)
    assert s3 == 0 and len(l3) == 2 and np.all(np.isfinite(l3))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_train_on_frames_loss_falls(dev, seed):
    """the mean of the last five losses is below the mean of the first five, at 40 steps, for seeds 0-2"""
    sampler = MF.MeshFrameSampler(_meshes(), 2, device=dev, seed=200 + seed)
    _, _, losses, skipped = ST.train_on_frames("bottle", sampler, dev, steps=STEPS, n_pairs=4000, seed=seed)
    assert len(losses) == STEPS - skipped >= 10 and np.all(np.isfinite(losses))
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    print(f"seed {seed}: first five {first:.4f}, last five {last:.4f}, skipped {skipped}")
    assert last < first
