"""The zero-shot scene path on the device (csrc/scene.hip, cppf_amd/zero_shot.py) against tests/zero_shot_ref.py, the numpy
restatement of nocs/zero_shot.ipynb cells 6, 9 and 11 (itself held to the notebook's own cells in test_zero_shot_cpu.py):
smoothing and proposals bit for bit, segmentation exactly, poses against the oracle-composed cell 11, graph replay = eager,
and the whole frame end to end."""
import os
import sys

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
from cppf_amd import scene_stage, zero_shot
from cppf_amd.config import CATEGORIES
from cppf_amd.utils.util import fibonacci_sphere

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zero_shot_ref as Z  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("sigma", [1.0, 2.0])
def test_smooth_bit_exact_small_dims(dev, sigma):
    rng = np.random.default_rng(11)
    for gx in range(1, 10):
        for gy in (1, 2, 3, 5, 9):
            for gz in (1, 4, 9):
                g = (rng.random((gx, gy, gz)) * 500).astype(np.float32)
                assert np.array_equal(_bits(zero_shot.smooth_grid(g, sigma)), _bits(Z.smooth(g, sigma))), (gx, gy, gz)


def test_smooth_bit_exact_demo_sized_grid(dev):
    rng = np.random.default_rng(12)
    g = np.zeros((321, 222, 164), np.float32)
    hot = rng.integers(0, g.size, 200000)
    g.reshape(-1)[hot] = rng.random(hot.size).astype(np.float32) * 40
    got = zero_shot.smooth_grid(torch.from_numpy(g).to(dev)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(Z.smooth(g)))


def _check_proposals(dev, g, **kw):
    loc, val, diff, count = zero_shot.scene_proposals_device(torch.from_numpy(g).to(dev), **kw)
    n = int(count.item())
    el, ev, ed, _ = Z.proposals(Z.smooth(g, kw.get("sigma", 1.0)), kw.get("thresh", 50), kw.get("margin", 10),
                                kw.get("max_proposals", 32), kw.get("max_iters"))
    assert n == el.shape[0], (n, el.shape)
    assert np.array_equal(loc[:n].cpu().numpy(), el)
    assert np.array_equal(_bits(val[:n].cpu().numpy()), _bits(ev)) and np.array_equal(_bits(diff[:n].cpu().numpy()), _bits(ed))
    return n


def test_proposals_fixture_grids(dev, golden):
    g = golden("zero_shot.npz")
    for name in g["cases"]:
        _check_proposals(dev, g[f"{name}.grid"])
        _check_proposals(dev, g[f"{name}.grid"], thresh=20, margin=3, max_proposals=5)
    sm = torch.empty(g["blobs.grid"].shape, dtype=torch.float32, device=dev)
    zero_shot.scene_proposals_device(torch.from_numpy(g["blobs.grid"]).to(dev), smoothed_out=sm)
    assert np.array_equal(_bits(sm.cpu().numpy()), _bits(Z.smooth(g["blobs.grid"])))


def _scene(n_obj, seed, n_pairs=None, n_points=2048):
    """n_obj bowls placed apart (axes = world axes) and a uniform pair list over all of them; within-object pairs get the known
    answer (closed-form (mu, nu), orientation and scale heads), cross-object pairs random values: a perfect 9-wide head"""
    cfg = CATEGORIES["bowl"]
    n_pairs = 150000 * n_obj if n_pairs is None else n_pairs
    rng = np.random.default_rng(seed)
    obs, pcs, nrms = [], [], []
    for k in range(n_obj):
        ob = syn.make_posed_object("bowl", n_points, seed * 10 + k, rotate=False)
        c = np.array([0.3 * k - 0.15 * (n_obj - 1), 0.05 * (k % 2), 0.8 + 0.1 * k])      # 0.3 apart: the bowls never touch
        ob["pc"] = (ob["pc"] - ob["center"] + c).astype(np.float32)
        ob["center"] = c
        obs.append(ob)
        pcs.append(ob["pc"])
        nrms.append(ob["normals"])
    pc, nrm = np.concatenate(pcs), np.concatenate(nrms)
    owner = np.repeat(np.arange(n_obj), n_points)
    idx = rng.integers(0, pc.shape[0], (n_pairs, 2))
    preds = np.empty((n_pairs, 9), np.float32)
    vr = cfg.vote_range
    preds[:, 0] = rng.uniform(-vr[0], vr[0], n_pairs)
    preds[:, 1] = rng.uniform(0, vr[1], n_pairs)
    preds[:, 2:4] = rng.uniform(0, np.pi, (n_pairs, 2))
    preds[:, 4:6] = rng.standard_normal((n_pairs, 2))
    preds[:, 6:9] = rng.standard_normal((n_pairs, 3))
    for k, ob in enumerate(obs):
        w = (owner[idx[:, 0]] == k) & (owner[idx[:, 1]] == k)
        preds[w, 0:2] = syn.closed_form_outputs(pc, ob["center"], idx[w], cfg, quantise=False)
        h = syn.closed_form_heads(pc, nrm, idx[w], cfg, quantise=False, seed=k)
        preds[w, 2:9] = h[:, :7]
    return cfg, obs, pc, nrm, owner, idx, preds


@pytest.mark.parametrize("n_obj,seed", [(2, 1), (3, 2), (4, 3)])
def test_synthetic_scene_proposals_segmentation_poses(oracle, dev, n_obj, seed):
    cfg, obs, pc, nrm, owner, idx, preds = _scene(n_obj, seed)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = zero_shot.zero_shot_scene(None, d(pc), d(nrm), None, d(idx), cfg, preds=d(preds))
    grid = out["grid"].cpu().numpy()
    # proposals: bit for bit the restatement on the device's own vote grid
    el, ev, ed, _ = Z.proposals(Z.smooth(grid))
    loc, val, diff = out["proposals"]
    assert np.array_equal(loc, el) and np.array_equal(_bits(val), _bits(ev)) and np.array_equal(_bits(diff), _bits(ed))
    poses = out["poses"]
    # every object is found (the notebook's loop may also propose a second peak of one object's vote ridge beyond the margin)
    assert len(poses) >= n_obj, [p["T"] for p in poses]
    sph = np.array(fibonacci_sphere(zero_shot.num_sphere_bins(2)))
    for k, ob in enumerate(obs):
        p = poses[int(np.argmin([np.linalg.norm(q["T"] - ob["center"]) for q in poses]))]
        assert np.abs(p["T"] - ob["center"]).max() <= cfg.res, (p["T"], ob["center"])
        # segmentation: exactly the restatement, and the object's points
        seg = zero_shot.segment_instance(d(pc), d(preds), d(idx), p["T"], out["corner"], cfg.res, out["dims"])
        _, surv = oracle.backvote(pc, preds[:, :2], idx.astype(np.int32), out["corner"], cfg.res, 72, out["dims"],
                                  p["T"].astype(np.float32), np.float32(3 * cfg.res))
        pm, pos = Z.segment(idx, surv, pc.shape[0])
        assert np.array_equal(seg["point_mask"].cpu().numpy(), pm) and np.array_equal(p["point_mask"], pm)
        assert np.array_equal(seg["pairs"].cpu().numpy(), pos) and p["n_pairs"] == pos.size
        truth = owner == k
        assert (pm & truth).sum() / (pm | truth).sum() > 0.9
        # pose: the oracle-composed rest of cell 11
        r = Z.pose_ref(oracle, pc, nrm, idx, preds, pos, p["T"], sph, cfg.scale_mean)
        assert np.degrees(np.arccos(np.clip(p["up"] @ np.array([0.0, 1.0, 0.0]), -1, 1))) < 2.0
        assert np.abs(p["R"] - r["R"]).max() < 1e-6 and np.abs(p["scale_3d"] - r["scale_3d"]).max() < 1e-6
        assert np.allclose(p["RT"][:3, :3], p["R"] * p["scale"]) and np.array_equal(p["RT"][:3, 3], p["T"])


def test_pair_filter_and_segmentation_kernels(dev, golden):
    rng = np.random.default_rng(21)
    pc = rng.standard_normal((3000, 3)).astype(np.float32)
    nrm = rng.standard_normal((3000, 3)).astype(np.float32)
    nrm[:1500] = [0, 0, 1]
    pc[:1500, 2] = 0.25
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    idx = rng.integers(0, 3000, (200000, 2))
    kept = zero_shot.distinct_pairs(torch.from_numpy(pc).to(dev), torch.from_numpy(nrm).to(dev), torch.from_numpy(idx).to(dev))
    assert np.array_equal(kept.cpu().numpy(), idx[Z.distinct_mask(pc, nrm, idx)])
    g = golden("zero_shot.npz")
    from cppf_amd import _lib
    from cppf_amd._torch_util import stream_ptr
    L = _lib.lib()
    for s in range(4):
        i32, surv = g[f"seg{s}.idx"], g[f"seg{s}.surv"]
        P, N = i32.shape[0], 200
        pm = torch.empty(N, dtype=torch.uint8, device=dev)
        pairs = torch.empty(P, dtype=torch.int32, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(L.cppf_segment_instance_workspace_bytes(N, P), dtype=torch.uint8, device=dev)
        di, ds = torch.from_numpy(i32).to(dev), torch.from_numpy(surv.astype(np.uint8)).to(dev)
        _lib.check(L.cppf_segment_instance(di.data_ptr(), ds.data_ptr(), P, N, 12, pm.data_ptr(), pairs.data_ptr(), cnt.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream_ptr(dev)), "cppf_segment_instance")
        n = int(cnt.item())
        assert np.array_equal(pm.cpu().numpy().astype(bool), g[f"seg{s}.point_mask"])
        assert np.array_equal(i32[pairs[:n].cpu().numpy()], g[f"seg{s}.pairs"])


def test_graph_replay_equals_eager(dev):
    cfg, obs, pc, nrm, owner, idx, preds = _scene(3, 7, n_pairs=100000)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eager = zero_shot.zero_shot_scene(None, d(pc), d(nrm), None, d(idx), cfg, preds=d(preds))
    grid, corner, dims = eager["grid"], eager["corner"], eager["dims"]
    pcd, od, i32 = d(pc), d(preds[:, :2]), d(idx.astype(np.int32))
    ws = zero_shot.proposals_workspace(dims, dev)
    res_t = tuple(torch.empty(s, dtype=t, device=dev) for s, t in [((32, 3), torch.int32), (32, torch.float32), (32, torch.float32),
                                                                   (1, torch.int32)])
    T32 = torch.from_numpy(eager["poses"][0]["T"].astype(np.float32)[None]).to(dev)
    cd = torch.from_numpy(corner.copy()).to(dev)

    def segment():                                     # the enqueue zero_shot_scene shares with scene_poses, at one centre
        bits = scene_stage.backvote_multi(pcd, od, i32, cd, cfg.res, dims, T32, 72, float(np.float32(3 * cfg.res)))
        return scene_stage.segment_instances(i32, bits, pcd.shape[0], 1, 12)
    zero_shot.scene_proposals_device(grid, out=res_t, ws=ws)                     # warm-up (scratch allocated outside the capture)
    segment()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            zero_shot.scene_proposals_device(grid, out=res_t, ws=ws)
            seg = segment()
    for t in res_t:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    n = int(res_t[3].item())
    loc, val, diff = eager["proposals"]
    assert n == loc.shape[0] and np.array_equal(res_t[0][:n].cpu().numpy(), loc)
    assert np.array_equal(_bits(res_t[1][:n].cpu().numpy()), _bits(val)) and np.array_equal(_bits(res_t[2][:n].cpu().numpy()), _bits(diff))
    masks, pairs, offsets = seg
    assert np.array_equal(masks[0].cpu().numpy().astype(bool), eager["poses"][0]["point_mask"])
    assert int(offsets[1].item()) == eager["poses"][0]["n_pairs"]


def test_zero_shot_frame_demo_depth(oracle, dev):
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.models.model import PointEncoder, PPFEncoder
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(ROOT, "tests", "golden", "demo_0000_depth.png"))
    cfg = CATEGORIES["bowl"]
    torch.manual_seed(0)
    enc = PPFEncoder([84, 32, 32, 16], 9)
    with torch.no_grad():            # a head that answers the same (mu, nu) for every pair: the votes pile up, proposals exist
        enc.final.weight.mul_(1e-3)
        enc.final.bias.copy_(torch.tensor([0.0, 0.02, 1.0, 1.5, 0.5, 0.0, 0.0, 0.0, 0.0]))
    enc = enc.to(dev).eval()
    penc = PointEncoder(k=cfg.knn, spfcs=[32, 64, 32, 32], out_dim=32, num_layers=1).to(dev).eval()
    out = zero_shot.zero_shot_frame(depth, NOCS_INTRINSICS, enc, penc, cfg, n_pairs=1_000_000, seed=0, thresh=5.0,
                                    max_proposals=4)
    hi = out["hi_pc"].cpu().numpy()
    assert np.array_equal(out["indices"].cpu().numpy(), oracle.voxel_dedupe(hi, 4 * cfg.res))
    assert np.array_equal(out["pc"].cpu().numpy(), hi[oracle.voxel_dedupe(hi, 4 * cfg.res)])
    assert 0 < out["n_pairs"] <= 1_000_000 and out["preds"].shape == (out["n_pairs"], 9)
    assert len(out["poses"]) >= 1
    for p in out["poses"]:
        for k in ("T", "R", "scale_3d", "RT"):
            assert np.isfinite(p[k]).all(), k
        assert p["point_mask"].shape == (out["pc"].shape[0],)
