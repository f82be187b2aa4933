"""Proposal verification on the device (csrc/verify.hip, scene_stage.verify_proposals) against tests/verify_ref.py:
cppf_proposal_support word for word on random lists (lane, wave and workgroup edges, a second grid-stride trip, out-of-range
endpoints, bits >= K) and on the outputs of cppf_backvote_multi + cppf_segment_instances; cppf_box_support equal to the float64
restatement on points kept out of a band around every face; the known answer of a perfect-head scene (true centres against decoys);
scene_poses / zero_shot_scene / frame_detections with and without verify; graph replay; the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
from conftest import GOLDEN
from cppf_amd import _lib, detections, scene_poses, scene_stage, training, zero_shot
from cppf_amd._torch_util import stream_ptr
from cppf_amd.config import CATEGORIES
from cppf_amd.inference import grid_shape

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_poses_ref as S  # noqa: E402
import verify_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
SECOND_TRIP = 1024 * 256 + 257           # csrc/verify.hip: VF_MAX_BLOCKS workgroups of 256 lanes -- a longer list enters the stride loop
SIZES = [0, 1, 63, 64, 65, 1023, 1025, 4099, SECOND_TRIP]
KS, NS = [1, 5, 32], [1, 70, 1000]
BAND = 1e-4                              # no point within this of a face, relative to the half extent (float64)
FRAME_KW = dict(n_pairs=200_000, seed=3, thresh=5.0, max_proposals=4)


def _d(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _support(dev, idx, bits, masks):
    """cppf_proposal_support through scene_stage.proposal_support, twice, into a table with guard words on both sides"""
    K = masks.shape[0]
    d = _d(dev)
    d_idx, d_bits, d_masks = d(idx.astype(np.int32)), d(bits.view(np.int32)), d(masks)
    runs = []
    for _ in range(2):
        buf = torch.full((4 * K + 16,), -7, dtype=torch.int32, device=dev)
        scene_stage.proposal_support(d_idx, d_bits, d_masks, out=buf[8:8 + 4 * K].view(K, 4))
        got = buf.cpu().numpy()
        assert (got[:8] == -7).all() and (got[8 + 4 * K:] == -7).all()
        runs.append(got[8:8 + 4 * K].reshape(K, 4))
    assert np.array_equal(runs[0], runs[1])                                   # the same words on every run
    return runs[0]


def _random_list(P, K, N, density, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(-2, N + 2, (P, 2)).astype(np.int32)                     # out-of-range endpoints on both sides
    bits = rng.integers(0, 1 << 32, P, dtype=np.uint64).astype(np.uint32)      # every bit, those >= K included
    masks = (rng.random((K, N)) < density).astype(np.uint8) * rng.integers(1, 256, (K, N)).astype(np.uint8)
    return idx, bits, masks


@pytest.mark.parametrize("P", SIZES)
def test_proposal_support_random_lists(dev, P):
    for K in KS:
        for N in NS:
            for density in ((0.3,) if P == SECOND_TRIP else (0.0, 0.3, 1.0)):
                idx, bits, masks = _random_list(P, K, N, density, seed=P + 7 * K + N)
                want = V.proposal_support(idx, bits, masks)
                got = _support(dev, idx, bits, masks)
                assert np.array_equal(got, want), (P, K, N, density)
                if P >= 1023 and density == 0.3 and N > 1:
                    assert want[:, 0].all() and want[:, 2].all() and (want[:, 1] < want[:, 0]).all()      # (something to count)
                if P == 0 or density == 0.0:
                    assert not got.any()


def _bowls():
    """the cloud of tests/test_gpu_scene_multi.py, rebuilt: 512 points of three posed bowls placed apart, points 0 and 1 coincident;
    4099 uniform pairs with the closed-form (mu, nu) inside an object and random values elsewhere, (i, i) pairs included"""
    cfg = CATEGORIES["bowl"]
    pcs, centers = [], []
    for k, n in enumerate((171, 171, 170)):
        ob = syn.make_posed_object("bowl", n, 40 + k)
        c = np.array([0.35 * k - 0.35, 0.04 * k, 0.8 + 0.05 * k])
        pcs.append((ob["pc"] - ob["center"] + c).astype(np.float32))
        centers.append(c)
    pc = np.concatenate(pcs)
    pc[1] = pc[0]
    owner = np.repeat(np.arange(3), (171, 171, 170))
    rng = np.random.default_rng(3)
    P = 4099
    idx = rng.integers(0, pc.shape[0], (P, 2)).astype(np.int32)
    idx[3] = idx[70] = (7, 7)
    out = np.empty((P, 2), np.float32)
    out[:, 0] = rng.uniform(-cfg.vote_range[0], cfg.vote_range[0], P)
    out[:, 1] = rng.uniform(0, cfg.vote_range[1], P)
    for k in range(3):
        w = (owner[idx[:, 0]] == k) & (owner[idx[:, 1]] == k)
        out[w] = syn.closed_form_outputs(pc, centers[k], idx[w], cfg, quantise=False)
    return cfg, pc, idx, out, np.array(centers)


def test_proposal_support_on_backvote_and_segmentation_outputs(dev):
    cfg, pc, idx, out, centers = _bowls()
    corners, dims = grid_shape(pc, cfg.res)
    d = _d(dev)
    tol = 3 * cfg.res
    worlds = np.concatenate([centers, centers[:1] + [0.5 * tol, 0, 0], corners[:1].astype(np.float64) - 5 * cfg.res]).astype(np.float32)
    d_pc, d_idx = d(pc), d(idx)
    bits = scene_stage.backvote_multi(d_pc, d(out), d_idx, d(corners[0]), cfg.res, dims, d(worlds), 72)
    for min_contrib in (0, 12):
        masks, _, _ = scene_stage.segment_instances(d_idx, bits, pc.shape[0], 5, min_contrib)
        got = scene_stage.proposal_support(d_idx, bits, masks).cpu().numpy()
        want = V.proposal_support(idx, bits.cpu().numpy().view(np.uint32), masks.cpu().numpy())
        assert np.array_equal(got, want), min_contrib
        if min_contrib == 0:
            # (something to count: on the host the restatement gives within 510..578 and agree 463..487 at the four centres in range)
            assert (want[:4, 0] > 100).all() and (2 * want[:4, 1] > want[:4, 0]).all() and want[:4, 2].all() and not want[4].any()


def _graph(dev, chain, outs):
    """eager (also the warm-up: scratch is allocated outside the capture), then a captured replay into poisoned outputs"""
    chain()
    torch.cuda.synchronize()
    eager = [t.cpu().numpy().copy() for t in outs]
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            chain()
    for t in outs:
        t.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    return eager, [t.cpu().numpy() for t in outs]


def test_proposal_support_graph_replay_equals_eager(dev):
    idx, bits, masks = _random_list(4099, 5, 1000, 0.3, seed=11)
    d = _d(dev)
    d_idx, d_bits, d_masks = d(idx), d(bits.view(np.int32)), d(masks)
    counts = torch.empty((5, 4), dtype=torch.int32, device=dev)
    eager, replay = _graph(dev, lambda: scene_stage.proposal_support(d_idx, d_bits, d_masks, out=counts), [counts])
    assert np.array_equal(eager[0], V.proposal_support(idx, bits, masks)) and np.array_equal(replay[0], eager[0])


def test_proposal_support_refusals(dev):
    L = _lib.lib()
    st = stream_ptr(dev)
    P, N, K = 64, 70, 5
    idx, bits, masks = _random_list(P, K, N, 0.3, seed=1)
    d = _d(dev)
    d_idx, d_bits, d_masks = d(idx), d(bits.view(np.int32)), d(masks)
    counts = torch.full((K, 4), -1, dtype=torch.int32, device=dev)
    need = L.cppf_proposal_support_workspace_bytes(N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    good = dict(idx=d_idx.data_ptr(), bits=d_bits.data_ptr(), masks=d_masks.data_ptr(), P=P, N=N, K=K, counts=counts.data_ptr(),
                ws=ws.data_ptr(), wsb=need)

    def run(**kw):
        a = dict(good, **kw)
        return L.cppf_proposal_support(a["idx"], a["bits"], a["masks"], a["P"], a["N"], a["K"], a["counts"], a["ws"], a["wsb"], st)
    for kw in (dict(K=0), dict(K=33), dict(N=0), dict(N=1 << 31), dict(P=-1), dict(P=1 << 27), dict(idx=None), dict(bits=None),
               dict(masks=None), dict(counts=None), dict(ws=None), dict(wsb=need - 1)):
        assert run(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == -1).all()                                 # a refused call writes nothing
    assert run() == 0
    assert np.array_equal(counts.cpu().numpy(), V.proposal_support(idx, bits, masks))
    assert run(P=0, idx=None, bits=None) == 0                                 # no pairs: zeros
    assert not counts.cpu().numpy().any()


# ----------------------------------------------------------------------------- cppf_box_support
def _rotations(rng, K):
    q, _ = np.linalg.qr(rng.standard_normal((K, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _box_case(N, K, seed):
    """uniform points in a 1 m cube and K boxes with random rotations: half extents from 0.05 m up, the last box holding everything
    and -- where there is room -- one box away from the cloud and one with negative half extents (both empty).  Points within BAND of
    a face (float64, relative to that half extent) are discarded and replaced; at most 5 % may be."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0.1, 0.9, (K, 3)).astype(np.float32)
    axes = _rotations(rng, K).reshape(K, 9).astype(np.float32)
    half = rng.uniform(0.05, 0.5, (K, 3)).astype(np.float32)
    half[K - 1] = 10.0
    if K >= 3:
        centers[0] = 5.0
        half[1] = -1.0
    cand = rng.random((N + max(64, N // 4), 3)).astype(np.float32)
    near = np.zeros(cand.shape[0], bool)
    for k in range(K):
        if (half[k] > 0).all():
            t = np.abs(V.box_coords(cand, centers[k], axes[k]))
            near |= (np.abs(t - half[k].astype(np.float64)) <= BAND * half[k]).any(axis=1)
    assert near.mean() <= 0.05, near.mean()
    pts = cand[~near][:N]
    assert pts.shape[0] == N and V.face_margin(pts, centers, axes, half) > BAND
    masks = (rng.random((K, N)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (K, N)).astype(np.uint8)
    return pts, masks, centers, axes, half


def _box(dev, pts, masks, centers, axes, half):
    d = _d(dev)
    K = masks.shape[0]
    buf = torch.full((3 * K + 16,), -7, dtype=torch.int32, device=dev)
    scene_stage.box_support(d(pts), d(masks), d(centers), d(axes), d(half), out=buf[8:8 + 3 * K].view(K, 3))
    got = buf.cpu().numpy()
    assert (got[:8] == -7).all() and (got[8 + 3 * K:] == -7).all()
    return got[8:8 + 3 * K].reshape(K, 3)


@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("N", [1, 63, 65, 4099])
def test_box_support_equals_the_float64_reference(dev, N, K):
    pts, masks, centers, axes, half = _box_case(N, K, seed=100 * K + N)
    want = V.box_support(pts, masks, centers, axes, half)
    got = _box(dev, pts, masks, centers, axes, half)
    assert np.array_equal(got, want), (N, K)
    assert want[K - 1, 2] == N                                                # the last box holds every point
    if K == 32:
        assert want[0, 2] == 0 and want[1, 2] == 0                            # the two empty boxes
        if N >= 63:                                                           # boxes that hold some points and not all of them
            assert ((want[2:31, 2] > 0) & (want[2:31, 2] < N)).any() and (want[2:31, 1] < want[2:31, 0]).any()
    # one non-finite point is in no box, the one that holds everything included; it stays a member of its masks
    for bad in (np.nan, np.inf):
        p2 = pts.copy()
        p2[N // 2, N % 3] = bad
        m2 = masks.copy()
        m2[:, N // 2] = 1
        want2 = V.box_support(p2, m2, centers, axes, half)
        assert want2[K - 1, 2] == N - 1 and want2[K - 1, 0] == m2[K - 1].astype(bool).sum() == want2[K - 1, 1] + 1
        assert np.array_equal(_box(dev, p2, m2, centers, axes, half), want2)


def test_box_support_graph_replay_and_refusals(dev):
    L = _lib.lib()
    st = stream_ptr(dev)
    N, K = 4099, 5
    pts, masks, centers, axes, half = _box_case(N, K, seed=9)
    d = _d(dev)
    t = dict(pts=d(pts), masks=d(masks), c=d(centers), A=d(axes), h=d(half))
    counts = torch.full((K, 3), -1, dtype=torch.int32, device=dev)
    good = dict({k: v.data_ptr() for k, v in t.items()}, N=N, K=K, counts=counts.data_ptr())

    def run(**kw):
        a = dict(good, **kw)
        return L.cppf_box_support(a["pts"], a["masks"], a["c"], a["A"], a["h"], a["N"], a["K"], a["counts"], st)
    for kw in (dict(K=0), dict(K=33), dict(N=0), dict(N=-1), dict(N=1 << 31), dict(pts=None), dict(masks=None), dict(c=None), dict(A=None),
               dict(h=None), dict(counts=None)):
        assert run(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == -1).all()
    want = V.box_support(pts, masks, centers, axes, half)
    eager, replay = _graph(dev, lambda: scene_stage.box_support(t["pts"], t["masks"], t["c"], t["A"], t["h"], out=counts), [counts])
    assert np.array_equal(eager[0], want) and np.array_equal(replay[0], want)


# ----------------------------------------------------------------------------- the known answer, the plumbing
@pytest.fixture(scope="module")
def scene():
    """two mugs with perfect heads: 80 000 pairs over 2 048 points (tests/scene_poses_ref.py)"""
    return S.perfect_scene("mug", 2, 1, pairs_per_object=40000, n_points=1024)


def test_true_centres_agree_and_decoys_do_not(dev, scene):
    """segment_proposals at the two true centres and two decoys -- midway between the objects, and the first centre shifted by six cells
    along x.  The restatement on the oracle's back-vote gives (on the host, where the decoys were fixed) agreement 0.999 / 0.999 at
    the true centres against 0.0 (an empty mask) / 0.847 at the decoys."""
    sc = scene
    cfg, pc, idx = sc["cfg"], sc["pc"], sc["idx"].astype(np.int32)
    c0, c1 = sc["obs"][0]["center"], sc["obs"][1]["center"]
    worlds = np.array([c0, c1, (c0 + c1) / 2, c0 + [6 * cfg.res, 0, 0]]).astype(np.float32).astype(np.float64)
    corners, dims = grid_shape(pc, cfg.res)
    d = _d(dev)
    d_pc, d_idx = d(pc), d(idx)
    masks, _, _, _, bits = scene_stage.segment_proposals(d_pc, d(sc["outputs"]), d_idx, d(corners[0]), cfg.res, dims, worlds, 72, None, 12)
    poses = []
    for k, w in enumerate(worlds):                                            # the object's own axis-aligned box at every centre
        o = sc["owner"] == (1 if k == 1 else 0)
        poses.append(dict(T=w, R=np.eye(3), scale=(pc[o].max(0) - pc[o].min(0)).astype(np.float64)))
    boxes = V.boxes_of(poses, cfg.res)
    assert V.face_margin(pc, boxes[:, 0:3], boxes[:, 3:12], boxes[:, 12:15]) > 1e-5       # (identity axes: fp32 cannot flip a point)
    got = scene_stage.verify_proposals(d_pc, d_idx, bits, masks, poses, cfg)
    want = V.verify(pc, idx, [b.cpu().numpy().view(np.uint32) for b in bits], masks.cpu().numpy(), poses, cfg.res)
    assert got == want
    agreement = [g["agreement"] for g in got]
    print("\nagreement at the true centres", agreement[:2], "at the decoys", agreement[2:])
    assert min(got[0]["within"], got[1]["within"]) > 10000
    assert min(agreement[:2]) > max(agreement[2:])
    assert got[0]["fill"] == got[1]["fill"] == 1.0 and got[0]["purity"] == 1.0 and got[3]["purity"] < 0.5
    # pad: the default is cfg.res
    assert got == scene_stage.verify_proposals(d_pc, d_idx, bits, masks, poses, cfg, pad=cfg.res)
    tight = scene_stage.verify_proposals(d_pc, d_idx, bits, masks, poses, cfg, pad=-0.01)
    assert tight == V.verify(pc, idx, [b.cpu().numpy().view(np.uint32) for b in bits], masks.cpu().numpy(), poses, cfg.res, pad=-0.01)
    assert tight[0]["mask_in_box"] < got[0]["mask_in_box"] and tight[0]["within"] == got[0]["within"]
    # a pose that is not finite: the pair counts stay, nothing is inside its box
    broken = [dict(p) for p in poses]
    broken[0]["R"] = np.full((3, 3), np.nan)
    b = scene_stage.verify_proposals(d_pc, d_idx, bits, masks, broken, cfg)
    assert b[0]["mask_in_box"] == b[0]["box_pts"] == 0 and b[0]["fill"] == 0.0 and b[0]["mask_pts"] == got[0]["mask_pts"]
    assert b[0]["agreement"] == got[0]["agreement"] and b[1:] == got[1:]


def test_verify_proposals_in_groups(dev, scene):
    """33 and 65 proposals: two and three groups of survivor words, every proposal equal to the restatement"""
    sc = scene
    cfg, pc, idx = sc["cfg"], sc["pc"], sc["idx"].astype(np.int32)[:20000]
    corners, dims = grid_shape(pc, cfg.res)
    rng = np.random.default_rng(4)
    lo = corners[0].astype(np.float64)
    worlds = rng.uniform(lo, lo + (np.array(dims) - 1) * cfg.res, (65, 3))
    worlds[[0, 32, 64]] = [sc["obs"][0]["center"], sc["obs"][1]["center"], sc["obs"][0]["center"]]
    worlds = worlds.astype(np.float32).astype(np.float64)
    d = _d(dev)
    d_pc, d_idx, d_out = d(pc), d(idx), d(sc["outputs"][:20000])
    for K in (33, 65):
        masks, _, _, _, bits = scene_stage.segment_proposals(d_pc, d_out, d_idx, d(corners[0]), cfg.res, dims, worlds[:K], 72, None, 3)
        assert len(bits) == (K + 31) // 32
        poses = [dict(T=w, R=np.eye(3), scale=np.full(3, 0.0997)) for w in worlds[:K]]
        got = scene_stage.verify_proposals(d_pc, d_idx, bits, masks, poses, cfg)
        want = V.verify(pc, idx, [b.cpu().numpy().view(np.uint32) for b in bits], masks.cpu().numpy(), poses, cfg.res)
        assert len(got) == K
        for k in range(K):
            assert {n: got[k][n] for n in V.COUNTS[:5]} == {n: want[k][n] for n in V.COUNTS[:5]}, (K, k)
        assert got[32]["within"] > 100                                        # the second group holds a real object
        with pytest.raises(ValueError, match="survivor-word"):
            scene_stage.verify_proposals(d_pc, d_idx, bits[:1], masks, poses, cfg)


POSE_KEYS = ("T", "R", "up", "scale", "RT", "point_mask")


def _same_poses(a, b, keys):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        for key in keys:
            assert np.array_equal(p[key], q[key]), key
        assert p["n_pairs"] == q["n_pairs"]


def test_scene_poses_with_verify(dev, scene):
    sc = scene
    cfg, d = sc["cfg"], _d(dev)
    d_pc, d_idx = d(sc["pc"]), d(sc["idx"])
    run = lambda **kw: scene_poses.scene_poses(None, d_pc, d(sc["nrm"]), None, d_idx, None, None, cfg, outputs=d(sc["outputs"]),
                                               heads=d(sc["heads"]), max_proposals=4, **kw)
    plain, ver = run(), run(verify=True)
    assert len(plain["poses"]) >= 2
    _same_poses(plain["poses"], ver["poses"], POSE_KEYS)
    assert all(p["scale_norm"] == q["scale_norm"] for p, q in zip(plain["poses"], ver["poses"]))
    assert torch.equal(plain["pairs"], ver["pairs"]) and np.array_equal(plain["offsets"], ver["offsets"])
    assert torch.equal(plain["surv_bits"], ver["surv_bits"])
    assert all("verify" not in p for p in plain["poses"]) and set(ver["poses"][0]) == set(plain["poses"][0]) | {"verify"}
    assert set(plain) == set(ver)
    masks = d(np.stack([p["point_mask"] for p in ver["poses"]]).astype(np.uint8))
    idx32 = d_idx.to(torch.int32).contiguous()
    by_hand = scene_stage.verify_proposals(d_pc, idx32, [ver["surv_bits"]], masks, ver["poses"], cfg)
    assert [p["verify"] for p in ver["poses"]] == by_hand
    want = V.verify(sc["pc"], sc["idx"], [ver["surv_bits"].cpu().numpy().view(np.uint32)], masks.cpu().numpy(), ver["poses"], cfg.res)
    for g, w in zip(by_hand, want):
        assert {n: g[n] for n in V.COUNTS[:5]} == {n: w[n] for n in V.COUNTS[:5]}
    m = S.match_objects(ver["proposals"][0], ver["corner"], cfg.res, [o["center"] for o in sc["obs"]])
    assert None not in m and all(ver["poses"][k]["verify"]["agreement"] > 0.95 for k in m)


def test_zero_shot_scene_with_verify(dev, scene):
    sc = scene
    cfg, d = sc["cfg"], _d(dev)
    preds = np.concatenate([sc["outputs"], sc["heads"][:, :7]], axis=1).astype(np.float32)     # mu nu | up right | aux, aux | scales
    d_pc, d_idx, d_preds = d(sc["pc"]), d(sc["idx"]), d(preds)
    run = lambda **kw: zero_shot.zero_shot_scene(None, d_pc, d(sc["nrm"]), None, d_idx, cfg, preds=d_preds, max_proposals=4, **kw)
    plain, ver = run(), run(verify=True)
    assert len(plain["poses"]) >= 2 and set(plain) == set(ver)
    _same_poses(plain["poses"], ver["poses"], ("T", "R", "up", "scale_3d", "RT", "point_mask"))
    assert all("verify" not in p for p in plain["poses"]) and set(ver["poses"][0]) == set(plain["poses"][0]) | {"verify"}
    assert [p["verify"] for p in zero_shot.zero_shot_poses(None, d_pc, d(sc["nrm"]), None, d_idx, cfg, preds=d_preds, max_proposals=4,
                                                           verify=True)] == [p["verify"] for p in ver["poses"]]
    idx32 = d_idx.to(torch.int32).contiguous()
    masks, _, _, _, bits = scene_stage.segment_proposals(d_pc, d_preds[:, :2].contiguous(), idx32, d(np.asarray(ver["corner"], np.float32)),
                                                         cfg.res, ver["dims"], np.stack([p["T"] for p in ver["poses"]]), 72, None, 12)
    assert np.array_equal(masks.cpu().numpy().astype(bool), np.stack([p["point_mask"] for p in ver["poses"]]))
    by_hand = scene_stage.verify_proposals(d_pc, idx32, bits, masks, ver["poses"], cfg)
    assert [p["verify"] for p in ver["poses"]] == by_hand
    boxes = scene_stage.verify_boxes(ver["poses"], cfg)                        # the zero-shot box: scale_3d, not the norm `scale`
    for p, row in zip(ver["poses"], boxes):
        assert np.array_equal(row[12:], (np.asarray(p["scale_3d"]) / 2 + cfg.res).astype(np.float32))


@pytest.fixture(scope="module")
def frame(dev):
    from cppf_amd.frames import NOCS_INTRINSICS
    from cppf_amd.utils.util import read_depth_png
    depth = read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))
    nets = {}
    for cat in ("bottle", "mug"):
        cfg = CATEGORIES[cat]
        penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
        nets[cat] = (penc, enc, cfg)
    return depth, NOCS_INTRINSICS, nets


def _ids(res):
    return [(d["category"], d["proposal"]) for d in res["detections"]]


def test_frame_detections_with_agreement(frame, dev):
    depth, K, nets = frame
    names, cfgs = list(nets), [cfg for _, _, cfg in nets.values()]
    outs = [scene_poses.scene_frame(depth, K, enc, penc, cfg, verify=True, **FRAME_KW) for penc, enc, cfg in nets.values()]
    ag = sorted(p["verify"]["agreement"] for o in outs for p in o["poses"])
    assert len(ag) >= 1
    bound = 0.5 * (ag[0] + ag[-1]) if ag[0] < ag[-1] else ag[0]               # between the lowest and the highest: a filter that bites
    for kw in (dict(score="agreement"), dict(score="agreement", min_agreement=bound), dict(min_fill=0.5, min_within=10),
               dict(score="agreement", cross_category=True)):
        got = detections.frame_detections(depth, K, nets, **FRAME_KW, **kw)
        want = detections.pool_detections(outs, names, cfgs, device=dev, **kw)
        assert _ids(got) == _ids(want) and got["filtered"] == want["filtered"], kw
        # (integer counts: the agreement is the same number on every run; a vote height agrees to rounding, tests/test_gpu_detections.py)
        assert np.allclose([d["score"] for d in got["detections"]], [d["score"] for d in want["detections"]], rtol=1e-4)
        assert got["kept_per_category"] == want["kept_per_category"] and got["suppressed"] == want["suppressed"]
        assert all("verify" in p for o in got["outs"] for p in o["poses"])
        for dg, dw in zip(got["detections"], want["detections"]):
            assert dg["pose"]["verify"] == dw["pose"]["verify"] and np.array_equal(dg["RT"], dw["RT"])
        if kw.get("score") == "agreement":
            assert [d["score"] for d in got["detections"]] == [d["pose"]["verify"]["agreement"] for d in got["detections"]]
            assert [d["score"] for d in got["detections"]] == [d["score"] for d in want["detections"]]
    if ag[0] < ag[-1]:
        f = detections.frame_detections(depth, K, nets, **FRAME_KW, score="agreement", min_agreement=bound)
        assert sum(f["filtered"].values()) > 0 and all(d["score"] >= bound for d in f["detections"])


def test_frame_detections_defaults_are_unchanged(frame, dev):
    depth, K, nets = frame
    names, cfgs = list(nets), [cfg for _, _, cfg in nets.values()]
    outs = [scene_poses.scene_frame(depth, K, enc, penc, cfg, **FRAME_KW) for penc, enc, cfg in nets.values()]
    old = detections.pool_detections(outs, names, cfgs, 0.3, False, "diff", device=dev)            # the call as it was
    got = detections.frame_detections(depth, K, nets, **FRAME_KW)
    assert set(got) == set(old) | {"outs"} and "filtered" not in got
    assert set(old) == {"detections", "kept_per_category", "suppressed", "proposals_per_category", "result", "cfgs"}
    assert _ids(got) == _ids(old)
    for key in ("kept_per_category", "suppressed", "proposals_per_category"):
        assert got[key] == old[key], key
    for dg, do in zip(got["detections"], old["detections"]):
        assert set(dg) == set(do) and set(dg["pose"]) == set(do["pose"]) and "verify" not in dg["pose"]
        assert np.array_equal(dg["RT"], do["RT"]) and np.array_equal(dg["scales"], do["scales"])
    for key in ("pred_class_ids", "pred_RTs", "pred_scales"):
        assert np.array_equal(got["result"][key], old["result"][key]), key
    # (the scores are heights of an fp32 atomic vote: equal to rounding from run to run, as tests/test_gpu_detections.py notes)
    assert np.allclose(got["result"]["pred_scores"], old["result"]["pred_scores"], rtol=1e-4)
    with pytest.raises(ValueError, match="verify=True"):
        detections.pool_detections(outs, names, cfgs, score="agreement", device=dev)
