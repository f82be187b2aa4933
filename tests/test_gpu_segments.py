"""csrc/segments.hip on the device against tests/segments_ref.py: the labelling bit for bit (every output array; labels, first and
sizes where no overflow occurred), the plane fit's planes against the fp32 restatement, its counts EXACTLY against the restatement
evaluated on the device's own planes, its arg-max exactly from the counts.  Depths are millimetres."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_ref as R  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from cppf_amd import segments as SG  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("labels", "comp_size", "first", "sizes", "counts")


def _run(dev, depth, valid=None, **kw):
    d = torch.from_numpy(np.ascontiguousarray(depth, np.uint16).view(np.int16)).to(dev)
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).to(dev)
    return {k: t.cpu().numpy() for k, t in SG.depth_segments_device(d, v, **kw).items()}


def _check(dev, depth, valid=None, **kw):
    """the kernel's five arrays against the restatement's; returns the restatement"""
    kw = dict(dict(tol_mm=10, slope_permille=10, min_pixels=1, max_pixels=0, capacity=256), **kw)
    got, want = _run(dev, depth, valid, **kw), R.segments_ref(depth, valid, **kw)
    for k in ("counts", "comp_size") + (() if want["overflow"] else ("labels", "first", "sizes")):
        assert np.array_equal(got[k], want[k]), (k, np.asarray(depth).shape, kw, got["counts"], want["counts"])
    return want


LINES = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("shape", [(1, w) for w in LINES] + [(h, 1) for h in LINES[1:]] + [(7, 9), (33, 65), (64, 64), (65, 129), (100, 257)])
def test_sizes(dev, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    d = (rng.choice([700, 900, 1400], shape) + rng.integers(-5, 6, shape)).astype(np.uint16)
    d[rng.random(shape) < 0.15] = 0
    if shape == (1, 1):
        for z, live in ((1000, 1), (0, 0)):
            w = _check(dev, np.full(shape, z, np.uint16))
            assert w["counts"].tolist() == [live, live, live, 0]
        return
    w = _check(dev, d)
    assert w["counts"][1] >= 1
    _check(dev, np.full(shape, 1000, np.uint16), min_pixels=shape[0] * shape[1])       # one component over every tile, root 0
    _check(dev, d, min_pixels=3, max_pixels=40, capacity=1024)


H, W = 65, 129


def _cut_mask():
    v = np.ones((H, W), np.uint8)
    v[:, 64] = 0
    return v


@pytest.mark.parametrize("name", ["flat", "checkerboard", "h_stripes", "v_stripes", "serpentine", "comb", "valid_cut"])
def test_patterns(dev, name):
    kw, valid = dict(capacity=1024), None
    if name == "flat":
        d = np.full((H, W), 1000, np.uint16)
    elif name == "checkerboard":
        d, kw = R.checkerboard(H, W), dict(capacity=8)                         # 4193 components of one pixel: overflow
    elif name == "h_stripes":
        d = np.repeat((1000 + 40 * (np.arange(H) % 3))[:, None], W, 1).astype(np.uint16)
    elif name == "v_stripes":
        d = np.repeat((1000 + 40 * (np.arange(W) % 3))[None, :], H, 0).astype(np.uint16)
    elif name == "serpentine":
        d = R.serpentine(H, W)
    elif name == "comb":
        d = R.comb(H, W)
    else:
        d, valid = np.full((H, W), 1000, np.uint16), _cut_mask()
    w = _check(dev, d, valid, **kw)
    n = {"flat": 1, "checkerboard": (H * W + 1) // 2, "h_stripes": H, "v_stripes": W, "serpentine": 1, "comb": 1, "valid_cut": 2}[name]
    assert w["counts"][1] == n
    if n == 1:
        assert w["first"][0] == 0 and w["sizes"][0] == w["counts"][2]          # the root's label travelled the whole component
    if name == "serpentine":
        assert w["counts"][2] == 33 * W + 32 and d[0, 0] and not d[1, 0]
    if name == "valid_cut":
        assert w["first"][:2].tolist() == [0, 65] and w["sizes"][:2].tolist() == [H * 64, H * 64]


def test_link_rule(dev):
    row = lambda *z: np.array([z], np.uint16)
    comps = lambda d, **kw: _check(dev, d, **kw)["counts"][1]
    assert comps(row(1000, 1010), slope_permille=0) == 1 and comps(row(1000, 1011), slope_permille=0) == 2
    assert comps(row(1000, 1020)) == 1 and comps(row(1000, 1021)) == 2          # slope 10 permille of 1000: + 10
    assert comps(row(999, 1018)) == 1 and comps(row(999, 1019)) == 2            # of 999: + 9 (the floor)
    assert comps(row(40000, 40005), slope_permille=0) == 1                      # beyond the int16 range: compared unsigned
    assert comps(row(40000, 40005), tol_mm=4, slope_permille=0) == 2
    col = np.array([[1000], [1010], [1021], [0], [1021]], np.uint16)
    assert comps(col, slope_permille=0) == 3


def _blobs(sizes, gap=2):
    """one row-run per size, separated by dead pixels, wrapped into a 40-wide image row by row (a run never wraps)"""
    Wb = 40
    rows, cur = [], []
    for s in sizes:
        assert s <= Wb
        if len(cur) + s > Wb:
            rows.append(cur + [0] * (Wb - len(cur)))
            rows.append([0] * Wb)
            cur = []
        cur += [1000] * s + [0] * min(gap, Wb - len(cur) - s)
    rows.append(cur + [0] * (Wb - len(cur)))
    return np.array(rows, np.uint16)


def test_filters_and_capacity(dev):
    d = _blobs([4, 5, 9, 10, 7])
    w = _check(dev, d, min_pixels=5, max_pixels=9)                             # min - 1, min, max, max + 1, between
    assert w["sizes"][:w["counts"][0]].tolist() == [5, 9, 7] and w["counts"][1] == 5
    d = _blobs([3] * 9)
    w = _check(dev, d, capacity=9)                                             # S == capacity
    assert w["counts"][0] == 9 and not w["overflow"]
    w = _check(dev, d, capacity=8)                                             # S == capacity + 1
    assert w["overflow"] and w["counts"].tolist() == [9, 9, 27, 0]
    s = SG.depth_segments(d, min_pixels=1, capacity=8)                         # the wrapper's retry
    full = R.segments_ref(d, min_pixels=1, capacity=9)
    assert s["n_segments"] == 9 and s["n_components"] == 9 and s["n_live"] == 27
    assert np.array_equal(s["labels"].cpu().numpy(), full["labels"]) and np.array_equal(s["first"].cpu().numpy(), full["first"])
    assert np.array_equal(s["sizes"].cpu().numpy(), full["sizes"]) and np.array_equal(s["comp_size"].cpu().numpy(), full["comp_size"])
    with pytest.raises(ValueError, match="1152"):
        SG.depth_segments(R.checkerboard(48, 48), min_pixels=1)


@pytest.mark.parametrize("seed", range(10))
def test_random_images(dev, seed):
    d = R.levels_image(seed)
    w = _check(dev, d, min_pixels=1 + seed % 3, capacity=1024)
    assert w["counts"][1] > 10
    _check(dev, d, min_pixels=20, max_pixels=(0 if seed % 2 else 400), capacity=64)


@pytest.fixture(scope="module")
def demo():
    from cppf_amd.utils.util import read_depth_png
    return read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))


def test_demo_frame(dev, demo):
    assert demo.shape == (480, 640)
    w = _check(dev, demo, min_pixels=200)
    assert w["counts"][1] == 9 and w["counts"][2] == 215686 and w["sizes"].max() == 206920             # the frame is one blob
    valid = np.ones(demo.shape, np.uint8)
    valid[200:203, :] = 0
    valid[:, 300] = 0
    w2 = _check(dev, demo, valid, min_pixels=200)
    assert w2["counts"][2] < w["counts"][2] and w2["counts"][0] > w["counts"][0]
    s = SG.depth_segments(demo, valid.astype(bool), min_pixels=200)
    assert s["n_segments"] == w2["counts"][0] and np.array_equal(s["labels"].cpu().numpy(), w2["labels"])


def _graph(dev, chain, outs):
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


def test_segments_same_bits_and_graph_replay(dev):
    d = R.levels_image(77, 100, 257)
    runs = [_run(dev, d, min_pixels=2, capacity=1024) for _ in range(3)]
    for r in runs[1:]:
        for k in KEYS:
            assert np.array_equal(r[k], runs[0][k]), k
    dd = torch.from_numpy(d.view(np.int16)).to(dev)
    out = SG.depth_segments_device(dd, None, min_pixels=2, capacity=1024)
    outs = [out[k] for k in KEYS]
    eager, replay = _graph(dev, lambda: SG.depth_segments_device(dd, None, min_pixels=2, capacity=1024, out=out), outs)
    for k, e, r in zip(KEYS, eager, replay):
        assert np.array_equal(e, runs[0][k]) and np.array_equal(r, e), k


# ------------------------------------------------------------------------------------------------------------------- the plane fit
def _plane_check(dev, pts, n_hyp, thresh, seed):
    """planes against the fp32 restatement bit for bit (NaN-free by construction: degenerate rows are zeros), counts exactly on the
    device's own planes, best exactly from the counts; returns (planes, counts, best) as numpy"""
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev)
    planes, counts, best = (t.cpu().numpy() for t in SG.plane_ransac_device(p, n_hyp, thresh, seed))
    want = R.planes_ref(pts, n_hyp, seed)
    assert np.array_equal(planes.view(np.uint32) & 0x7FFFFFFF == 0, want.view(np.uint32) & 0x7FFFFFFF == 0)       # the same zeros
    assert np.array_equal(planes.view(np.uint32), want.view(np.uint32)), np.abs(planes - want).max()
    assert np.array_equal(counts, R.counts_ref(pts, planes, thresh))
    assert np.array_equal(best, R.best_ref(planes, counts))
    return planes, counts, best


def _plane_cloud(N, seed, inlier_frac=0.6):
    """inlier_frac of the points on the plane n.p = 1.2 (|n| = 1) with 2 mm noise, the rest uniform in a 2 m cube"""
    rng = np.random.default_rng(seed)
    n = np.array([0.2, -0.5, 0.8])
    n /= np.linalg.norm(n)
    k = int(N * inlier_frac)
    u, v = np.cross(n, [1, 0, 0]), None
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    on = 1.2 * n + rng.uniform(-1, 1, (k, 1)) * u + rng.uniform(-1, 1, (k, 1)) * v + 0.002 * rng.standard_normal((k, 1)) * n
    pts = np.concatenate([on, rng.uniform(-1, 1, (N - k, 3)) + [0, 0, 1.0]]).astype(np.float32)
    return pts[rng.permutation(N)], n


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 1000, 100003])
def test_plane_point_counts(dev, N):
    pts, _ = _plane_cloud(max(N, 4), N)
    pts = pts[:N]
    planes, counts, best = _plane_check(dev, pts, 64, 0.01, seed=N)
    if N == 1:
        assert not planes.any() and not counts.any() and best.tolist() == [-1, 0]
    if N == 3:                                                                 # the one plane or a repeated point: a tie, lowest index
        ok = planes[:, :3].any(-1)
        assert ok.any() and (counts[ok] == 3).all() and best.tolist() == [int(np.nonzero(ok)[0][0]), 3]


@pytest.mark.parametrize("n_hyp", [1, 64, 65, 1024])
def test_plane_hypothesis_counts(dev, n_hyp):
    pts, _ = _plane_cloud(5000, 9)
    _plane_check(dev, pts, n_hyp, 0.01, seed=n_hyp)


def test_plane_found_among_outliers(dev):
    pts, n = _plane_cloud(20000, 4)
    planes, counts, best = _plane_check(dev, pts, 256, 0.01, seed=1)
    pl = planes[best[0]]
    assert pl[3] >= 0 and best[1] > 0.5 * 20000
    cosang = abs(float(pl[:3] @ (-n)))                                         # the truth written with d >= 0: {-n, 1.2}
    assert cosang >= np.cos(np.deg2rad(1.0)) and abs(float(pl[3]) - 1.2) <= 0.01
    r = SG.plane_ransac(pts, 256, 0.01, seed=1)
    assert r["index"] == best[0] and r["count"] == best[1] and np.array_equal(r["plane"], pl)


def test_plane_edge_values(dev):
    line = (np.arange(50, dtype=np.float32)[:, None] * np.array([[1, 2, 3]], np.float32))
    planes, counts, best = _plane_check(dev, line, 65, 0.01, seed=2)
    assert not planes.any() and best.tolist() == [-1, 0]                       # collinear: every hypothesis degenerate
    pts, _ = _plane_cloud(1000, 5)
    bad = pts.copy()
    bad[::7, 0], bad[3::7, 2], bad[5::7, 1] = np.nan, np.inf, -np.inf
    planes, counts, _ = _plane_check(dev, bad, 128, 0.05, seed=3)
    fin = np.isfinite(bad).all(-1)
    ok = planes[:, :3].any(-1)
    assert ok.any() and (~ok).any()                                            # a hypothesis that drew a non-finite point is degenerate
    assert np.array_equal(counts, R.counts_ref(bad[fin], planes, 0.05))        # NaN / inf points are counted nowhere
    # a point at exactly thresh: the plane z = 2 from three exact points, a fourth at z = 2.5 with thresh 0.5 (all exact in fp32)
    tri = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2], [0.25, 0.25, 2.5], [0.25, 0.25, 2.5000002]], np.float32)
    planes, counts, _ = _plane_check(dev, tri, 256, 0.5, seed=4)
    flat = np.all(planes == np.array([0, 0, -1, 2], np.float32), -1)
    assert flat.any() and (counts[flat] == 4).all()


def test_plane_same_bits_and_graph_replay(dev):
    pts, _ = _plane_cloud(30011, 6)
    p = torch.from_numpy(pts).to(dev)
    first = [t.cpu().numpy() for t in SG.plane_ransac_device(p, 300, 0.01, 8)]
    for _ in range(2):
        for a, b in zip(first, SG.plane_ransac_device(p, 300, 0.01, 8)):
            assert np.array_equal(a, b.cpu().numpy())
    out = (torch.empty((300, 4), dtype=torch.float32, device=dev), torch.empty(300, dtype=torch.int32, device=dev),
           torch.empty(2, dtype=torch.int32, device=dev))
    eager, replay = _graph(dev, lambda: SG.plane_ransac_device(p, 300, 0.01, 8, out=out), list(out))
    for a, e, r in zip(first, eager, replay):
        assert np.array_equal(a, e) and np.array_equal(e, r)


def test_support_mask_and_frame_segments_on_the_demo_frame(dev, demo):
    """the device path reproduces what the frame is known to hold: one blob without plane removal, and a first plane of about 81 000
    inliers whose removal breaks it up (the counts themselves depend on the RANSAC draw and are measured, not pinned: DESIGN.md 3.7j)"""
    from cppf_amd.frames import NOCS_INTRINSICS
    s0 = SG.frame_segments(demo, NOCS_INTRINSICS, n_planes=0)
    assert s0["valid"] is None and s0["planes"] == [] and s0["n_components"] == 9 and int(s0["sizes"].max()) == 206920
    s2 = SG.frame_segments(demo, NOCS_INTRINSICS, n_planes=2)
    assert len(s2["planes"]) == 2 and s2["options"]["n_planes"] == 2
    valid = s2["valid"].cpu().numpy()
    want = R.segments_ref(demo, valid, min_pixels=200, capacity=max(s2["n_segments"], 1))
    assert np.array_equal(s2["labels"].cpu().numpy(), want["labels"]) and s2["n_components"] == want["counts"][1]
    assert int(s2["sizes"].max()) < 60000 and s2["n_segments"] >= 5
    p = torch.from_numpy(np.zeros((1, 3), np.float32)).to(dev)
    for pl in s2["planes"]:
        assert pl[3] >= 0 and abs(np.linalg.norm(pl[:3]) - 1) < 1e-5
        assert SG.off_planes(p, [pl], 0.015).item() == (pl[3] > 0.015)
