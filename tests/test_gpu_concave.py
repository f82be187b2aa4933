"""csrc/concave.hip on the device against tests/concave_ref.py: edge, normal and counts bit for bit at every size at which the kernels
take another path (the 32 x 8 tile of the fit, the 256-pixel blocks and 64-lane ballots of the other two), at the caps of the
options, at the rule's own edges (the gate, min_count, a collinear window), on the demo frame; the same bits on every run and from a
graph; the refusals; and frame_segments(concave=) against its hand composition.  Depths are millimetres."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concave_ref as C  # noqa: E402
import segments_ref as R  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from cppf_amd import segments as SG  # noqa: E402
from cppf_amd._torch_util import call  # noqa: E402
from cppf_amd.frames import NOCS_INTRINSICS  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("edge", "normal", "counts")
TILE_W, TILE_H = 32, 8                                                        # csrc/concave.hip: CC_TW, CC_TH
K = np.asarray(NOCS_INTRINSICS, np.float64)


def _cam(H, W):
    """a camera that sees an H x W image about as the NOCS camera sees its own (the principal point at the image centre)"""
    return np.array([[K[0, 0], 0, (W - 1) / 2], [0, K[1, 1], (H - 1) / 2], [0, 0, 1]])


def _run(dev, depth, valid=None, cam=None, **kw):
    depth = np.ascontiguousarray(depth, np.uint16)
    d = torch.from_numpy(depth.view(np.int16)).to(dev)
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).to(dev)
    return {k: t.cpu().numpy() for k, t in SG.concave_edges_device(d, _cam(*depth.shape) if cam is None else cam, v, **kw).items()}


def _check(dev, depth, valid=None, cam=None, **kw):
    """the kernel's three arrays against the restatement's, bit for bit; returns the restatement"""
    depth = np.asarray(depth, np.uint16)
    cam = _cam(*depth.shape) if cam is None else cam
    o = SG.concave_options(**kw)
    got, want = _run(dev, depth, valid, cam, **kw), C.concave_ref(depth, valid, cam[0, 0], cam[1, 1], cam[0, 2], cam[1, 2], **o)
    where = (depth.shape, o, got["counts"], want["counts"])
    assert np.array_equal(got["counts"], want["counts"]), where
    assert np.array_equal(got["edge"], want["edge"]), where
    assert got["normal"].shape == want["normal"].shape and np.array_equal(got["normal"].view(np.uint64), want["normal"].view(np.uint64)), where
    return want


def _image(seed, H, W, valid=True):
    d, v = C.planar_image(seed, H, W)
    return d, (v if valid else None)


LINES = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("shape", [(1, w) for w in LINES] + [(h, 1) for h in LINES[1:]])
def test_lines(dev, shape):
    if shape == (1, 1):
        for z, live in ((1000, 1), (0, 0)):
            w = _check(dev, np.full(shape, z, np.uint16), min_count=3)
            assert w["counts"].tolist() == [0, 0, live, 0] and not w["normal"].any()
        return
    d, _ = _image(shape[0] + shape[1], *shape)
    w = _check(dev, d, radius=2, step=1, min_count=3)
    assert w["counts"][1] == 0 and w["counts"][2] > 0                          # a line of pixels is collinear: D = 0 everywhere
    _check(dev, d, radius=8, step=16, min_count=3)


@pytest.mark.parametrize("shape", [(7, 9), (33, 65), (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1),
                                   (2 * TILE_H + 1, 2 * TILE_W + 1), (TILE_H + 1, TILE_W - 1), (2 * TILE_H + 1, TILE_W), (3, 257)])
def test_sizes(dev, shape):
    d, v = _image(shape[0] * 1000 + shape[1], *shape)
    w = _check(dev, d, v, radius=2, step=2, min_count=8, cos_max=0.95, span_max=0.2)
    assert w["counts"][2] > 0 and (shape[0] < 5 or w["counts"][1] > 0)
    _check(dev, d, None)                                                       # the defaults: radius 3, step 4
    _check(dev, np.full(shape, 1000, np.uint16), radius=1, step=1, min_count=4)


@pytest.mark.parametrize("seed", range(10))
def test_random_images(dev, seed):
    d, v = _image(seed, 67, 131)
    w = _check(dev, d, v, radius=1 + seed % 4, step=1 + seed % 5, min_count=3 + seed % 5, cos_max=0.9 + 0.008 * seed, span_max=0.05 + 0.02 * seed)
    assert 0 < w["counts"][1] <= w["counts"][2]
    _check(dev, d, None, radius=2, step=2, min_count=8, cos_max=0.97, span_max=0.3)


def test_random_images_mark_edges(dev):
    """the ten images above hold creases: the comparison is not between two empty masks"""
    tot = sum(C.concave_ref(*_image(s, 67, 131), K[0, 0], K[1, 1], 65.0, 33.0, radius=2, step=2, min_count=8, cos_max=0.97, span_max=0.3)["counts"][0]
              for s in range(10))
    assert tot > 100


@pytest.mark.parametrize("kw", [dict(radius=1, step=1, min_count=3), dict(radius=8, step=1, min_count=3), dict(radius=1, step=16, min_count=4),
                                dict(radius=8, step=16, min_count=96), dict(radius=8, step=16, min_count=3, tol_mm=65535, slope_permille=1000)])
def test_option_caps_on_a_small_image(dev, kw):
    """40 x 40: at radius 8 most windows leave the frame, at step 16 only the middle 8 x 8 pixels have both neighbours"""
    d, v = _image(40, 40, 40)
    w = _check(dev, d, v, cos_max=0.97, span_max=0.5, **kw)
    assert w["counts"][1] > 0
    _check(dev, d, None, cos_max=-0.999, span_max=1e-9, **kw)
    _check(dev, d, None, cos_max=0.999999, span_max=1e9, **kw)


def test_more_tile_rows_than_a_grid_dimension_takes(dev):
    """a frame two pixels wide and 8 x 65536 + 3 high: 65537 rows of tiles (they are numbered along one grid dimension)"""
    Ht = TILE_H * 65536 + 3
    yy = np.arange(Ht)[:, None]
    d = (1000 + (yy % 50) * 3 + np.array([[0, 2]])).astype(np.uint16)
    d[::97, 0] = 0
    w = _check(dev, d, radius=1, step=1, min_count=4)
    assert w["counts"][1] > Ht and w["normal"][-1].any() and w["normal"][65536 * TILE_H - 1].any()


def test_valid_mask_cuts_a_plane(dev):
    yy, xx = np.mgrid[:33, :70]
    d = (900 + 3 * xx + 2 * yy).astype(np.uint16)
    valid = np.ones(d.shape, np.uint8)
    valid[:, 35] = 0
    valid[16, :20] = 0
    w = _check(dev, d, valid, radius=3, step=4)
    full = _check(dev, d, None, radius=3, step=4)
    assert w["counts"][2] == d.size - 33 - 20 + 0 and full["counts"][2] == d.size
    assert not w["normal"][:, 35].any() and full["normal"][:, 35].any() and w["counts"][0] == 0 == full["counts"][0]
    # the windows beside the cut lose pixels but keep their plane: the same normal up to rounding, not the same sums
    assert np.abs(w["normal"][5, 34] - full["normal"][5, 34]).max() < 1e-9


def test_depths_at_the_top_of_the_range(dev):
    d = np.full((20, 40), 65535, np.uint16)
    w = _check(dev, d, radius=3, step=2)
    assert w["counts"][1] == 800                                               # compared unsigned: 65535 is a depth, not -1
    d[::2, ::3] = 65534
    d[5:9, 10:30] = 1
    _check(dev, d, radius=8, step=3, tol_mm=65535, slope_permille=1000, min_count=3, span_max=100.0)
    _check(dev, d, radius=2, step=1, tol_mm=0, slope_permille=0, min_count=3)


def test_all_dead(dev):
    for shape in ((1, 1), (9, 33), (17, 300)):
        w = _check(dev, np.zeros(shape, np.uint16), radius=2, step=1, min_count=3)
        assert not w["counts"].any() and not w["edge"].any() and not w["normal"].any()
    d, _ = _image(3, 17, 65)
    w = _check(dev, d, np.zeros(d.shape, np.uint8))
    assert not w["counts"].any()


def test_the_gate(dev):
    """tol 10, slope 0: lim = 10.  A plane rising 10 mm per column is admitted whole (|dz| = 10 |du| <= 10 max(|du|, |dv|, 1)); at 11 mm
    per column a window of radius 1 keeps its own column alone -- collinear, no fit -- while one of radius 2 still admits the pixels
    with |dv| > |du|.  With slope 10 permille at 1000 mm: lim = 20."""
    yy, xx = np.mgrid[:12, :40]
    at = _check(dev, (1000 + 10 * xx).astype(np.uint16), radius=1, step=1, tol_mm=10, slope_permille=0, min_count=3)
    beyond = _check(dev, (1000 + 11 * xx).astype(np.uint16), radius=1, step=1, tol_mm=10, slope_permille=0, min_count=3)
    assert at["counts"].tolist() == [0, 480, 480, 0] and beyond["counts"].tolist() == [0, 0, 480, 0]
    assert C.sums_ref((1000 + 10 * xx).astype(np.uint16), None, 1, 10, 0)[0][5, 5] == 9
    assert C.sums_ref((1000 + 11 * xx).astype(np.uint16), None, 1, 10, 0)[0][5, 5] == 3
    assert _check(dev, (1000 + 11 * xx).astype(np.uint16), radius=2, step=1, tol_mm=10, slope_permille=0, min_count=3)["counts"][1] == 480
    d = np.full((9, 9), 1000, np.uint16)
    d[4, 5], d[4, 3] = 1020, 979                                               # one at the gate, one a millimetre beyond
    S = C.sums_ref(d, None, 1, 10, 10)
    assert S[0][4, 4] == 8
    _check(dev, d, radius=1, step=1, min_count=3)
    _check(dev, d, radius=1, step=1, min_count=9)


def test_min_count(dev):
    """a flat 5 x 5 image at radius 1: windows of 9 (inside), 6 (sides) and 4 (corners) pixels"""
    d = np.full((5, 5), 1000, np.uint16)
    assert _check(dev, d, radius=1, step=1, min_count=6)["counts"][1] == 21    # n = min_count fits
    assert _check(dev, d, radius=1, step=1, min_count=7)["counts"][1] == 9     # n = min_count - 1 does not
    assert _check(dev, d, radius=1, step=1, min_count=4)["counts"][1] == 25
    assert _check(dev, d, radius=1, step=1, min_count=10)["counts"][1] == 0


def test_collinear_window(dev):
    d = np.zeros((9, 40), np.uint16)
    d[4, :] = 1000
    d[:, 7] = 1000                                                             # a cross: its arms are collinear, its centre is not
    w = _check(dev, d, radius=2, step=1, min_count=3)
    fit = w["normal"].any(-1)
    assert w["counts"][2] == 48 and fit[4, 7] and not fit[4, 20] and not fit[0, 7] and 0 < w["counts"][1] < 48


def test_a_crease_is_marked_and_a_ridge_is_not(dev):
    """two planes that meet in a vertical line, as a valley (further in the middle: concave) and as a ridge (nearer in the middle)"""
    yy, xx = np.mgrid[:40, :80]
    valley = (1000 - 6 * np.abs(xx - 40)).astype(np.uint16)
    ridge = (900 + 6 * np.abs(xx - 40)).astype(np.uint16)
    kw = dict(radius=2, step=3, min_count=8, cos_max=0.999, span_max=0.1)
    v, r = _check(dev, valley, **kw), _check(dev, ridge, **kw)
    assert v["edge"][:, 38:43].all() and not v["edge"][:, :30].any() and not v["edge"][:, 50:].any()
    assert not r["edge"].any() and r["counts"][1] == v["counts"][1] == 3200


@pytest.fixture(scope="module")
def demo():
    from cppf_amd.utils.util import read_depth_png
    return read_depth_png(os.path.join(GOLDEN, "demo_0000_depth.png"))


def test_demo_frame(dev, demo):
    assert demo.shape == (480, 640)
    w = _check(dev, demo, None, K)
    assert w["counts"][2] == 215686 and 0 < w["counts"][0] < w["counts"][1] <= w["counts"][2]
    r = SG.concave_edges(demo, K)
    assert [r["n_edge"], r["n_fit"], r["n_live"]] == w["counts"][:3].tolist() and r["options"] == SG.concave_options()
    assert np.array_equal(r["edge"].cpu().numpy(), w["edge"])
    # the cut alone breaks up the frame's one blob of 206 920 pixels (figures, not pinned: DESIGN.md 3.7l)
    cut = R.segments_ref(demo, w["edge"] == 0, min_pixels=200, capacity=1024)
    assert cut["sizes"].max() < 206920 and cut["counts"][0] > 9
    valid = np.ones(demo.shape, np.uint8)
    valid[200:203, :] = 0
    r2 = SG.concave_edges(demo, K, valid.astype(bool), radius=4, step=5)
    w2 = C.concave_ref(demo, valid, K[0, 0], K[1, 1], K[0, 2], K[1, 2], **SG.concave_options(radius=4, step=5))
    assert np.array_equal(r2["edge"].cpu().numpy(), w2["edge"]) and r2["n_live"] == w2["counts"][2] < r["n_live"]


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
        t.fill_(3)
    g.replay()
    torch.cuda.synchronize()
    return eager, [t.cpu().numpy() for t in outs]


def test_same_bits_and_graph_replay(dev):
    d, _ = _image(78, 100, 257)                                                # (an image with a valley: some thousand edge pixels)
    v = (np.random.default_rng(78).random(d.shape) < 0.97).astype(np.uint8)
    cam = _cam(100, 257)
    runs = [_run(dev, d, v, cam, radius=2, step=2, min_count=8, cos_max=0.97, span_max=0.3) for _ in range(3)]
    assert runs[0]["counts"][0] > 0
    for r in runs[1:]:
        for k in KEYS:
            assert np.array_equal(r[k].view(np.uint8), runs[0][k].view(np.uint8)), k
    dd, vv = torch.from_numpy(d.view(np.int16)).to(dev), torch.from_numpy(v).to(dev)
    kw = dict(radius=2, step=2, min_count=8, cos_max=0.97, span_max=0.3)
    out = SG.concave_edges_device(dd, cam, vv, **kw)
    eager, replay = _graph(dev, lambda: SG.concave_edges_device(dd, cam, vv, out=out, **kw), [out[k] for k in KEYS])
    for k, e, r in zip(KEYS, eager, replay):
        assert np.array_equal(e.view(np.uint8), runs[0][k].view(np.uint8)) and np.array_equal(r.view(np.uint8), e.view(np.uint8)), k


def test_refusals_leave_poisoned_outputs_alone(dev):
    d = torch.full((4, 4), 1000, dtype=torch.int16, device=dev)
    edge = torch.full((4, 4), 0xAB, dtype=torch.uint8, device=dev)
    normal = torch.full((4, 4, 3), -7.5, dtype=torch.float64, device=dev)
    counts = torch.full((4,), -9, dtype=torch.int32, device=dev)
    good = dict(H=4, W=4, r=3, s=4, tol=10, slope=10, mc=16, cos=0.866, span=0.08)
    for kw in [dict(r=0), dict(r=9), dict(s=0), dict(s=17), dict(slope=1001), dict(tol=65536), dict(mc=2), dict(cos=1.0), dict(cos=-1.0),
               dict(span=0.0), dict(H=1, W=(1 << 24) + 1)]:
        a = dict(good, **kw)
        rc = call("cppf_concave_edges", dev, d, None, a["H"], a["W"], K[0, 0], K[1, 1], K[0, 2], K[1, 2], a["r"], a["s"], a["tol"], a["slope"],
                  a["mc"], a["cos"], a["span"], edge, normal, counts, ok=(-1,))
        assert rc == -1, kw
    out = dict(edge=edge, normal=normal, counts=counts)
    for kw in [dict(radius=0), dict(radius=9), dict(step=17), dict(min_count=2), dict(cos_max=1.0), dict(span_max=0.0), dict(tol_mm=65536)]:
        with pytest.raises(ValueError):
            SG.concave_edges_device(d, K, None, out=out, **kw)
    torch.cuda.synchronize()
    assert (edge == 0xAB).all() and (normal == -7.5).all() and (counts == -9).all()
    with pytest.raises(TypeError):
        SG.concave_edges(np.zeros((4, 4), np.float32), K)
    with pytest.raises(ValueError):
        SG.concave_edges(np.zeros((4, 4), np.uint16), K, np.ones((4, 5), bool))


def test_frame_segments_plumbing(dev, demo):
    """concave=None: today's dict key for key (support_mask, then depth_segments); concave={...}: edge == 0 ANDed into the mask that
    depth_segments is handed, after support_mask at n_planes > 0 and alone at n_planes = 0 -- bit for bit the hand composition"""
    keys = ["first", "labels", "n_components", "n_segments", "options", "planes", "sizes", "valid"]
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in ("labels", "sizes", "first")) and a["n_segments"] == b["n_segments"] \
        and a["n_components"] == b["n_components"]
    opts = dict(radius=4, step=5)
    c = SG.concave_edges(demo, K, **opts)
    keep = (c["edge"] == 0).to(torch.uint8)
    for n_planes in (0, 1):
        plain = SG.frame_segments(demo, K, n_planes=n_planes)
        assert sorted(plain) == keys
        valid, planes = (None, []) if n_planes == 0 else SG.support_mask(demo, K, n_planes)
        assert same(plain, SG.depth_segments(demo, valid)) and len(plain["planes"]) == len(planes) == n_planes
        assert (plain["valid"] is None) if n_planes == 0 else torch.equal(plain["valid"], valid)
        seg = SG.frame_segments(demo, K, n_planes=n_planes, concave=opts)
        assert sorted(seg) == sorted(keys + ["edge", "concave"]) and seg["concave"] == SG.concave_options(**opts) and seg["options"] == plain["options"]
        hand_valid = keep if valid is None else valid * keep
        assert torch.equal(seg["edge"], c["edge"]) and torch.equal(seg["valid"], hand_valid) and same(seg, SG.depth_segments(demo, hand_valid))
        lab = seg["labels"].cpu().numpy()
        assert (lab[c["edge"].cpu().numpy() != 0] == -1).all()                  # crease pixels stay unlabelled
        if n_planes == 0:                                                      # the cut alone breaks up the frame's one blob
            assert seg["n_segments"] > plain["n_segments"] and int(seg["sizes"].max()) < int(plain["sizes"].max())
        print(f"demo frame, {n_planes} planes: {plain['n_segments']} segments (largest {int(plain['sizes'].max())}) -> with the cut "
              f"{seg['n_segments']} (largest {int(seg['sizes'].max())}), {plain['n_components']} -> {seg['n_components']} components")
    assert SG.frame_segments(demo, K, n_planes=0, concave={})["concave"] == SG.concave_options()
    with pytest.raises(ValueError):
        SG.frame_segments(demo, K, n_planes=0, concave=dict(radius=9))
    with pytest.raises(TypeError):
        SG.frame_segments(demo, K, n_planes=0, concave=dict(radios=3))
