"""Depth segments without a device: tests/segments_ref.py (the restatement csrc/segments.hip is held to) against a plain Python flood
fill, the refusals of cppf_depth_segments / cppf_plane_ransac that are decided on the host, the wrappers' refusals, support_mask's
band logic on a hand-made plane, and the header's promise that neither entry point brings a size query."""
import os
import re

import numpy as np
import pytest
import torch

import segments_ref as R
from conftest import ROOT
from cppf_amd import _lib
from cppf_amd import segments as SG

EINVAL = -1


@pytest.mark.parametrize("seed", range(20))
def test_restatement_equals_the_flood_fill(seed):
    rng = np.random.default_rng(seed)
    d = (rng.choice([500, 508, 520, 900], (12, 17)) + rng.integers(-3, 4, (12, 17))).astype(np.uint16)
    d[rng.random((12, 17)) < 0.2] = 0
    valid = (rng.random((12, 17)) < 0.9).astype(np.uint8) if seed % 2 else None
    kw = dict(tol_mm=int(rng.integers(0, 12)), slope_permille=int(rng.integers(0, 20)), min_pixels=int(rng.integers(1, 5)),
              max_pixels=int(rng.choice([0, 20])), capacity=int(rng.choice([3, 64])))
    a, b = R.segments_ref(d, valid, **kw), R.flood_ref(d, valid, **kw)
    for k in ("labels", "comp_size", "first", "sizes", "counts"):
        assert np.array_equal(a[k], b[k]), (k, kw)
    assert a["overflow"] == b["overflow"] == (a["counts"][0] > kw["capacity"])
    live = R.live_ref(d, valid)[1]
    assert a["counts"][2] == live.sum() and (a["comp_size"] > 0).sum() == live.sum()
    if not a["overflow"]:
        S = a["counts"][0]
        assert np.all(np.diff(a["first"][:S]) > 0) and np.array_equal(np.bincount(a["labels"][a["labels"] >= 0], minlength=S), a["sizes"][:S])
        assert np.array_equal(a["labels"].reshape(-1)[a["first"][:S]], np.arange(S))


def test_link_rule_words():
    """|dz| equal to the limit links, the limit + 1 does not; the slope term floors; depths beyond the int16 range compare unsigned"""
    seg = lambda row, **kw: R.segments_ref(np.array([row], np.uint16), min_pixels=1, **kw)["counts"][1]
    assert seg([1000, 1010], tol_mm=10, slope_permille=0) == 1 and seg([1000, 1011], tol_mm=10, slope_permille=0) == 2
    assert seg([1000, 1020], tol_mm=10, slope_permille=10) == 1 and seg([1000, 1021], tol_mm=10, slope_permille=10) == 2
    assert seg([999, 1018], tol_mm=10, slope_permille=10) == 1 and seg([999, 1019], tol_mm=10, slope_permille=10) == 2
    assert seg([40000, 40005], tol_mm=10, slope_permille=0) == 1
    assert seg([40000, 40005], tol_mm=4, slope_permille=0) == 2


def test_depth_segments_refusals_through_the_library():
    L = _lib.lib()
    buf = np.zeros(64, np.int32)                                              # (never followed: every call below is refused)
    p = buf.ctypes.data
    good = dict(H=4, W=4, tol=10, slope=10, mn=1, mx=0, cap=4)

    def call(ptrs=(p,) * 7, **kw):
        a = dict(good, **kw)
        depth, valid, labels, comp, first, sizes, counts = ptrs
        return L.cppf_depth_segments(depth, valid, a["H"], a["W"], a["tol"], a["slope"], a["mn"], a["mx"], a["cap"], labels, comp, first, sizes,
                                     counts, None)

    for kw in [dict(H=0), dict(W=0), dict(H=-1), dict(H=4097, W=4096), dict(H=1 << 16, W=1 << 16), dict(tol=-1), dict(tol=65536), dict(slope=-1),
               dict(slope=1001), dict(mn=0), dict(mx=-1), dict(cap=0), dict(cap=1025)]:
        assert call(**kw) == EINVAL, kw
        a = dict(good, **kw)
        with pytest.raises(ValueError):
            SG.check_segment_args(a["H"], a["W"], a["tol"], a["slope"], a["mn"], a["mx"], a["cap"])
    for i in (0, 2, 3, 4, 5, 6):                                              # every pointer but `valid`
        assert call(ptrs=tuple(None if j == i else p for j in range(7))) == EINVAL, i
    SG.check_segment_args(4096, 4096, 0, 0, 1, 0, 1024)
    SG.check_segment_args(1, 1, 65535, 1000, 1, 5, 1)


def test_plane_ransac_refusals_through_the_library():
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data & ~15
    call = lambda N=10, n_hyp=4, thresh=0.01, ptrs=(p,) * 4: L.cppf_plane_ransac(ptrs[0], N, n_hyp, thresh, 0, ptrs[1], ptrs[2], ptrs[3], None)
    for kw in [dict(N=0), dict(N=-1), dict(N=2 ** 31), dict(n_hyp=0), dict(n_hyp=1025), dict(thresh=-1e-6), dict(thresh=float("nan")),
               dict(thresh=float("inf"))]:
        assert call(**kw) == EINVAL, kw
        with pytest.raises(ValueError):
            SG.check_plane_args(kw.get("N", 10), kw.get("n_hyp", 4), kw.get("thresh", 0.01))
    for i in range(4):
        assert call(ptrs=tuple(None if j == i else p for j in range(4))) == EINVAL, i
    SG.check_plane_args(2 ** 31 - 1, 1024, 0.0)


def test_wrappers_refuse_what_they_cannot_take():
    with pytest.raises(TypeError):
        SG.segment_labels(dict(labels=np.zeros((3, 3), np.float32)))
    with pytest.raises(TypeError):
        SG.segment_labels(dict(labels=torch.zeros(9, dtype=torch.int32)))
    assert SG.segment_labels(dict(labels=np.zeros((3, 4), np.int64))).dtype == torch.int32
    if not torch.cuda.is_available():                                         # (with a device these are tested on it)
        with pytest.raises(_lib.CppfError):
            SG.depth_segments(np.zeros((4, 4), np.uint16))
        with pytest.raises(_lib.CppfError):
            SG.plane_ransac(np.zeros((4, 3), np.float32))
    else:
        with pytest.raises(TypeError):
            SG.depth_tensor(np.zeros((4, 4), np.float32))
        with pytest.raises(ValueError):
            SG.depth_tensor(torch.zeros((4, 4), dtype=torch.int16))            # a host tensor is not uploaded
        with pytest.raises(ValueError):
            SG.depth_tensor(np.zeros(4, np.uint16))


def test_band_logic_on_a_hand_made_plane():
    """off_planes on the CPU: the plane z = 1 written {0, 0, -1, 1} (d >= 0); points at 1 +- 0.0149 are on it, at 1 +- 0.0151 off it,
    a second plane removes more, a point that is not finite is off nothing"""
    pl = np.array([0, 0, -1, 1], np.float32)
    z = np.array([1.0, 1.0149, 0.9851, 1.0151, 0.9849, 2.0, np.nan], np.float32)
    pts = torch.from_numpy(np.stack([np.linspace(-1, 1, z.size, dtype=np.float32), np.zeros(z.size, np.float32), z], -1))
    assert SG.off_planes(pts, [pl], 0.015).tolist() == [False, False, False, True, True, True, False]
    assert SG.off_planes(pts, [], 0.015).all()
    pl2 = np.array([0, 0, -1, 2], np.float32)
    assert SG.off_planes(pts, [pl, pl2], 0.015).tolist() == [False, False, False, True, True, False, False]


def test_planes_restatement_on_a_known_triple():
    """three points of the plane z = 2 whatever the draw: every hypothesis is that plane or degenerate (a repeated point), with the
    normal turned so that d >= 0; collinear points are degenerate"""
    pts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], np.float32)
    pl = R.planes_ref(pts, 64, seed=3)
    ok = pl[:, :3].any(-1)
    assert ok.any() and (~ok).any()
    assert np.array_equal(pl[ok], np.tile(np.array([0, 0, -1, 2], np.float32), (ok.sum(), 1)))
    c = R.counts_ref(pts, pl, 0.0)
    assert np.array_equal(c, np.where(ok, 3, 0))
    b = R.best_ref(pl, c)
    assert b[0] == np.nonzero(ok)[0][0] and b[1] == 3
    line = np.stack([np.arange(5), np.arange(5), np.arange(5)], -1).astype(np.float32)
    assert not R.planes_ref(line, 32, seed=0).any()
    assert R.best_ref(np.zeros((4, 4), np.float32), np.zeros(4, np.int32)).tolist() == [-1, 0]
    ia, ib, ic = R.plane_indices_ref(1, 8, 0)
    assert not (ia.any() or ib.any() or ic.any())


def test_no_new_size_query_and_the_caps_agree():
    hdr = open(os.path.join(ROOT, "include", "cppf.h")).read()
    assert not re.findall(r"size_t\s+cppf_(?:depth_segments|plane_ransac|segments)\w*\(", hdr)
    assert not [s for s in _lib.exported_symbols() if ("segments_" in s or "plane_" in s) and "bytes" in s and "segment_instance" not in s]
    assert f"#define CPPF_SEGMENTS_MAX {SG.SEGMENTS_MAX}\n" in hdr and f"#define CPPF_PLANE_MAX_HYPOTHESES {SG.PLANE_MAX_HYPOTHESES}\n" in hdr
    assert "cppf_depth_segments" in _lib.exported_symbols() and "cppf_plane_ransac" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 4


def test_the_cap_holds_on_the_oracle_vote(oracle):
    """without a device: the oracle's vote of the perfect-head scene whose pairs all lie inside the true objects, smoothed, yields
    every object within one cell under max_proposals = 2 n_obj -- so tests/test_gpu_segment_scene.py asks the device for nothing the
    definition does not give"""
    import scene_poses_ref as S
    import zero_shot_ref as Z
    from cppf_amd.inference import grid_shape
    sc, idx, outputs, _ = R.perfect_segment_scene()
    cfg, n_obj = sc["cfg"], R.PERFECT[1]
    corners, dims = grid_shape(sc["pc"], cfg.res)
    grid = np.zeros(tuple(int(d) for d in dims), np.float32)
    oracle.ppf_voting(sc["pc"], outputs, np.ones(idx.shape[0], np.float32), idx.astype(np.int32), grid, corners[0], cfg.res, 72, True)
    loc, _, _, _ = Z.proposals(Z.smooth(grid), max_proposals=2 * n_obj)
    m = S.match_objects(loc, corners[0], cfg.res, [o["center"] for o in sc["obs"]])
    assert None not in m and len(set(m)) == n_obj, m
