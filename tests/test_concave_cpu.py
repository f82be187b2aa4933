"""Concave edges without a device: tests/concave_ref.py (the restatement csrc/concave.hip is held to) against a loop-per-pixel brute
force with Python integers and fractions, the int64 / fp64 bound on the Cramer determinants, the refusals of cppf_concave_edges that
are decided on the host, the wrappers' refusals, the header's promise of no size query, and the analytic tabletop the cut was
designed on."""
import os
import re

import numpy as np
import pytest

import concave_ref as C
import segments_ref as R
from conftest import ROOT
from cppf_amd import _lib
from cppf_amd import segments as SG
from cppf_amd.frames import NOCS_INTRINSICS

EINVAL = -1
K = np.asarray(NOCS_INTRINSICS, np.float64)
CAM = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("seed", range(24))
def test_restatement_equals_the_brute_force(seed):
    rng = np.random.default_rng(1000 + seed)
    d, valid = C.planar_image(seed)
    r = int(rng.integers(1, 5)) if seed % 6 else 8
    kw = dict(radius=r, step=int(rng.integers(1, 6)) if seed % 5 else 16, tol_mm=int(rng.integers(0, 15)), slope_permille=int(rng.integers(0, 20)),
              min_count=int(rng.integers(3, max(4, (2 * r + 1) ** 2 // 2))), cos_max=float(rng.uniform(0.5, 0.99)), span_max=float(rng.uniform(0.01, 0.2)))
    # the principal point off the image centre on some seeds; 24 x 31 pixels of a 640 x 480 camera otherwise
    cam = CAM if seed % 3 else (CAM[0], CAM[1], 15.25, 11.5)
    a, b = C.concave_ref(d, valid, *cam, **kw), C.brute_ref(d, valid, *cam, **kw)
    assert np.array_equal(a["edge"], b["edge"]), kw
    assert np.array_equal(_bits(a["normal"]), _bits(b["normal"])), kw
    assert np.array_equal(a["counts"], b["counts"]), kw
    live = C.live_ref(d, valid)[1]
    fit = a["normal"].any(-1)
    assert a["counts"].tolist() == [int(a["edge"].sum()), int(fit.sum()), int(live.sum()), 0]
    assert not (a["edge"].astype(bool) & ~live).any() and not (fit & ~live).any()
    n2 = (a["normal"] ** 2).sum(-1)
    assert np.all(np.abs(n2[fit] - 1) < 1e-12)


def test_the_images_exercise_the_rule():
    """over the seeded images both outcomes of every test occur: pixels with and without a fit, edges and none"""
    tot = np.zeros(4, np.int64)
    for seed in range(24):
        d, valid = C.planar_image(seed)
        tot += C.concave_ref(d, valid, *CAM, radius=2, step=2, min_count=8, cos_max=0.95, span_max=0.2)["counts"]
    assert 0 < tot[0] < tot[1] < tot[2]


def test_determinants_stay_inside_int64_and_fp64():
    """The bound of include/cppf.h: at radius 8 every determinant is under 2^53 -- so int64 holds it (the issue's 5e18 with room) and
    its conversion to fp64 is exact -- for ANY accepted tol_mm and slope_permille, because |dz| <= 65535.  No accepted parameter breaks
    it; radius > 8 is refused.  An adversarial window (depths 1 and 65535 split along a diagonal, everything admitted) stays under it."""
    d_bound, n_bound = C.numerator_bound(8, 65535)
    assert d_bound < 2 ** 53 and n_bound < 2 ** 53 < 5 * 10 ** 18 < 2 ** 63
    assert C.numerator_bound(8)[1] == n_bound and C.numerator_bound(7)[1] < n_bound
    assert not C.check_args(4, 4, *CAM, 9, 1, 0, 0, 3, 0.5, 0.1)
    yy, xx = np.mgrid[:17, :17]
    worst = 0
    for pattern in (xx + yy > 16, xx > 8, (xx + 2 * yy) % 3 == 0):
        d = np.where(pattern, 65535, 1).astype(np.uint16)
        track = {}
        kw = dict(radius=8, step=1, tol_mm=65535, slope_permille=1000, min_count=3, cos_max=0.9, span_max=1e6)
        b = C.brute_ref(d, None, *CAM, track=track, **kw)
        a = C.concave_ref(d, None, *CAM, **kw)
        assert np.array_equal(a["edge"], b["edge"]) and np.array_equal(_bits(a["normal"]), _bits(b["normal"]))
        assert a["counts"][1] == 289                                          # every pixel admits the whole image
        worst = max(worst, track["max_abs_num"])
    assert 10 ** 12 < worst <= n_bound


def test_refusals_through_the_library_leave_poisoned_outputs_alone():
    L = _lib.lib()
    depth = np.full(16, 1000, np.uint16)
    edge, normal, counts = np.full(16, 0xAB, np.uint8), np.full(48, -7.5), np.full(4, -9, np.int32)
    good = dict(H=4, W=4, fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], r=3, s=4, tol=10, slope=10, mc=16, cos=0.866, span=0.08)

    def call(ptrs=None, **kw):
        a = dict(good, **kw)
        p = ptrs or (depth.ctypes.data, None, edge.ctypes.data, normal.ctypes.data, counts.ctypes.data)
        return L.cppf_concave_edges(p[0], p[1], a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], a["r"], a["s"], a["tol"], a["slope"], a["mc"],
                                    a["cos"], a["span"], p[2], p[3], p[4], None)

    bad = [dict(r=0), dict(r=9), dict(s=0), dict(s=17), dict(slope=1001), dict(slope=-1), dict(tol=65536), dict(tol=-1), dict(mc=2),
           dict(cos=1.0), dict(cos=-1.0), dict(cos=float("nan")), dict(span=0.0), dict(span=-1.0), dict(span=float("inf")), dict(span=float("nan")),
           dict(H=1, W=(1 << 24) + 1), dict(H=4097, W=4096), dict(H=0), dict(W=0), dict(H=-1), dict(fx=0.0), dict(fy=-1.0), dict(fx=float("nan")),
           dict(cx=float("inf"))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        a = dict(good, **kw)
        Km = np.array([[a["fx"], 0, a["cx"]], [0, a["fy"], a["cy"]], [0, 0, 1]])
        with pytest.raises(ValueError):
            SG.check_concave_args(a["H"], a["W"], Km, a["r"], a["s"], a["tol"], a["slope"], a["mc"], a["cos"], a["span"])
        assert not C.check_args(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], a["r"], a["s"], a["tol"], a["slope"], a["mc"], a["cos"], a["span"])
    base = (depth.ctypes.data, None, edge.ctypes.data, normal.ctypes.data, counts.ctypes.data)
    for i in (0, 2, 3, 4):                                                    # every pointer but `valid`
        assert call(ptrs=tuple(None if j == i else p for j, p in enumerate(base))) == EINVAL, i
    assert (edge == 0xAB).all() and (normal == -7.5).all() and (counts == -9).all()
    assert SG.check_concave_args(4096, 4096, K, 8, 16, 65535, 1000, 3, 0.999, 1e9) == CAM
    assert SG.check_concave_args(1, 1, K, 1, 1, 0, 0, 10 ** 6, -0.999, 1e-9) == CAM
    with pytest.raises(ValueError):
        SG.check_concave_args(4, 4, np.eye(4), 3, 4, 10, 10, 16, 0.5, 0.1)


def test_options_and_wrappers():
    o = SG.concave_options()
    assert o == dict(radius=3, step=4, tol_mm=10, slope_permille=10, min_count=16, cos_max=float(np.cos(np.deg2rad(30.0))), span_max=0.08)
    assert {k: o[k] for k in C.DEFAULTS} == C.DEFAULTS
    assert SG.concave_options(radius=4)["min_count"] == 27 and SG.concave_options(radius=4, min_count=5)["min_count"] == 5
    with pytest.raises(TypeError):
        SG.concave_options(radious=3)
    import torch
    if not torch.cuda.is_available():                                         # (with a device these are tested on it)
        with pytest.raises(_lib.CppfError):
            SG.concave_edges(np.zeros((4, 4), np.uint16), K)
        with pytest.raises(_lib.CppfError):
            SG.frame_segments(np.zeros((4, 4), np.uint16), K, n_planes=0, concave={})


def test_no_size_query_and_the_caps_agree():
    hdr = open(os.path.join(ROOT, "include", "cppf.h")).read()
    assert not re.findall(r"size_t\s+cppf_concave\w*\(", hdr)
    assert [s for s in _lib.exported_symbols() if "concave" in s] == ["cppf_concave_edges"]
    assert f"#define CPPF_CONCAVE_MAX_RADIUS {SG.CONCAVE_MAX_RADIUS}\n" in hdr and f"#define CPPF_CONCAVE_MAX_STEP {SG.CONCAVE_MAX_STEP}\n" in hdr
    assert (C.MAX_RADIUS, C.MAX_STEP) == (SG.CONCAVE_MAX_RADIUS, SG.CONCAVE_MAX_STEP) == (8, 16)
    assert _lib.ABI_VERSION == 4


@pytest.mark.parametrize("tilt", [30, 45, 60])
def test_the_analytic_tabletop(tilt):
    """A table through (0, 0.15, 1.0) m with up = (0, -cos t, -sin t) and four upright cylinders, two of them 2 mm apart, ray-cast and
    rounded to millimetres: without the cut the frame is ONE component; with it every cylinder's largest segment holds >= 0.80 of the
    cylinder's pixels and >= 0.99 of that segment belongs to the cylinder.  (Measured here: 0.89 .. 0.94 held, purity 1.000.)"""
    d, owner = C.tabletop_scene(tilt, K)
    assert d.shape == (480, 640) and all((owner == k).sum() > 2000 for k in range(4)) and (owner == 4).sum() > 200000
    gap = np.hypot(C.TABLE_CYLINDERS[2][0] - C.TABLE_CYLINDERS[1][0], C.TABLE_CYLINDERS[2][1] - C.TABLE_CYLINDERS[1][1])
    assert abs(gap - (C.TABLE_CYLINDERS[1][2] + C.TABLE_CYLINDERS[2][2])) < 0.0025      # the second and third touch
    r = C.concave_ref(d, None, *CAM, radius=3, step=4, cos_max=float(np.cos(np.deg2rad(30.0))), tol_mm=10, slope_permille=10, span_max=0.08,
                      min_count=(2 * 3 + 1) ** 2 // 3)
    plain = R.segments_ref(d, None, min_pixels=200)
    assert plain["counts"][0] == 1
    cut = R.segments_ref(d, r["edge"] == 0, min_pixels=200)
    for k in range(4):
        m = owner == k
        lab = cut["labels"][m]
        lab = lab[lab >= 0]
        assert lab.size
        seg = cut["labels"] == np.bincount(lab).argmax()
        held, purity = (seg & m).sum() / m.sum(), (seg & m).sum() / seg.sum()
        print(f"tilt {tilt} cylinder {k}: {m.sum()} pixels, held {held:.3f}, purity {purity:.3f}")
        assert held >= 0.80 and purity >= 0.99, (tilt, k, held, purity)
