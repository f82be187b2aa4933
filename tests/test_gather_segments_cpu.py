"""Segment labels -> segment clouds without a device: tests/gather_segments_ref.py (the restatement cppf_gather_segments is held to)
against plain Python loops -- the stable order, labels in no segment, empty segments, the bounds' order of -0.0 and +0.0 and the points
with a NaN or an infinite coordinate that the bounds leave out --, the refusals of cppf_gather_segments that are decided on the
host, and detections.select_per_segment, the choice among a segment's candidates."""
import os

import numpy as np
import pytest

import gather_segments_ref as R
from conftest import ROOT
from cppf_amd import _lib, detections, segments

EINVAL = -1


def test_the_key_orders_the_zeros_and_follows_the_float_order():
    x = np.array([-np.inf, -3.5, -1e-38, -1e-45, -0.0, 0.0, 1e-45, 1e-38, 3.5, np.inf], np.float32)
    k = R.key(x)
    assert (np.diff(k) > 0).all() and k[4] == -1 and k[5] == 0                # strictly increasing: -0.0 lies below +0.0
    rng = np.random.default_rng(0)
    y = rng.standard_normal(500).astype(np.float32)
    assert np.array_equal(np.argsort(R.key(y), kind="stable"), np.argsort(y, kind="stable"))


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("S", [1, 3, 7])
def test_restatement_equals_the_loop(S, pattern):
    M = 131
    hi, nrm = R.cloud(M, seed=S)
    lab = R.labels_case(pattern, M, S, seed=S)
    offsets, pts, nr, src, bounds = R.gather_segments_loop(hi, nrm, lab, S)
    T = int(offsets[-1])
    g = R.gather_segments_ref(hi, nrm, lab, S, capacity=T + 3)
    assert np.array_equal(g["offsets"], offsets) and np.array_equal(g["src"][:T], src) and (g["src"][T:] == R.POISON_I).all()
    assert np.array_equal(R.bits(g["pts"][:T]), R.bits(pts)) and np.array_equal(R.bits(g["nrm"][:T]), R.bits(nr))
    assert np.array_equal(R.bits(g["bounds"]), R.bits(bounds))
    assert T == R.in_range(lab, S).sum()
    for s in range(S):                                                        # hi[labels == s], in increasing dense index
        rows = np.nonzero(lab == s)[0]
        assert np.array_equal(src[offsets[s]:offsets[s + 1]], rows)
        assert np.array_equal(R.bits(pts[offsets[s]:offsets[s + 1]]), R.bits(hi[rows]))
    # the intermediate: the points of segment s in the chunks before c (one chunk here: all zero), and its last row + the last chunk's
    # points = the totals
    assert g["chunk_counts"].shape == (1, S) and not g["chunk_counts"].any()
    if T >= 1:
        s_ = R.gather_segments_ref(hi, nrm, lab, S, capacity=T - 1)           # one row short: complete offsets, the last row dropped
        assert np.array_equal(s_["offsets"], offsets) and np.array_equal(s_["src"], src[:T - 1])
        assert np.array_equal(R.bits(s_["pts"]), R.bits(pts[:T - 1]))


def test_patterns_are_what_their_names_say():
    for S in (1, 7, 33, 1024):
        M = 3 * 1024 + 7
        lanes = R.labels_case("lanes", M, S)
        for w in (0, 1, 17, M // 64 - 1):
            assert np.unique(lanes[64 * w:64 * w + 64]).size == min(S, 64)
        assert np.unique(R.labels_case("one", M, S)).tolist() == [S // 2]
        runs = R.labels_case("runs", M, S)
        ends = np.nonzero(np.diff(runs))[0] + 1
        if S > 1:
            assert {37, 64, 129, 130, 960, 1023, 1087}.issubset(set(ends.tolist()))          # run edges beside the wave and the chunk edge
            assert (np.diff(runs[ends]) < 0).any()                                          # labels do not arrive in order
        mixed = R.labels_case("mixed", M, S)
        assert {-1, S, R.INT32_MAX, R.INT32_MIN}.issubset(set(mixed.tolist())) and R.in_range(mixed, S).sum() > M // 2
        empty = R.labels_case("empty", M, S)
        counts = np.bincount(empty[R.in_range(empty, S)], minlength=S)
        assert counts[0] == counts[S // 2] == counts[S - 1] == 0 and (S <= 3 or S > 64 or (counts > 0).sum() == S - 3)


def test_bounds_order_the_zeros_and_leave_out_points_that_are_not_finite():
    z, nz, nan, inf = np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(np.inf)
    hi = np.array([[z, nz, 1.0],          # segment 0: x {+0, -0}: min -0, max +0;   y {-0, +0};   z {1, 2}
                   [nz, z, 2.0],
                   [nan, 5.0, 5.0],       # segment 0, NaN: left out whole (its finite y = 5 too)
                   [-9.0, inf, 0.0],      # segment 0, inf: left out whole
                   [1.0, 1.0, -inf],      # segment 1: only this point: empty bounds
                   [nz, nz, nz],          # segment 2: a single -0.0 point: min = max = -0.0
                   [3.0, -4.0, 5.0]],     # label 7: in no segment
                  np.float32)
    lab = np.array([0, 0, 0, 0, 1, 2, 7], np.int32)
    nrm = np.zeros_like(hi)
    g = R.gather_segments_ref(hi, nrm, lab, 4)
    want = np.array([[nz, nz, 1.0, z, z, 2.0], R.EMPTY_BOUNDS, [nz] * 6, R.EMPTY_BOUNDS], np.float32)
    assert np.array_equal(R.bits(g["bounds"]), R.bits(want))
    assert np.array_equal(R.bits(g["bounds"]), R.bits(R.gather_segments_loop(hi, nrm, lab, 4)[4]))
    assert g["offsets"].tolist() == [0, 4, 5, 6, 6] and g["src"][:6].tolist() == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(R.bits(g["pts"][:6]), R.bits(hi[:6]))               # the rows still hold every point, NaN bits included


def test_chunk_counts_of_the_restatement():
    M, S = 3 * 1024 + 7, 7
    hi, nrm = R.cloud(M, seed=1)
    lab = R.labels_case("mixed", M, S, seed=1)
    g = R.gather_segments_ref(hi, nrm, lab, S)
    cc = g["chunk_counts"]
    assert cc.shape == (4, S) and not cc[0].any()
    for c in range(4):
        for s in range(S):
            assert cc[c, s] == (lab[:c * 1024] == s).sum()


def test_refusals_that_need_no_device():
    """the host's checks of cppf_gather_segments return before anything is launched; segments.check_segment_cloud_args mirrors them"""
    L = _lib.lib()
    buf = np.full(64, R.POISON_I, np.int32)                                   # (never followed: every call below is refused)
    p = buf.ctypes.data
    call = lambda S, M, cap: L.cppf_gather_segments(p, p, p, S, M, cap, p, p, p, p, p, p, None)
    for S, M, cap in [(0, 4, 4), (1025, 4, 4), (-1, 4, 4), (2, -1, 4), (2, 4, -1), (2, 2 ** 31, 4)]:
        assert call(S, M, cap) == EINVAL, (S, M, cap)
        with pytest.raises(ValueError):
            segments.check_segment_cloud_args(S, M, cap)
    cap_m = segments.GATHER_CHUNK * segments.GATHER_MAX_CHUNKS
    assert call(1, cap_m + 1, 4) == _lib.EUNSUPPORTED and call(1024, 2 ** 31 - 1, 0) == _lib.EUNSUPPORTED
    with pytest.raises(ValueError, match="at most"):
        segments.check_segment_cloud_args(1, cap_m + 1, 4)
    segments.check_segment_cloud_args(1024, cap_m, 0)
    f = L.cppf_gather_segments
    assert f(p, p, p, 2, 4, 4, None, p, p, p, p, p, None) == EINVAL           # offsets NULL
    for j in (7, 8, 9):                                                       # pts / nrm / src NULL, capacity > 0
        a = [p, p, p, 2, 4, 4, p, p, p, p, p, p, None]
        a[j] = None
        assert f(*a) == EINVAL, j
    for j in (0, 1, 2, 11):                                                   # hi / hi_nrm / labels / chunk_counts NULL, points
        a = [p, p, p, 2, 4, 4, p, p, p, p, p, p, None]
        a[j] = None
        assert f(*a) == EINVAL, j
    assert (buf == R.POISON_I).all()
    hdr = open(os.path.join(ROOT, "include", "cppf.h")).read()
    assert f"#define CPPF_GATHER_SEGMENTS_MAX {segments.SEGMENTS_MAX} " in hdr and f"#define CPPF_SEGMENTS_MAX {segments.SEGMENTS_MAX}\n" in hdr


def test_a_cloud_without_labels_is_refused_without_a_device():
    import torch
    from cppf_amd.scene_stage import SceneCloud
    z = torch.zeros((4, 3))
    bare = SceneCloud(hi=z, hi_nrm=z, hi_labels=None, ind=torch.arange(4), pc=z, nrm=z, labels=None)
    for fn in (segments.segment_clouds, segments.segment_clouds_device):
        with pytest.raises(ValueError, match="labels"):
            fn(bare, 3)
    with pytest.raises(ValueError, match="labels"):
        segments.segment_clouds((z, z), 3)


# ------------------------------------------------------------------------------------------------ select_per_segment
def _c(segment, category, score, **kw):
    return dict(segment=segment, category=category, score=score, **kw)


def test_select_best_takes_the_highest_score_per_segment():
    cands = [_c(2, 0, 0.25), _c(2, 1, 0.75), _c(2, 2, 0.5), _c(0, 0, 0.125), _c(0, 1, 0.0625), _c(5, 2, 0.0)]
    got = detections.select_per_segment(cands, "best")
    assert [(g["segment"], g["category"]) for g in got] == [(0, 0), (2, 1), (5, 2)]                     # ascending segment
    assert got[1] is cands[1] and got[0] is cands[3]                          # the dicts themselves
    assert detections.select_per_segment(cands) == got                        # the default rule


def test_select_best_gives_an_equal_score_to_the_lower_category():
    a = [_c(1, 2, 0.5), _c(1, 0, 0.5), _c(1, 1, 0.5), _c(3, 1, 0.25), _c(3, 0, 0.125)]
    for order in (a, a[::-1], [a[1], a[0], a[2], a[4], a[3]]):               # whatever the order they arrive in
        got = detections.select_per_segment(order, "best")
        assert [(g["segment"], g["category"]) for g in got] == [(1, 0), (3, 1)]
    # a higher score beats a lower category; NaN never wins, not even alone
    got = detections.select_per_segment([_c(1, 0, 0.5), _c(1, 3, 0.5000001), _c(4, 0, float("nan")), _c(6, 1, float("nan")), _c(6, 2, -1.0)])
    assert [(g["segment"], g["category"]) for g in got] == [(1, 3), (6, 2)]


def test_select_leaves_out_a_segment_with_no_candidate_and_all_keeps_everything():
    cands = [_c(0, 0, 0.5), _c(3, 1, 0.25), _c(3, 0, 0.125)]                  # segments 1 and 2 have no candidate
    assert [g["segment"] for g in detections.select_per_segment(cands, "best")] == [0, 3]
    assert detections.select_per_segment([], "best") == [] and detections.select_per_segment([], "all") == []
    everything = detections.select_per_segment(cands, "all")
    assert everything == cands and everything is not cands and all(a is b for a, b in zip(everything, cands))
    with pytest.raises(ValueError, match="'best' or 'all'"):
        detections.select_per_segment(cands, "first")
