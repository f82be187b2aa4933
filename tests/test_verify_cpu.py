"""Proposal verification without a device: tests/verify_ref.py (the restatement csrc/verify.hip is held to) on hand-built cases with
known counts, the host halves of scene_stage.verify_proposals (the boxes, the ratios) against it, the refusals of the two entry points
that return before anything is touched, and detections.pool_detections with score="agreement" and the three filters on hand-written
pose dicts."""
import os
import sys

import numpy as np
import pytest

from cppf_amd import _lib, detections, scene_stage
from cppf_amd.config import CATEGORIES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_ref as V  # noqa: E402

EINVAL = -1


def test_proposal_support_hand_counts():
    """mask 0 = {0, 1, 2}, mask 1 empty, N = 6: a pair (i, i), endpoints at -1 and at N, a bit >= K"""
    masks = np.zeros((2, 6), np.uint8)
    masks[0, [0, 1, 2]] = (1, 7, 255)                       # any non-zero byte is a member
    pairs = [((0, 1), 0b01),     # within, agree
             ((1, 1), 0b00),     # (i, i) in the mask: within, once
             ((0, 4), 0b01),     # cross, agree
             ((-1, 2), 0b01),    # -1 is a non-member, the pair counts through 2: cross, agree
             ((6, 2), 0b00),     # N likewise: cross
             ((4, 5), 0b11),     # no endpoint in any mask: nothing, whatever its bits
             ((-1, 6), 0b01),    # both outside
             ((0, 2), 0b100),    # a bit >= K set, bit 0 clear: within, not agree
             ((4, 4), 0b01)]     # (i, i) outside the mask
    idx = np.array([p for p, _ in pairs], np.int32)
    bits = np.array([b for _, b in pairs], np.uint32)
    got = V.proposal_support(idx, bits, masks)
    assert got.tolist() == [[3, 1, 3, 2], [0, 0, 0, 0]]      # the empty mask counts nothing
    assert V.proposal_support(idx[:0], bits[:0], masks).tolist() == [[0] * 4] * 2
    # the counts do not depend on the order of the pairs or of a pair's endpoints
    assert np.array_equal(V.proposal_support(idx[::-1, ::-1], bits[::-1], masks), got)


def test_proposal_support_bit_31():
    """K = 32 with only bit 31 in use"""
    masks = np.zeros((32, 4), np.uint8)
    masks[31, [0, 1]] = 1
    idx = np.array([(0, 1), (0, 1), (1, 3), (2, 3)], np.int32)
    bits = np.array([0x80000000, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)
    got = V.proposal_support(idx, bits, masks)
    assert got[31].tolist() == [2, 1, 1, 1] and not got[:31].any()
    assert V.proposal_support(idx, bits.view(np.int32), masks)[31].tolist() == [2, 1, 1, 1]      # the words as int32, as torch holds them


def _rotated_box():
    a = np.deg2rad(30.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    b = np.deg2rad(20.0)
    Rx = np.array([[1.0, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = Rz @ Rx
    c = np.array([0.3, -0.2, 0.9])
    h = np.array([0.1, 0.2, 0.3])
    local, inside = [], []
    for ax in range(3):
        for sign in (-1.0, 1.0):
            for eps, is_in in ((-1e-3, True), (1e-3, False)):               # just inside and just outside each of the six faces
                p = np.zeros(3)
                p[ax] = sign * (h[ax] + eps)
                local.append(p)
                inside.append(is_in)
    pts = c + np.array(local) @ R.T                                           # p = c + R local: the columns of R are the box axes
    return pts, np.array(inside), c, R, h


def test_box_support_rotated_box():
    pts, inside, c, R, h = _rotated_box()
    assert np.allclose(V.box_coords(pts, c, R.reshape(9))[0], [-(0.1 - 1e-3), 0, 0])
    masks = np.stack([np.ones(12, np.uint8), (~inside).astype(np.uint8), np.zeros(12, np.uint8)])
    K = masks.shape[0]
    got = V.box_support(pts, masks, np.tile(c, (K, 1)), np.tile(R.reshape(9), (K, 1)), np.tile(h, (K, 1)))
    assert got.tolist() == [[12, 6, 6], [6, 0, 6], [0, 0, 6]]
    # the transposed matrix is another box: the axes are R's COLUMNS
    assert V.box_support(pts, masks[:1], c[None], R.T.reshape(1, 9), h[None]).tolist() != [[12, 6, 6]]
    # a non-finite point is in no box (an infinite box included); a NaN box and a negative half extent hold nothing
    bad = pts.copy()
    bad[0, 1] = np.nan
    bad[2, 0] = np.inf
    assert inside[0] and inside[2]
    assert V.box_support(bad, masks[:1], c[None], R.reshape(1, 9), h[None]).tolist() == [[12, 4, 4]]
    assert V.box_support(bad, masks[:1], c[None], R.reshape(1, 9), np.full((1, 3), np.inf)).tolist() == [[12, 10, 10]]
    assert V.box_support(pts, masks[:1], np.full((1, 3), np.nan), R.reshape(1, 9), h[None]).tolist() == [[12, 0, 0]]
    assert V.box_support(pts, masks[:1], c[None], R.reshape(1, 9), -np.ones((1, 3))).tolist() == [[12, 0, 0]]
    assert abs(V.face_margin(pts, c[None], R.reshape(1, 9), h[None]) - 1e-3 / 0.3) < 1e-9


def test_ratios_and_the_zero_denominator_rule():
    r = V.ratios([8, 6, 10, 1, 20, 15, 60])
    assert (r["agreement"], r["leak"], r["fill"], r["purity"]) == (0.75, 0.1, 0.75, 0.25)
    assert [r[k] for k in V.COUNTS] == [8, 6, 10, 1, 20, 15, 60] and all(isinstance(r[k], int) for k in V.COUNTS)
    z = V.ratios([0] * 7)
    assert (z["agreement"], z["leak"], z["fill"], z["purity"]) == (0.0, 0.0, 0.0, 0.0)
    part = V.ratios([0, 0, 5, 5, 3, 0, 0])
    assert (part["agreement"], part["leak"], part["fill"], part["purity"]) == (0.0, 1.0, 0.0, 0.0)
    for counts in ([8, 6, 10, 1, 20, 15, 60], [0] * 7, [0, 0, 5, 5, 3, 0, 0]):
        got = scene_stage.verify_ratios(np.array(counts, np.int32))
        assert got == V.ratios(counts) and all(type(got[k]) is int for k in V.COUNTS) and type(got["agreement"]) is float
    assert scene_stage.VERIFY_COUNTS == V.COUNTS


def test_verify_boxes():
    cfg = CATEGORIES["mug"]
    pts, _, c, R, h = _rotated_box()
    poses = [dict(T=c, R=R, scale=2 * h), dict(T=c, R=R, scale_3d=2 * h, scale=7.0),          # the zero-shot form: scale is a norm
             dict(T=c, R=R * np.nan, scale=2 * h), dict(T=c, R=R, scale=np.array([np.inf, 1, 1]))]
    for pad in (None, 0.0, 0.02):
        got = scene_stage.verify_boxes(poses, cfg, pad)
        assert got.dtype == np.float32 and got.shape == (4, 15) and np.array_equal(got, V.boxes_of(poses, cfg.res, pad))
        want = np.concatenate([c, R.reshape(9), h + (cfg.res if pad is None else pad)]).astype(np.float32)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        assert (got[2:, 12:] == -1).all() and (got[2:, :12] == 0).all()
    assert scene_stage.proposal_group(4099) == 32 and scene_stage.proposal_group(1 << 26) == 31 and scene_stage.proposal_group(0) == 32


def test_entry_points_refuse_before_touching_anything():
    """cppf_proposal_support / cppf_box_support with fake non-null pointers: every case here returns before a launch"""
    L = _lib.lib()
    P, N, K = 100, 50, 5
    need = L.cppf_proposal_support_workspace_bytes(N)
    assert need >= 4 * N and need % 256 == 0 and L.cppf_proposal_support_workspace_bytes(-1) == 0
    good = dict(idx=0x1000, bits=0x2000, masks=0x3000, P=P, N=N, K=K, counts=0x4000, ws=0x5000, wsb=need)

    def sup(**kw):
        a = dict(good, **kw)
        return L.cppf_proposal_support(a["idx"], a["bits"], a["masks"], a["P"], a["N"], a["K"], a["counts"], a["ws"], a["wsb"], None)
    for kw in (dict(K=0), dict(K=33), dict(K=-1), dict(N=0), dict(N=1 << 31), dict(P=-1), dict(P=1 << 27), dict(idx=None), dict(bits=None),
               dict(masks=None), dict(counts=None), dict(ws=None), dict(wsb=need - 1), dict(wsb=0)):
        assert sup(**kw) == EINVAL, kw
    bgood = dict(pts=0x1000, masks=0x2000, c=0x3000, A=0x4000, h=0x5000, N=N, K=K, counts=0x6000)

    def box(**kw):
        a = dict(bgood, **kw)
        return L.cppf_box_support(a["pts"], a["masks"], a["c"], a["A"], a["h"], a["N"], a["K"], a["counts"], None)
    for kw in (dict(K=0), dict(K=33), dict(N=0), dict(N=1 << 31), dict(N=-1), dict(pts=None), dict(masks=None), dict(c=None), dict(A=None),
               dict(h=None), dict(counts=None)):
        assert box(**kw) == EINVAL, kw
    assert L.cppf_abi_version() == 4                                         # additive: the version stays


def _pose(x, agreement, fill, within, diff, verify=True):
    """an axis-aligned 10 cm box at (x, 0, 1): far enough from its neighbours that the NMS suppresses nothing"""
    p = dict(T=np.array([x, 0.0, 1.0]), R=np.eye(3), scale=np.full(3, 0.1), scale_norm=float(np.linalg.norm(np.full(3, 0.1))), diff=diff,
             cnt=diff + 1.0)
    if verify:
        p["verify"] = dict(agreement=agreement, fill=fill, within=within, agree=int(agreement * within), leak=0.0, purity=0.0)
    return p


def test_pool_detections_agreement_score_and_filters():
    #                 x    agreement fill within diff
    a = dict(poses=[_pose(0.0, 0.90, 0.8, 400, 10.0), _pose(1.0, 0.20, 0.9, 900, 50.0), _pose(2.0, 0.60, 0.1, 50, 30.0)])
    b = dict(poses=[_pose(3.0, 0.70, 0.5, 10, 99.0), None, _pose(4.0, 0.95, 0.7, 300, 1.0)])
    names = ["mug", "cup"]
    by_diff = detections.pool_detections([a, b], names)
    assert [(d["category"], d["proposal"]) for d in by_diff["detections"]] == [(1, 0), (0, 1), (0, 2), (0, 0), (1, 2)]
    assert "filtered" not in by_diff                                         # the defaults: today's keys
    assert set(by_diff) == {"detections", "kept_per_category", "suppressed", "proposals_per_category", "result", "cfgs"}

    res = detections.pool_detections([a, b], names, score="agreement")
    assert [(d["category"], d["proposal"]) for d in res["detections"]] == [(1, 2), (0, 0), (1, 0), (0, 2), (0, 1)]
    assert [d["score"] for d in res["detections"]] == [0.95, 0.90, 0.70, 0.60, 0.20]
    assert np.array_equal(res["result"]["pred_scores"], [0.95, 0.90, 0.70, 0.60, 0.20])
    assert res["filtered"] == {"mug": 0, "cup": 0} and res["proposals_per_category"] == {"mug": 3, "cup": 2}

    f = detections.pool_detections([a, b], names, score="agreement", min_agreement=0.6)          # the bound itself passes
    assert [(d["category"], d["proposal"]) for d in f["detections"]] == [(1, 2), (0, 0), (1, 0), (0, 2)]
    assert f["filtered"] == {"mug": 1, "cup": 0} and f["kept_per_category"] == {"mug": 2, "cup": 2}
    assert f["proposals_per_category"] == {"mug": 3, "cup": 2} and f["suppressed"] == {"mug": 0, "cup": 0}
    f = detections.pool_detections([a, b], names, min_fill=0.6)                                  # a filter with the old score
    assert [(d["category"], d["proposal"]) for d in f["detections"]] == [(0, 1), (0, 0), (1, 2)] and f["filtered"] == {"mug": 1, "cup": 1}
    assert [d["score"] for d in f["detections"]] == [50.0, 10.0, 1.0]
    f = detections.pool_detections([a, b], names, score="agreement", min_within=100)
    assert [(d["category"], d["proposal"]) for d in f["detections"]] == [(1, 2), (0, 0), (0, 1)] and f["filtered"] == {"mug": 1, "cup": 1}
    f = detections.pool_detections([a, b], names, score="agreement", min_agreement=0.5, min_fill=0.6, min_within=350)
    assert [(d["category"], d["proposal"]) for d in f["detections"]] == [(0, 0)] and f["filtered"] == {"mug": 2, "cup": 2}
    f = detections.pool_detections([a, b], names, score="agreement", min_agreement=2.0)
    assert f["detections"] == [] and f["filtered"] == {"mug": 3, "cup": 2} and f["result"]["pred_RTs"].shape == (0, 4, 4)

    # filters come before the NMS: a coincident, higher-scored detection that the filter drops suppresses nothing
    twin = dict(poses=[_pose(0.0, 0.90, 0.8, 400, 10.0), _pose(0.001, 0.99, 0.8, 5, 20.0)])
    assert [d["proposal"] for d in detections.pool_detections([twin], ["mug"], score="agreement")["detections"]] == [1]
    assert [d["proposal"] for d in detections.pool_detections([twin], ["mug"], score="agreement", min_within=100)["detections"]] == [0]


def test_pool_detections_needs_verify():
    plain = dict(poses=[_pose(0.0, 0, 0, 0, 10.0, verify=False)])
    for kw in (dict(score="agreement"), dict(min_agreement=0.5), dict(min_fill=0.5), dict(min_within=1)):
        with pytest.raises(ValueError, match="verify=True"):
            detections.pool_detections([plain], ["mug"], **kw)
    assert len(detections.pool_detections([plain], ["mug"])["detections"]) == 1
    with pytest.raises(ValueError, match="agreement"):
        detections.pool_detections([plain], ["mug"], score="purity")
