"""3D box NMS without a device: evaluation.nms_3d's host path (the checker of csrc/box_nms.hip) on what the reference's own `nms` /
`iou_3d` (sunrgbd/eval.py:13-35) returned for seeded boxes (tests/golden/make_golden_nms.py -> nms_cases.npz), the tie and strictness
rules, the degenerate-box filter, nms_results, and every refusal of the C entry point that needs no launch."""
import ctypes as C

import numpy as np
import pytest

from cppf_amd import evaluation as E


@pytest.fixture(scope="module")
def z(golden):
    return golden("nms_cases.npz")


def _case(z, k):
    return z[f"RT_{k}"], z[f"scales_{k}"], z[f"scores_{k}"], float(z[f"thresh_{k}"]), z[f"pick_{k}"], z[f"iou_{k}"]


def _boxes(centres, extent=1.0):
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    RT = np.tile(np.eye(4), (len(centres), 1, 1))
    RT[:, :3, 3] = centres
    return RT, np.full((len(centres), 3), float(extent))


def test_golden_cases_hold_what_the_generator_asserts(z):
    sizes = [len(z[f"scores_{k}"]) for k in range(int(z["n_cases"]))]
    assert sizes == [1, 2, 33, 64, 65, 130]
    for k, m in enumerate(sizes):
        _, _, scores, thresh, pick, iou = _case(z, k)
        assert len(np.unique(scores)) == m and len(iou) == m * (m - 1) // 2
        assert len(iou) == 0 or np.abs(iou - thresh).min() >= 1e-6
        assert 1 <= len(pick) <= m and len(set(pick.tolist())) == len(pick)


def test_host_path_returns_the_reference_pick_lists(z):
    for k in range(int(z["n_cases"])):
        RT, scales, scores, thresh, pick, _ = _case(z, k)
        (got,) = E.nms_3d(RT, scales, scores, thresh)
        assert got.dtype == np.int64 and np.array_equal(got, pick), k


def test_host_iou_is_the_reference_iou_to_1e_6(z):
    worst = 0.0
    for k in range(int(z["n_cases"])):
        RT, scales, _, _, _, want = _case(z, k)
        m = len(RT)
        got = np.array([E.compute_3d_iou(RT[i], RT[j], scales[i], scales[j], False, None, None) for i in range(m) for j in range(i + 1, m)])
        if len(want):
            worst = max(worst, float(np.abs(got - want).max()))
    print("largest |host IoU - reference IoU|:", worst)
    assert worst <= 1e-6


def test_equal_scores_the_higher_index_goes_first():
    RT, sc = _boxes([[0, 0, 0]] * 3)
    (got,) = E.nms_3d(RT, sc, [0.5, 0.5, 0.5], 0.3)
    assert got.tolist() == [2]
    # disjoint boxes with equal scores are all kept, in descending index
    RT, sc = _boxes([[0, 0, 0], [5, 0, 0], [0, 5, 0]])
    (got,) = E.nms_3d(RT, sc, [1.0, 1.0, 1.0], 0.3)
    assert got.tolist() == [2, 1, 0]


def test_the_comparison_is_strict():
    RT, sc = _boxes([[0, 0, 0]] * 4)
    scores = [0.1, 0.4, 0.3, 0.2]
    assert E.compute_3d_iou(RT[0], RT[1], sc[0], sc[1], False, None, None) == 1.0
    (got,) = E.nms_3d(RT, sc, scores, 1.0)                        # IoU 1.0 is not > 1.0
    assert got.tolist() == [1, 2, 3, 0]
    # thresh 0: one box of every overlapping cluster -- two clusters of touching-and-overlapping boxes, far apart
    RT, sc = _boxes([[0, 0, 0], [0.5, 0, 0], [0.9, 0, 0], [10, 0, 0], [10.2, 0.1, 0]])
    (got,) = E.nms_3d(RT, sc, [5, 4, 3, 2, 1], 0.0)
    assert got.tolist() == [0, 3]
    RT, sc = _boxes([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3]])     # disjoint: all kept, by score
    (got,) = E.nms_3d(RT, sc, [1, 4, 2, 3], 0.0)
    assert got.tolist() == [1, 3, 2, 0]


def test_degenerate_predictions_are_dropped_and_indices_refer_to_the_input():
    RT, sc = _boxes([[0, 0, 0], [0, 0, 0], [4, 0, 0], [4, 0, 0], [8, 0, 0], [8, 0, 0], [12, 0, 0], [12, 0, 0], [16, 0, 0], [16, 0, 0]])
    scores = np.array([9.0, 1.0, 9.0, 1.0, 9.0, 1.0, 9.0, 1.0, 9.0, 1.0])
    RT[0, 0, 3] = np.nan                                          # non-finite pose
    RT[2, :3, :3] = 0.0                                           # singular rotation block
    sc[4, 1] = 0.0                                                # zero extent
    RT[6, 3] = [0, 0, 0, 2]                                       # wrong last row
    scores[8] = np.inf                                            # non-finite score
    (got,) = E.nms_3d(RT, sc, scores, 0.3)
    assert sorted(got.tolist()) == [1, 3, 5, 7, 9]                # the low-scored twin of every dropped box survives
    sc2 = sc.copy()
    sc2[5] = [np.nan, 1, 1]
    sc2[7, 2] = -1.0
    (got,) = E.nms_3d(RT, sc2, scores, 0.3)
    assert sorted(got.tolist()) == [1, 3, 9]
    assert [g.tolist() for g in E.nms_3d(RT[:0], sc[:0], scores[:0], 0.3)] == [[]]
    with pytest.raises(ValueError):
        E.nms_3d(RT, sc[:3], scores, 0.3)


def test_groups_are_suppressed_separately():
    RT, sc = _boxes([[0, 0, 0]] * 5)
    got = E.nms_3d(RT, sc, [1, 2, 3, 4, 5], 0.3, groups=[2, 0, 2, 0, 0])
    assert [g.tolist() for g in got] == [[4], [], [2]]


def _results():
    rng = np.random.default_rng(3)
    RT, sc = _boxes([[0, 0, 0], [0, 0, 0], [0.05, 0, 0], [3, 0, 0], [0, 0, 0]])
    RT[:, :3, :3] *= 2.0                                          # a scaled rotation block: extents 2 * scales in the metric
    a = dict(gt_class_ids=np.array([1]), gt_RTs=RT[:1].copy(), gt_scales=sc[:1].copy(), gt_up_syms=np.array([False]),
             pred_class_ids=np.array([1, 2, 1, 1, 1]), pred_RTs=RT, pred_scales=sc, pred_scores=np.array([0.9, 0.8, 0.95, 0.2, 0.5]),
             pred_bboxes=rng.integers(0, 100, size=(5, 4)), other="kept")
    b = dict(gt_class_ids=np.zeros(0, int), gt_RTs=np.zeros((0, 4, 4)), gt_scales=np.zeros((0, 3)), gt_up_syms=np.zeros(0, bool),
             pred_class_ids=np.zeros(0, int), pred_RTs=np.zeros((0, 4, 4)), pred_scales=np.zeros((0, 3)), pred_scores=np.zeros(0))
    RT2, sc2 = _boxes([[1, 1, 1], [1, 1, 1]])
    c = dict(gt_class_ids=np.array([2]), gt_RTs=RT2[:1].copy(), gt_scales=sc2[:1].copy(), gt_up_syms=np.array([False]),
             pred_class_ids=np.array([2, 2]), pred_RTs=RT2, pred_scales=sc2, pred_scores=np.array([0.3, 0.3]))
    return [a, b, c]


def test_nms_results_keeps_the_arrays_in_step_and_the_input_untouched():
    import copy
    res = _results()
    before = copy.deepcopy(res)
    out = E.nms_results(res, 0.3)
    for r, q in zip(res, before):
        assert r.keys() == q.keys() and all(np.array_equal(r[k], q[k]) for k in r)
    a, b, c = out
    # image 0: class 1 = predictions 0, 2, 3, 4 (0, 2 and 4 overlap: 2 has the best score), class 2 = prediction 1, coincident with 0
    # and kept all the same: classes are suppressed separately
    keep = [2, 3, 1]
    for key in ("pred_class_ids", "pred_RTs", "pred_scales", "pred_scores", "pred_bboxes"):
        assert np.array_equal(a[key], res[0][key][keep]), key
    assert a["other"] == "kept" and a["gt_RTs"] is res[0]["gt_RTs"]
    assert len(b["pred_class_ids"]) == 0 and b["pred_RTs"].shape == (0, 4, 4)
    assert c["pred_scores"].tolist() == [0.3] and np.array_equal(c["pred_RTs"], res[2]["pred_RTs"][[1]])   # the tie rule
    assert "pred_bboxes" not in c
    E.compute_degree_cm_mAP(out, ["BG", "a", "b"], None)          # the format the metric reads


# ------------------------------------------------------------------------------------------------ the C entry point, no device
def _entry():
    from cppf_amd import _lib
    return _lib.lib()


def _call(L, n, off, G, ws_bytes=None, nul=(), thresh=0.3):
    """cppf_box_nms_batch with fake non-null device pointers: every case here returns before anything is touched"""
    fake = C.c_void_p(0x1000)
    ptr = {k: (None if k in nul else fake) for k in ("RT", "scales", "scores", "pick", "n_pick", "ws")}
    table = np.ascontiguousarray(off, np.int32)                   # (kept alive until the call has returned)
    off_a = None if "off" in nul else table.ctypes.data
    need = L.cppf_box_nms_workspace_bytes(n, G) if ws_bytes is None else ws_bytes
    return L.cppf_box_nms_batch(ptr["RT"], ptr["scales"], ptr["scores"], n, off_a, G, thresh, ptr["pick"], ptr["n_pick"], None, ptr["ws"],
                                need, None)


def test_workspace_bytes():
    L = _entry()
    w = L.cppf_box_nms_workspace_bytes
    assert w(-1, 1) == 0 and w(1, -1) == 0
    # three offset tables (256-byte aligned each) and the bit matrices: at most n rows of min(16, ceil(n / 64)) words
    assert w(10, 1) == 3 * 256 + 256
    assert w(130, 3) == 3 * 256 + 130 * 3 * 8 + (-(130 * 3 * 8)) % 256
    assert w(5000, 100) == 512 + 2 * 1024 + 5000 * 16 * 8 + (-(5000 * 16 * 8)) % 256
    assert w(0, 0) == 3 * 256
    assert w(2000, 2) > w(1000, 2) > w(100, 2)


def test_entry_point_refusals_need_no_device():
    L = _entry()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
    assert _call(L, 3, [0, 1, 3], 2, nul=("ws",)) == EWORKSPACE          # (a good call up to the workspace)
    for name in ("RT", "scales", "scores", "pick", "n_pick", "off"):
        assert _call(L, 3, [0, 1, 3], 2, nul=(name,)) == EINVAL, name
    assert _call(L, -1, [0, 0], 1) == EINVAL and _call(L, 3, [0, 3], -1) == EINVAL
    assert _call(L, 3, [0, 2, 1, 3], 3) == EINVAL                         # a table that decreases
    assert _call(L, 3, [0, 1, 2], 2) == EINVAL                            # ... that does not end at n
    assert _call(L, 3, [1, 2, 3], 2) == EINVAL                            # ... that does not start at 0
    assert _call(L, 1025, [0, 1025], 1) == EUNSUPPORTED                   # a group above CPPF_BOX_NMS_GROUP_CAP
    assert _call(L, 2048, [0, 1024, 2048], 2, ws_bytes=16) == EWORKSPACE  # two full groups are fine; the workspace is short
    assert _call(L, 3, [0, 1, 3], 2, ws_bytes=L.cppf_box_nms_workspace_bytes(3, 2) - 1) == EWORKSPACE
    # more than 2^31 - 1 pairs in one call: 4 101 groups of 1 024
    G = 4101
    assert _call(L, 1024 * G, np.arange(G + 1) * 1024, G) == EUNSUPPORTED
    assert _call(L, 1024 * 4100, np.arange(4101) * 1024, 4100, ws_bytes=16) == EWORKSPACE
    # nothing to do: 0, whatever else is passed
    assert _call(L, 0, [0, 0, 0], 2, nul=("RT", "scales", "scores", "pick", "n_pick", "ws")) == 0
    assert _call(L, 5, [0], 0, nul=("RT", "ws")) == 0


def test_device_path_refuses_an_oversized_group_before_any_upload():
    RT, sc = _boxes(np.zeros((1025, 3)))
    with pytest.raises(ValueError, match="1025"):
        E.nms_3d(RT, sc, np.arange(1025.0), 0.3, device="cuda:0")
