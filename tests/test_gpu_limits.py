"""The newest kernels at their documented caps and on the second trip of their grid-stride loops (cases: tests/limits_cases.py,
their conditions: tests/test_limits_cpu.py): cppf_raster_instances with more than one instance per lane of its scan,
cppf_box_nms_batch at the group cap, in the last word of a row and over thousands of groups, cppf_pose_eval_pairs across the
trip boundary, cppf_gaussian_filter3d / cppf_scene_proposals at radius 0 / 31 / 32 and margin 1 / 64, and the pair filter and
the instance segmentation of csrc/scene.hip beyond one trip, with both index widths and with indices outside the cloud.

Every expected value is a closed form, a numpy / fp64 reference checked on the CPU, or an invariance (the same pairs in single-trip
chunks, the same instances in reverse) -- never the kernel under test at the same shape."""
import numpy as np
import pytest
import torch

import limits_cases as LC
import zero_shot_ref as Z
from cppf_amd import _lib, zero_shot
from cppf_amd import evaluation as E
from cppf_amd import meshes as M
from cppf_amd._torch_util import call, scratch
from test_gpu_box_nms import _lists, _pairs_iou, _run

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. instances: K > 1024
def _render(dev, K, order=None):
    meshes, inst, mvs = LC.instances_case()
    inst, mvs = inst[:K], mvs[:K]
    if order is not None:
        inst, mvs = inst[order], mvs[order]
    depth, labels = M.render_instances(meshes, inst, mvs, fx=LC.INST_FX, fy=LC.INST_FY, width=LC.INST_W, height=LC.INST_H, device=dev)
    return depth.cpu().numpy(), labels.cpu().numpy()


@pytest.mark.parametrize("K", LC.INST_KS)
def test_instances_with_several_per_scan_lane(dev, K):
    """rs_inst_scan_kernel gives each of its 1024 lanes ceil(K / 1024) instances: 1, 2, 3 and 4 here, the last lanes fewer"""
    assert -(-K // LC.SCAN_LANES) == 1 + LC.INST_KS.index(K) and (K > 1024 or K == LC.INST_KS[0])
    d, l = _render(dev, K)
    # the known answer: every label appears, inside its own cell only, and nothing else is covered
    assert np.array_equal(np.unique(l), np.arange(-1, K))
    rows, cols = np.nonzero(l >= 0)
    assert np.array_equal(l[rows, cols], LC.cell_of_pixels(rows, cols))
    assert np.array_equal(d > 0, l >= 0)
    # the restatement, bit for bit
    rd, rl = LC.instances_ref()[K]
    assert np.array_equal(l, rl), int((l != rl).sum())
    assert np.array_equal(_u32(d), _u32(rd))


def test_instances_listed_in_reverse_give_the_same_image(dev):
    K = 2049
    assert K > LC.SCAN_LANES
    d, l = _render(dev, K, np.arange(K)[::-1])
    rd, rl = LC.instances_ref()[K]
    assert np.array_equal(l, np.where(rl >= 0, K - 1 - rl, -1)) and np.array_equal(_u32(d), _u32(rd))


def test_instances_above_the_cap_are_refused_and_nothing_is_written(dev):
    K = LC.RS_MAX_INST + 1
    meshes, _, mvs = LC.instances_case()
    ms = M.mesh_set(meshes, dev)
    W, H = LC.INST_W, LC.INST_H
    depth = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    labels = torch.full((H, W), 7, dtype=torch.int32, device=dev)
    ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    assert _lib.lib().cppf_raster_instances_workspace_bytes(K, 2 * K, ms.n, W, H, 1 << 20) == 0
    assert _lib.lib().cppf_raster_instances_workspace_bytes(K - 1, 2 * K, ms.n, W, H, 1 << 20) > 0
    rc = call("cppf_raster_instances", dev, ms.v, ms.f, ms.vert_off, ms.face_off, ms.n, np.zeros(K, np.int32),
              np.ascontiguousarray(np.tile(mvs[0, :3], (K, 1, 1))), K, LC.INST_FX, LC.INST_FY, W, H, M.ZNEAR, True, depth, labels, 1 << 20, True,
              scratch(ws), ok=(EINVAL,))
    torch.cuda.synchronize(dev)
    assert rc == EINVAL and (depth == 7.0).all() and (labels == 7).all() and (ws == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 2. NMS: the cap, the last word
@pytest.mark.parametrize("m", LC.NMS_SIZES)
def test_nms_group_at_the_cap_and_in_the_last_word(dev, m):
    """Axis-aligned boxes, so the IoU is a closed form: the pick list, the bit matrix and iou_out against it; iou_out also
    against cppf_pose_eval_pairs bit for bit.  The tolerance on iou_out is 4 x the largest deviation of evaluation.py's fp64 path
    from the closed form on these boxes, measured at 7.22e-16 (limits_cases.NMS_HOST_IOU_DEVIATION): 2.92e-15."""
    assert max(LC.NMS_SIZES) == LC.NMS_GROUP_CAP and m <= LC.NMS_GROUP_CAP
    assert ((m + 63) // 64, m % 64) in ((15, 0), (16, 1), (16, 63), (16, 0))      # full rows of 15 / 16 words, one bit and 63 in word 15
    RT, scales, scores, want_iou = LC.nms_group(m)
    pick, n_pick, iou, bits = _run(dev, RT, scales, scores, [m], LC.NMS_THRESH)
    over = want_iou > LC.NMS_THRESH
    (got,) = _lists(pick, n_pick, [m])
    assert got == LC.greedy_pick(scores, over)
    assert np.array_equal(bits, LC.pack_bits(over))
    pairs = m * (m - 1) // 2
    assert iou.shape == (pairs,) and pairs <= LC.PE_LANES_TOTAL                   # (one trip of pe_pairs_kernel)
    assert np.array_equal(_u64(iou), _u64(_pairs_iou(dev, RT, scales)))
    worst = float(np.abs(iou - want_iou[np.triu_indices(m, 1)]).max())
    print("largest |iou_out - closed form|:", worst)
    assert worst <= 4 * LC.NMS_HOST_IOU_DEVIATION


def test_nms_three_thousand_groups_in_one_call(dev):
    RT, scales, scores, sizes, ious = LC.nms_many_groups()
    assert len(sizes) == 3000 and (sizes * (sizes - 1) // 2).sum() > 2048 * 64     # nms_over_kernel's stride loop, across groups
    pick, n_pick, iou, bits = _run(dev, RT, scales, scores, sizes.tolist(), LC.NMS_THRESH)
    starts = np.cumsum(sizes) - sizes
    want = [LC.greedy_pick(scores[a:a + m], u > LC.NMS_THRESH) for a, m, u in zip(starts, sizes, ious)]
    assert _lists(pick, n_pick, sizes.tolist()) == want
    assert np.array_equal(bits, np.concatenate([LC.pack_bits(u > LC.NMS_THRESH) for u in ious]))
    want_iou = np.concatenate([u[np.triu_indices(len(u), 1)] for u in ious])
    assert np.abs(iou - want_iou).max() <= 4 * LC.NMS_HOST_IOU_DEVIATION
    pick2, n_pick2, _, bits2 = _run(dev, RT, scales, scores, sizes.tolist(), LC.NMS_THRESH)
    assert pick.tobytes() == pick2.tobytes() and n_pick.tobytes() == n_pick2.tobytes() and bits.tobytes() == bits2.tobytes()


def test_nms_coincident_geometry(dev):
    """identical boxes (IoU 1), boxes that share a face (0), a box inside another (the ratio of the volumes): the device through
    both entry points, the host path and the closed form agree"""
    RT, scales, pairs, want = LC.coincident_boxes()
    host = np.array([E.compute_3d_iou(RT[a], RT[b], scales[a], scales[b], False, None, None) for a, b in pairs])
    iou, _, _ = E.pose_metrics_device(RT, scales, RT, scales, np.zeros(len(RT), np.int32), pairs, np.zeros(len(pairs), np.int32), device=dev)
    iou = iou.cpu().numpy()
    print("device", iou, "host", host, "closed form", want)
    np.testing.assert_allclose(iou, want, atol=1e-9, rtol=0)
    np.testing.assert_allclose(iou, host, atol=1e-9, rtol=0)
    assert iou[1] == 0.0 and host[1] == 0.0
    for (a, b), v, w in zip(pairs, iou, want):                                     # cppf_box_nms_batch: the same bits, the same decision
        pick, n_pick, out, _ = _run(dev, RT[[a, b]], scales[[a, b]], np.array([1.0, 2.0]), [2], 0.04)
        assert np.array_equal(_u64(out), _u64(np.array([v]))) and _lists(pick, n_pick, [2]) == [[1] if w > 0.04 else [1, 0]]


def test_nms_group_above_the_cap_is_refused_and_nothing_is_written(dev):
    m = LC.NMS_GROUP_CAP + 1
    RT, scales, scores = LC.aligned_boxes(np.random.default_rng(1), m)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    pick = torch.full((m,), -7, dtype=torch.int32, device=dev)
    n_pick = torch.full((1,), -7, dtype=torch.int32, device=dev)
    iou = torch.full((m * (m - 1) // 2,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.full((_lib.lib().cppf_box_nms_workspace_bytes(m, 1),), 0xA5, dtype=torch.uint8, device=dev)
    rc = call("cppf_box_nms_batch", dev, d(RT), d(scales), d(scores), m, np.array([0, m], np.int32), 1, LC.NMS_THRESH, pick, n_pick, iou,
              scratch(ws), ok=(EUNSUPPORTED,))
    torch.cuda.synchronize(dev)
    assert rc == EUNSUPPORTED
    assert (pick == -7).all() and (n_pick == -7).all() and (iou == -7.0).all() and (ws == 0xA5).all()     # not even the tables were copied


# ------------------------------------------------------------------------------------------------ 3. pose-eval pairs: the second trip
class _PoseCase:
    def __init__(self, dev, n_plain, n_swept):
        self.c = c = LC.pose_eval_case(n_plain, n_swept, 7)
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        self.boxes = (f64(c["pred_RT"]), f64(c["pred_scales"]), f64(c["gt_RT"]), f64(c["gt_scales"]), torch.from_numpy(c["up_sym"]).to(dev))
        self.dev = dev

    def run(self, pairs, sweep):
        """(iou, degrees, centimetres) as numpy; `pairs` goes in as a device tensor: an index outside the arrays gives NaN"""
        a, b, c_, d, e = self.boxes
        out = E.pose_metrics_device(a, b, c_, d, e, torch.from_numpy(np.ascontiguousarray(pairs)).to(self.dev),
                                    torch.from_numpy(np.ascontiguousarray(sweep)).to(self.dev))
        return [t.cpu().numpy() for t in out]

    def host(self, p):
        c = self.c
        ip, ig = c["pairs"][p]
        v = E.compute_3d_iou(c["pred_RT"][ip], c["gt_RT"][ig], c["pred_scales"][ip], c["gt_scales"][ig], bool(c["sweep"][p]), "a", "a")
        return (v,) + tuple(E.compute_RT_degree_cm_symmetry(c["pred_RT"][ip], c["gt_RT"][ig], bool(c["up_sym"][ig])))


@pytest.mark.parametrize("n_plain,n_swept,n_host", [(0, 26300, 60), (300000, 12000, 140)], ids=["swept", "mixed"])
def test_pose_eval_pairs_across_the_trip_boundary(dev, n_plain, n_swept, n_host):
    """More work items than pe_pairs_kernel's 8192 x 64 lanes.  Invariance: the same pairs in single-trip chunks (the shape the
    fixtures and the closed forms pin) give the same bits.  Independently: 200 pairs over the two cases, the ones around the trip
    boundary among them, against evaluation.py's fp64 path at test_gpu_evaluation.py's bounds."""
    pc = _PoseCase(dev, n_plain, n_swept)
    c = pc.c
    items = int(c["item_off"][-1])
    assert items == n_plain + LC.PE_SYM * n_swept and items > 8192 * 64
    iou, deg, cm = pc.run(c["pairs"], c["sweep"])
    n = len(c["pairs"])
    for a in range(0, n, LC.PE_CHUNK):
        sl = slice(a, min(n, a + LC.PE_CHUNK))
        assert (c["item_off"][sl.stop] - c["item_off"][sl.start]) <= 8192 * 64            # one trip
        i2, d2, c2 = pc.run(c["pairs"][sl], c["sweep"][sl])
        assert np.array_equal(_u64(iou[sl]), _u64(i2)) and np.array_equal(_u64(deg[sl]), _u64(d2)) and np.array_equal(_u64(cm[sl]), _u64(c2)), a
    p = LC.straddling_pair(c["item_off"])
    if not n_plain:
        assert c["sweep"][p] and c["item_off"][p] < 8192 * 64 < c["item_off"][p + 1]      # its 20 items lie on both sides
    sel = np.unique(np.concatenate([np.random.default_rng(3).choice(n, n_host - 5, replace=False), np.arange(p - 2, p + 3)]))
    host = np.array([pc.host(q) for q in sel])
    print("max |iou - host|", np.abs(iou[sel] - host[:, 0]).max(), "deg", np.abs(deg[sel] - host[:, 1]).max(), "cm", np.abs(cm[sel] - host[:, 2]).max())
    np.testing.assert_allclose(iou[sel], host[:, 0], atol=1e-9, rtol=0)
    np.testing.assert_allclose(cm[sel], host[:, 2], atol=1e-9, rtol=0)
    np.testing.assert_allclose(deg[sel], host[:, 1], atol=1e-5, rtol=0)
    assert (iou[sel] > 0).sum() > 10 and np.isfinite(iou).all() and iou.min() >= 0 and iou.max() <= 1


def test_pose_eval_index_outside_the_arrays_in_the_second_trip(dev):
    pc = _PoseCase(dev, 0, 26300)
    c = pc.c
    p = LC.straddling_pair(c["item_off"])
    clean = pc.run(c["pairs"], c["sweep"])
    pairs = c["pairs"].copy()
    bad = {p + 1: (0, LC.PE_N_BOXES), p + 5: (LC.PE_N_BOXES, 3), p + 9: (4, -1), len(pairs) - 1: (LC.INT32_MAX, 5)}
    for q, v in bad.items():
        assert c["item_off"][q] >= 8192 * 64                                               # every item of these pairs: second trip
        pairs[q] = v
    got = pc.run(pairs, c["sweep"])
    rest = np.setdiff1d(np.arange(len(pairs)), list(bad))
    for g, w in zip(got, clean):
        assert np.isnan(g[list(bad)]).all() and np.array_equal(_u64(g[rest]), _u64(w[rest]))


# ------------------------------------------------------------------------------------------------ 4. smoothing and proposals
@pytest.mark.parametrize("sigma,truncate,radius", LC.SMOOTH_PARAMS)
def test_smooth_at_radius_0_31_32(dev, sigma, truncate, radius):
    assert radius in (0, LC.SCN_MAX_RADIUS - 1, LC.SCN_MAX_RADIUS)
    assert (zero_shot.gaussian_weights(sigma, truncate).shape[0] - 1) // 2 == radius
    for shape in LC.SMOOTH_GRIDS:                                  # lines shorter than the radius: the reflection repeats
        g = LC.smooth_grid_case(shape)
        got = zero_shot.smooth_grid(g, sigma, truncate)
        assert np.array_equal(_u32(got), _u32(Z.smooth(g, sigma, truncate))), shape
        if radius == 0:
            assert np.array_equal(_u32(got), _u32(g))


def test_radius_33_is_refused(dev):
    g = LC.smooth_grid_case((2, 2, 2))
    with pytest.raises(ValueError, match="33"):
        zero_shot.smooth_grid(g, 1.0, 33.0)
    with pytest.raises(ValueError, match="33"):
        zero_shot.scene_proposals_device(g, 1.0, truncate=33.0)


def _proposals(dev, g, smoothed, **kw):
    """scene_proposals_device on grid g against Z.proposals on the restatement's smoothed grid, bit for bit -> the rows"""
    loc, val, diff, count = zero_shot.scene_proposals_device(torch.from_numpy(g).to(dev), **kw)
    n = int(count.item())
    el, ev, ed, _ = Z.proposals(smoothed, kw.get("thresh", 50), kw.get("margin", 10), kw.get("max_proposals", 32), kw.get("max_iters"))
    assert n == el.shape[0], (n, el.shape[0])
    assert np.array_equal(loc[:n].cpu().numpy(), el)
    assert np.array_equal(_u32(val[:n].cpu().numpy()), _u32(ev)) and np.array_equal(_u32(diff[:n].cpu().numpy()), _u32(ed))
    return el


@pytest.mark.parametrize("margin", [64, 1])
def test_proposals_at_margin_64_and_1(dev, margin):
    """peaks in a corner cell, on a face, inside and in the opposite corner of a 140 x 137 x 131 grid: the boxes clip at both ends
    and end inside the last, partial tiles; at margin 64 the interior box has 128-cell edges"""
    assert margin in (1, LC.SCN_MAX_MARGIN) and all(d % 8 for d in LC.MARGIN_GRID)
    g = LC.margin_grid()
    sm = torch.empty(g.shape, dtype=torch.float32, device=dev)
    loc = _proposals(dev, g, LC.margin_grid_smoothed(), margin=margin, smoothed_out=sm)
    assert np.array_equal(_u32(sm.cpu().numpy()), _u32(LC.margin_grid_smoothed()))
    assert loc.shape[0] >= 4 and {tuple(r) for r in loc.tolist()} == set(LC.MARGIN_PEAKS)
    small = LC.smooth_grid_case((33, 7, 70))                      # boxes wider than the grid in one axis, narrower in another
    assert _proposals(dev, small, Z.smooth(small), margin=margin, thresh=1.0).shape[0] >= 1


def test_equal_maxima_in_different_tiles_come_in_flat_index_order(dev):
    g = LC.plateau_grid()
    loc = _proposals(dev, g, g, truncate=0.0, margin=3, max_proposals=5)          # radius 0: the ties survive the smoothing
    assert loc.tolist() == [list(c) for c in LC.plateau_order()]


def test_proposal_loop_bounds(dev):
    g = LC.plateau_grid()
    kw = dict(truncate=0.0, margin=3)
    assert _proposals(dev, g, g, max_proposals=0, **kw).shape[0] == 0
    assert _proposals(dev, g, g, max_iters=0, **kw).shape[0] == 0
    assert _proposals(dev, g, g, max_iters=1, **kw).shape[0] == 1
    zero = np.zeros((9, 10, 11), np.float32)
    assert _proposals(dev, zero, Z.smooth(zero)).shape[0] == 0
    assert _proposals(dev, zero, Z.smooth(zero), thresh=-1.0, margin=3).shape[0] >= 1      # diff 0 > -1: proposed, then repeated
    neg = np.full((9, 10, 11), -5.0, np.float32)
    assert _proposals(dev, neg, Z.smooth(neg)).shape[0] == 0
    assert _proposals(dev, neg, Z.smooth(neg), thresh=-1.0, margin=3).shape[0] >= 1


# ------------------------------------------------------------------------------------------------ 5. pair filter, segmentation
@pytest.mark.parametrize("width", ["i64", "i32"])
def test_pair_filter_beyond_one_trip(dev, width):
    """4 194 304 + 333 pairs: every lane of the capped grid takes a second trip or is in the ragged tail; then the same list with
    about 1000 endpoints at -1, N or the largest index (for int64 also 2^32 + 7): those pairs are dropped"""
    assert LC.SCENE_P > 16384 * 256
    pc, nrm = LC.scene_cloud()
    dpc, dnrm = torch.from_numpy(pc).to(dev), torch.from_numpy(nrm).to(dev)
    for bad in (None, width):
        idx, pos, _ = LC.scene_pairs(bad)
        idx = idx if width == "i64" else idx.astype(np.int32)
        keep = LC.scene_distinct(bad)
        assert not keep[pos].any() and 0.1 < keep.mean() < 0.9
        kept = zero_shot.distinct_pairs(dpc, dnrm, torch.from_numpy(idx).to(dev))
        assert kept.dtype == (torch.int64 if width == "i64" else torch.int32)
        assert np.array_equal(kept.cpu().numpy(), idx[keep]), bad


def test_segmentation_beyond_one_trip_with_bad_endpoints(dev):
    assert LC.SCENE_P > 16384 * 256
    idx, pos, side = LC.scene_pairs("i32")
    surv = LC.scene_survivors()
    P, N = LC.SCENE_P, LC.SCENE_N
    want_pm, want_pos = Z.segment(idx, surv, N, LC.SCENE_MIN_CONTRIB)
    assert 0 < want_pm.sum() < N and 0 < len(want_pos) < surv.sum() and surv[pos].sum() > 400
    L = _lib.lib()
    pm = torch.empty(N, dtype=torch.uint8, device=dev)
    pairs = torch.empty(P, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.cppf_segment_instance_workspace_bytes(N, P), dtype=torch.uint8, device=dev)
    call("cppf_segment_instance", dev, torch.from_numpy(idx.astype(np.int32)).to(dev), torch.from_numpy(surv.astype(np.uint8)).to(dev), P, N,
         LC.SCENE_MIN_CONTRIB, pm, pairs, cnt, scratch(ws))
    n = int(cnt.item())
    assert np.array_equal(pm.cpu().numpy().astype(bool), want_pm)
    assert n == len(want_pos) and np.array_equal(pairs[:n].cpu().numpy(), want_pos)
