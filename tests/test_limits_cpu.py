"""The conditions of tests/limits_cases.py without a device: the references alone satisfy what tests/test_gpu_limits.py relies on
-- the limits are really reached, every instance owns pixels of its own cell only, no closed-form IoU lies near the NMS threshold,
the last word of every removed set decides, the margin-64 grid yields at least four proposals, and every mask has both values."""
import numpy as np
import pytest

import limits_cases as LC
import mesh_frames_ref as FR
import zero_shot_ref as Z
from cppf_amd import evaluation as E


# ------------------------------------------------------------------------------------------------ 1. instances
def test_instance_counts_reach_two_three_and_four_per_lane():
    assert [-(-K // LC.SCAN_LANES) for K in LC.INST_KS] == [1, 2, 3, 4]
    for K in LC.INST_KS[1:]:
        per = -(-K // LC.SCAN_LANES)
        assert K > LC.SCAN_LANES and (K % per != 0 or -(-K // per) < LC.SCAN_LANES)        # the last lanes hold fewer than `per`
    assert LC.INST_K_MAX <= LC.INST_COLS * LC.INST_ROWS and LC.INST_K_MAX < LC.RS_MAX_INST
    meshes, inst, _ = LC.instances_case()
    faces = np.array([m[1].shape[0] for m in meshes])[inst]
    assert set(inst.tolist()) == {0, 1, 2} and len(set(np.diff(np.cumsum(faces)[::7]).tolist())) > 5      # irregular prefix sums


def test_every_instance_owns_pixels_of_its_own_cell_only():
    for K, (depth, labels) in LC.instances_ref().items():
        counts = np.bincount(labels[labels >= 0], minlength=K)
        assert counts.shape[0] == K and counts.min() >= 4, (K, counts.min())
        rows, cols = np.nonzero(labels >= 0)
        assert np.array_equal(labels[rows, cols], LC.cell_of_pixels(rows, cols)), K
        assert np.array_equal(depth > 0, labels >= 0) and depth[labels >= 0].min() > 0.79 and depth.max() < 1.61


def test_no_pixel_is_claimed_by_two_instances_and_the_streaming_composition_is_the_rule():
    meshes, inst, mvs = LC.instances_case()
    import mesh_ref as R
    K = 300
    singles = [R.raster_ref(*meshes[m], mv, LC.INST_FX, LC.INST_FY, LC.INST_W, LC.INST_H) for m, mv in zip(inst[:K], mvs[:K])]
    assert np.sum([s > 0 for s in singles], 0).max() == 1
    # the composition rule on overlapping images: the minimum depth, on equal depth the lowest index (argmin: the first)
    rng = np.random.default_rng(0)
    imgs = [np.where(rng.random((6, 7)) < 0.6, rng.integers(1, 4, (6, 7)), 0).astype(np.float32) for _ in range(9)]
    d, l = FR._compose(iter(imgs))
    stack = np.stack([np.where(s > 0, s, np.inf) for s in imgs])
    assert np.array_equal(d, np.where(np.isinf(stack.min(0)), 0, stack.min(0)))
    assert np.array_equal(l, np.where(np.isinf(stack.min(0)), -1, stack.argmin(0)))
    part = FR._compose(iter(imgs), at=(4, 9))
    assert np.array_equal(part[9][0], d) and np.array_equal(part[9][1], l) and np.array_equal(part[4][1], FR._compose(iter(imgs[:4]))[1])


def test_restatement_agrees_with_the_ray_caster_on_a_subset():
    """200 instances spread over the 3100: labels equal and depths within 1e-5 (relative) at every pixel farther than 0.05 px from
    a projected edge.  The rays of an instance are cast in a window of 8 pixels around its cell; that it covers nothing outside
    its cell is test_every_instance_owns_pixels_of_its_own_cell_only."""
    meshes, inst, mvs = LC.instances_case()
    sel = np.sort(np.random.default_rng(2).choice(LC.INST_K_MAX, 200, replace=False))
    win = LC.instance_windows(LC.INST_K_MAX)[sel]
    args = (meshes, inst[sel], mvs[sel], LC.INST_FX, LC.INST_FY, LC.INST_W, LC.INST_H)
    rd, rl = FR.raster_instances_ref(*args)
    cd, cl = FR.ray_cast_instances(*args, windows=win)
    far = FR.edge_distance_instances(*args, windows=win) > 0.05
    assert far.mean() > 0.95 and (rl >= 0)[far].sum() > 4 * 200 * 0.5
    assert np.array_equal(rl[far], cl[far])
    hit = far & (rl >= 0)
    assert np.abs(rd[hit] / cd[hit] - 1).max() < 1e-5
    three = (meshes, inst[sel][:3], mvs[sel][:3]) + args[3:]                              # the windows change nothing
    full, part = FR.ray_cast_instances(*three), FR.ray_cast_instances(*three, windows=win[:3])
    assert np.array_equal(full[0], part[0]) and np.array_equal(full[1], part[1])


# ------------------------------------------------------------------------------------------------ 2. NMS
def _upper(iou):
    return iou[np.triu_indices(len(iou), 1)]


@pytest.mark.parametrize("m", LC.NMS_SIZES)
def test_nms_groups_meet_their_conditions(m):
    RT, scales, scores, iou = LC.nms_group(m)
    assert m <= LC.NMS_GROUP_CAP and (m + 63) // 64 == {960: 15}.get(m, 16)
    assert np.array_equal(RT[:, :3, :3], np.tile(np.eye(3), (m, 1, 1))) and set(np.unique(scales)) == set(LC.NMS_EDGES)
    assert np.abs(_upper(iou) - LC.NMS_THRESH).min() > 1e-6                              # no IoU near the threshold
    lo, hi = RT[:, :3, 3] - 0.5 * scales, RT[:, :3, 3] + 0.5 * scales
    assert np.diff(np.sort(np.concatenate([lo, hi]), 0), axis=0).min() > 1e-10           # no two faces coplanar
    ov = np.clip(np.minimum(hi[:, None], hi[None]) - np.maximum(lo[:, None], lo[None]), 0, None).prod(-1)
    assert not ((ov > 0) & (ov < 1e-8 * scales.prod(-1).min())).any()                    # no sliver near the `<= 1e-9 -> 0` rule
    assert len(np.unique(scores)) == 7                                                   # ties everywhere
    pick = LC.greedy_pick(scores, iou > LC.NMS_THRESH)
    assert 0.4 * m < len(pick) < 0.6 * m, len(pick)                                      # roughly half are suppressed
    last_word = set(range(64 * ((m - 1) // 64), m))
    assert m - 1 not in pick and (len(last_word) == 1 or last_word & set(pick))          # the last word of the removed set decides
    words = LC.pack_bits(iou > LC.NMS_THRESH).reshape(m, -1)
    assert words[:, -1].any() and (m % 64 == 0 or int(words[:, -1].max()) < 1 << (m % 64))


def test_nms_tie_rule_of_the_walk():
    over = np.zeros((4, 4), bool)
    assert LC.greedy_pick(np.array([1.0, 1.0, 2.0, 1.0]), over) == [2, 3, 1, 0]
    over[3, 1] = over[1, 3] = True
    assert LC.greedy_pick(np.array([1.0, 1.0, 2.0, 1.0]), over) == [2, 3, 0]


def test_many_groups_meet_their_conditions():
    RT, scales, scores, sizes, ious = LC.nms_many_groups()
    assert len(sizes) == LC.NMS_MANY_GROUPS and set(sizes.tolist()) == set(LC.NMS_MANY_SIZES) and sizes.sum() == len(RT)
    pairs = sizes * (sizes - 1) // 2
    assert pairs[0] == pairs[1] == 0 and pairs[-1] == 0 and (pairs[1499:1502] == 0).all() and pairs[2] > 0 and pairs[-2] > 0
    assert (pairs == 0).mean() > 0.5 and pairs.sum() > 2048 * 64                         # most groups have no pairs; the stride loop
    assert min(np.abs(_upper(i) - LC.NMS_THRESH).min() for i in ious if len(i) > 1) > 1e-6
    n_pick = [len(LC.greedy_pick(scores[a:a + m], i > LC.NMS_THRESH)) for a, m, i in zip(np.cumsum(sizes) - sizes, sizes, ious)]
    assert any(k < m for k, m in zip(n_pick, sizes) if m == 2) and any(k == m for k, m in zip(n_pick, sizes) if m == 2)


def test_host_iou_deviation_from_the_closed_form():
    """the figure test_gpu_limits.py's iou_out tolerance is 4 x of: evaluation.py's fp64 path against the closed form"""
    RT, scales, _, iou = LC.nms_group(1024)
    i, j = np.triu_indices(1024, 1)
    rng = np.random.default_rng(0)
    sel = np.concatenate([rng.choice(np.nonzero(iou[i, j] > 0)[0], 600, replace=False), rng.choice(len(i), 100, replace=False)])
    host = np.array([E.compute_3d_iou(RT[a], RT[b], scales[a], scales[b], False, None, None) for a, b in zip(i[sel], j[sel])])
    worst = float(np.abs(host - iou[i[sel], j[sel]]).max())
    print("largest |host IoU - closed form|:", worst)
    assert worst <= LC.NMS_HOST_IOU_DEVIATION
    assert np.array_equal(LC.aligned_iou(RT, scales, i[sel], j[sel]), iou[i[sel], j[sel]])


def test_coincident_geometry_on_the_host_path():
    RT, scales, pairs, want = LC.coincident_boxes()
    got = np.array([E.compute_3d_iou(RT[a], RT[b], scales[a], scales[b], False, None, None) for a, b in pairs])
    np.testing.assert_allclose(got, want, atol=1e-9, rtol=0)
    assert got[1] == 0.0                                                                 # a shared face is no volume
    np.testing.assert_allclose(LC.aligned_iou(RT, scales, pairs[:, 0], pairs[:, 1]), want, atol=1e-15, rtol=0)
    # touching from opposite sides in every direction and order, rotated: still nothing; overlapping by a hair: that hair
    from scipy.spatial.transform import Rotation
    Q = np.eye(4)
    Q[:3, :3] = Rotation.from_rotvec([0.3, -1.1, 0.7]).as_matrix()
    for ax in range(3):
        for sgn in (1.0, -1.0):
            t = np.zeros(3)
            t[ax] = sgn
            for A, B in ((FR.model(np.zeros(3)), FR.model(t)), (FR.model(t), FR.model(np.zeros(3)))):
                assert E.compute_3d_iou(Q @ A, Q @ B, [1, 1, 1], [1, 1, 1], False, None, None) <= 1e-12, (ax, sgn)
            t[ax] = sgn * 0.999
            v = E.compute_3d_iou(Q @ FR.model(np.zeros(3)), Q @ FR.model(t), [1, 1, 1], [1, 1, 1], False, None, None)
            assert abs(v - 0.001 / 1.999) < 1e-9


# ------------------------------------------------------------------------------------------------ 3. pose-eval pairs
def test_pose_eval_cases_cross_the_trip_boundary():
    assert LC.PE_LANES_TOTAL % LC.PE_SYM != 0 and LC.PE_CHUNK * LC.PE_SYM <= LC.PE_LANES_TOTAL
    for n_plain, n_swept in ((0, 26300), (300000, 12000)):
        c = LC.pose_eval_case(n_plain, n_swept, 7)
        off = c["item_off"]
        assert off[-1] == n_plain + LC.PE_SYM * n_swept > LC.PE_LANES_TOTAL
        p = LC.straddling_pair(off)
        assert c["sweep"][p] or n_plain                       # all swept: the boundary pair is swept ...
        if not n_plain:
            assert off[p] < LC.PE_LANES_TOTAL < off[p + 1]    # ... and its 20 items lie on both sides
        assert c["pairs"].min() >= 0 and c["pairs"].max() < LC.PE_N_BOXES and set(np.unique(c["up_sym"])) == {0, 1}


# ------------------------------------------------------------------------------------------------ 4. smoothing, proposals
def test_smoothing_cases_reach_the_radii():
    from cppf_amd import zero_shot
    for sigma, truncate, radius in LC.SMOOTH_PARAMS:
        w = zero_shot.gaussian_weights(sigma, truncate)
        assert (w.shape[0] - 1) // 2 == radius and np.array_equal(w, Z.gaussian_weights(sigma, truncate))
    assert {p[2] for p in LC.SMOOTH_PARAMS} == {0, LC.SCN_MAX_RADIUS - 1, LC.SCN_MAX_RADIUS}
    with pytest.raises(ValueError):
        zero_shot.gaussian_weights(1.0, 33.0)
    assert min(min(s) for s in LC.SMOOTH_GRIDS) == 1 and any(max(s) > 2 * LC.SCN_MAX_RADIUS for s in LC.SMOOTH_GRIDS)
    # at sigma 8 the outermost weight reaches the float32 result: leaving it out changes the output
    g = LC.smooth_grid_case((65, 64, 9))
    assert not np.array_equal(Z.smooth(g, 8.0, 4.0), Z.smooth(g, 8.0, 3.9))


def test_margin_grid_yields_at_least_four_proposals():
    assert all(d % LC.SCN_TILE for d in LC.MARGIN_GRID) and min(LC.MARGIN_GRID) > 2 * LC.SCN_MAX_MARGIN
    loc, val, diff, it = Z.proposals(LC.margin_grid_smoothed(), 50, LC.SCN_MAX_MARGIN)
    assert loc.shape[0] >= 4 and {tuple(r) for r in loc.tolist()} == set(LC.MARGIN_PEAKS)
    assert loc[:4].tolist() == [list(LC.MARGIN_PEAKS[k]) for k in (0, 2, 1, 3)] and np.all(np.diff(val) <= 0)
    # the interior peak's box has 128-cell edges (the whole of np.mean's base case); the far corner's ends inside the last tiles
    assert all(min(d - 1, p + 64) - max(0, p - 64) == 128 for p, d in zip(LC.MARGIN_PEAKS[2], LC.MARGIN_GRID))
    assert sum((d - 1) // LC.SCN_TILE == (d - 2) // LC.SCN_TILE and d % LC.SCN_TILE != 0 for d in LC.MARGIN_GRID) >= 2
    assert Z.proposals(LC.margin_grid_smoothed(), 50, 1)[0].shape[0] >= 4


def test_plateau_proposals_come_in_flat_index_order():
    g = LC.plateau_grid()
    sm = Z.smooth(g, 1.0, 0.0)
    assert np.array_equal(sm, g) and (g == g.max()).sum() == 5 and np.array_equal(g, np.round(g))
    tiles = [tuple(c // LC.SCN_TILE for c in cell) for cell in LC.plateau_order()]
    dims = tuple(-(-d // LC.SCN_TILE) for d in LC.PLATEAU_GRID)
    flat = [(t[0] * dims[1] + t[1]) * dims[2] + t[2] for t in tiles]
    assert len(set(tiles)) == 5 and flat != sorted(flat) and np.prod(dims) > 1024
    loc, val, _, _ = Z.proposals(sm, 50, 3, max_proposals=5)
    assert loc.tolist() == [list(c) for c in LC.plateau_order()] and np.all(val == 1000.0)


def test_loop_bounds_of_the_restatement():
    sm = Z.smooth(LC.plateau_grid(), 1.0, 0.0)
    assert Z.proposals(sm, 50, 3, max_proposals=0)[0].shape[0] == 0
    assert Z.proposals(sm, 50, 3, max_iters=0)[0].shape[0] == 0
    assert Z.proposals(sm, 50, 3, max_iters=1)[0].shape[0] == 1
    assert Z.proposals(np.zeros((9, 10, 11), np.float32))[0].shape[0] == 0
    assert Z.proposals(np.full((9, 10, 11), -5.0, np.float32), thresh=-1.0, margin=3)[0].shape[0] >= 1


# ------------------------------------------------------------------------------------------------ 5. pair filter, segmentation
def test_scene_pairs_and_masks_have_both_outcomes():
    assert LC.SCENE_P > LC.SCENE_LANES_TOTAL and LC.SCENE_P < 2 * LC.SCENE_LANES_TOTAL and (LC.SCENE_P - LC.SCENE_LANES_TOTAL) % 256
    keep = LC.scene_distinct(None)
    assert 0.1 < keep.mean() < 0.9 and 0.1 < keep[LC.SCENE_LANES_TOTAL:].mean() < 0.9      # both outcomes, in the second trip too
    for bad, top in (("i32", LC.INT32_MAX), ("i64", LC.INT64_MAX)):
        idx, pos, side = LC.scene_pairs(bad)
        assert 900 <= len(pos) <= 1100 and idx.max() == top and idx.min() == -1 and (idx == LC.SCENE_N).any()
        assert (pos < LC.SCENE_LANES_TOTAL).sum() > 300 and ((pos >= LC.SCENE_LANES_TOTAL) & (pos < LC.SCENE_LANES_TOTAL + 256)).sum() > 100
        assert (pos >= LC.SCENE_LANES_TOTAL + 256).sum() == LC.SCENE_P - LC.SCENE_LANES_TOTAL - 256
        other = idx[pos, 1 - side]
        assert other.min() >= 0 and other.max() < LC.SCENE_N                                  # exactly one endpoint is bad
        k = LC.scene_distinct(bad)
        assert not k[pos].any() and np.array_equal(np.delete(k, pos), np.delete(keep, pos))
    assert (LC.scene_pairs("i64")[0] == 2 ** 32 + 7).any() and np.array_equal(LC.scene_pairs("i32")[1], LC.scene_pairs("i64")[1])
    # segmentation: survivors, point mask and kept pairs all have both values; a bad endpoint is not counted, the other one is
    idx, pos, side = LC.scene_pairs("i32")
    surv = LC.scene_survivors()
    assert 0.02 < surv.mean() < 0.05 and surv[pos].sum() >= 400
    pm, kept = Z.segment(idx, surv, LC.SCENE_N, LC.SCENE_MIN_CONTRIB)
    assert 0.2 < pm.mean() < 0.8 and 0.2 * surv.sum() < len(kept) < 0.95 * surv.sum()
    bad_surv = pos[surv[pos]]
    in_kept = np.isin(bad_surv, kept)
    assert in_kept.any() and not in_kept.all()
    assert np.array_equal(in_kept, pm[idx[bad_surv, 1 - side[surv[pos]]]])                    # decided by the good endpoint alone
    ends = np.concatenate([idx[surv, 0], idx[surv, 1]])
    want = np.bincount(ends[(ends >= 0) & (ends < LC.SCENE_N)], minlength=LC.SCENE_N)
    assert np.array_equal(pm, want > LC.SCENE_MIN_CONTRIB)
