"""csrc/instances.hip, csrc/segments.hip and csrc/scene_train.hip at their caps, on the second trips of their loops and on lists
that break their promises (cases: tests/scene_limits_cases.py; that each case reaches its trip or branch:
tests/test_scene_limits_cpu.py).  cppf_gather_instances with more than 64 chunks and more than 16 proposals, at 8192 chunks, and
refusing an owner seen only by the far workgroups; cppf_depth_segments with 1023 / 1024 / 1025 and 256 / 257 listed segments and
the link rule at depth, tolerance and slope 65535 / 65535 / 1000; cppf_plane_ransac beyond one trip of its capped launch;
cppf_sample_scene_pairs on each list its four guards exist for; cppf_scene_pair_targets at 2 and 256 bins and on a scene whose
answer is exact.

Every expected value is a numpy restatement (instances_ref, segments_ref, scene_training_ref) -- never the kernel under test."""
import dataclasses
import time

import numpy as np
import pytest
import torch

import instances_ref as IR
import scene_limits_cases as C
import scene_training_ref as TR
from cppf_amd import scene_training as ST
from cppf_amd._torch_util import call
from cppf_amd.config import CATEGORIES
from test_gpu_instances import _assert_equal, _run as _gather
from test_gpu_scene_training import _check_against, _device_targets, _np, scene3_case
from test_gpu_segments import _check, _plane_check

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ A. instance gather
@pytest.mark.parametrize("M", C.EDGE_MS)
def test_gather_at_lane_and_chunk_edges(dev, M):
    K = 7
    hi, nrm, owner, masks = IR.case(M, K, N=301, seed=M)
    total = int(IR.gather_ref(hi, nrm, owner, masks, capacity=0)["offsets"][K])
    assert total >= 2
    for cap in (total + 5, total - 1):
        _assert_equal(_gather(dev, hi, nrm, owner, masks, cap), IR.gather_ref(hi, nrm, owner, masks, capacity=cap), K, M, cap, cap - total)


@pytest.mark.parametrize("K", C.FAR_KS)
@pytest.mark.parametrize("M", C.FAR_MS)
def test_gather_on_the_second_trip_of_the_table_sum(dev, M, K):
    """more than 64 chunks: gi_scatter_kernel's `c += 64` makes a second trip and the workgroups >= 64 place their rows behind a sum
    over both trips; K = 16 / 17 / 32: one trip of `k += GI_WAVES`, a ragged second one, two full ones.  Roomy and one row short."""
    hi, nrm, owner, masks = C.gather_far_case(M, K)
    roomy, total = C.gather_far_ref(M, K)
    _assert_equal(_gather(dev, hi, nrm, owner, masks, total + 5), roomy, K, M, total + 5, "roomy")
    short = _gather(dev, hi, nrm, owner, masks, total - 1)
    _assert_equal(short, IR.gather_ref(hi, nrm, owner, masks, capacity=total - 1), K, M, total - 1, "short")
    assert int(short["offsets"][K]) == total


@pytest.mark.parametrize("M,where", [(C.FAR_MS[1], C.FAR_START), (C.FAR_MS[2], C.FAR_START + 5), (C.FAR_MS[2], C.FAR_MS[2] - 1)],
                         ids=["65_chunks_chunk_64", "66_chunks_chunk_64", "66_chunks_last_chunk"])
def test_gather_refuses_an_owner_seen_from_the_far_side(dev, M, where):
    """the offending chunk's -1 stands in a column >= 64 of the table: workgroup 0, which writes offsets, meets it on its second trip"""
    K = 17
    hi, nrm, owner, masks = C.gather_far_case(M, K)
    owner = owner.copy()
    owner[where] = C.N_SPARSE
    total = C.gather_far_ref(M, K)[1]
    got = _gather(dev, hi, nrm, owner, masks, total)
    assert got["offsets"][:K + 1].tolist() == [0] * K + [-1]
    for key in ("pts", "nrm"):
        assert (got[key] == IR.POISON_F).all(), key                               # nothing copied, by any workgroup
    assert (got["src"] == IR.POISON_I).all() and (got["member"][M:] == IR.POISON_I).all() and (got["offsets"][K + 1:] == IR.POISON_I).all()


def test_gather_at_8192_chunks(dev):
    """CPPF_GATHER_MAX_CHUNKS chunks, 8 388 608 points, one mask of a few sparse points: accepted, equal to the restatement.  (One
    chunk more is refused: tests/test_scene_limits_cpu.py.)  The call's time on the device is printed."""
    from cppf_amd import scene_stage
    hi, nrm, owner, masks = C.gather_cap_case()
    M, cap = hi.shape[0], 64
    want = IR.gather_ref(hi, nrm, owner, masks, capacity=cap)
    d = lambda a: torch.from_numpy(a).to(dev)
    args = d(hi), d(nrm), d(owner), d(masks)
    G = 8
    out = dict(member=torch.full((M + G,), int(IR.POISON_I), dtype=torch.int32, device=dev),
               offsets=torch.full((2 + G,), int(IR.POISON_I), dtype=torch.int32, device=dev),
               pts=torch.full((cap + G, 3), float(IR.POISON_F), dtype=torch.float32, device=dev),
               nrm=torch.full((cap + G, 3), float(IR.POISON_F), dtype=torch.float32, device=dev),
               src=torch.full((cap + G,), int(IR.POISON_I), dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    scene_stage.gather_instances_device(*args, capacity=cap, out=out)
    torch.cuda.synchronize(dev)
    print(f"cppf_gather_instances on {M} points, 8192 chunks: {1e3 * (time.perf_counter() - t0):.2f} ms")
    _assert_equal({k: v.cpu().numpy() for k, v in out.items()}, want, 1, M, cap, "8192 chunks")


# ------------------------------------------------------------------------------------------------ B. depth segments
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_segments_around_the_cap(dev, n):
    """1024 one-pixel components at capacity 1024: every thread of seg_rank_kernel is live and `first` has no tail; 1023: one tail
    entry; 1025: overflow at the largest capacity -- nothing listed, every live pixel labelled -1"""
    w = _check(dev, C.cap_image(n), min_pixels=1, capacity=C.SEG_MAX)
    assert w["counts"].tolist() == [n, n, n, 0] and w["overflow"] == (n == 1025)
    if n == 1025:                                                                 # on overflow _check leaves these three out: by hand
        d = C.cap_image(n)
        from test_gpu_segments import _run
        got = _run(dev, d, min_pixels=1, capacity=C.SEG_MAX)
        assert (got["labels"] == -1).all() and (got["first"] == -1).all() and not got["sizes"].any()


@pytest.mark.parametrize("n_kept", [256, 257])
def test_segments_staged_in_one_and_two_trips(dev, n_kept):
    """256 / 257 kept segments among over 500 components whose kept and dropped roots interleave: seg_label_kernel's staging loop
    makes exactly one trip / a second trip for one entry, and a rank is neither a ticket nor the root's ordinal among all roots"""
    d = C.staging_image(n_kept)
    for cap in (C.SEG_MAX, n_kept, n_kept - 1):
        w = _check(dev, d, capacity=cap, **C.STAGING_FILTER)
        assert w["counts"][0] == n_kept and w["overflow"] == (cap < n_kept)


def test_link_rule_at_the_ends_of_its_ranges(dev):
    for row, tol, slope, comps in C.LINK_ENDS:
        w = _check(dev, np.array([row], np.uint16), tol_mm=tol, slope_permille=slope)
        assert w["counts"][1] == comps, (row, tol, slope)


def test_one_long_row(dev):
    """65 537 flat pixels in one row: 1025 waves, each joined to the one before by its lane 0; one component, root 0"""
    w = _check(dev, np.full((1, C.LONG_ROW), 1000, np.uint16))
    assert w["counts"].tolist() == [1, 1, C.LONG_ROW, 0] and w["first"][0] == 0 and w["sizes"][0] == C.LONG_ROW


# ------------------------------------------------------------------------------------------------ C. plane RANSAC
@pytest.mark.parametrize("N", C.PLANE_NS)
def test_plane_counts_beyond_one_trip(dev, N):
    """131 072 points fill one trip of pr_count_kernel's 512 x 256 lanes; one point more, 65 more (a full wave and a wave of one
    point in the second trip) and 262 145 (a third trip of one point).  The last 65 points hold inliers of the best plane."""
    planes, counts, best = _plane_check(dev, C.plane_case(N), C.PLANE_HYP, C.PLANE_THRESH, seed=N)
    assert best[0] >= 0 and best[1] > 0.5 * N


# ------------------------------------------------------------------------------------------------ D. the draw
def _draw(dev, name, P=C.DRAW_P, n_pos=None):
    """cppf_sample_scene_pairs on draw_case(name): every array is a view into a larger device allocation of in-range junk"""
    c = C.draw_case(name)
    mb, sb, ib = (torch.from_numpy(c[k]).to(dev) for k in ("members_buf", "seg_buf", "inst_buf"))
    m, s, i = mb[C.M_OFF:C.M_OFF + c["M"]], sb[C.S_OFF:C.S_OFF + C.DRAW_K + 1], ib[C.I_OFF:C.I_OFF + C.DRAW_N]
    idx = torch.full((P + 4, 2), -9, dtype=torch.int32, device=dev)
    call("cppf_sample_scene_pairs", dev, m, c["cap"], s, C.DRAW_K, i, C.DRAW_N, P, P if n_pos is None else n_pos, C.DRAW_SEED, idx)
    torch.cuda.synchronize(dev)
    got = idx.cpu().numpy()
    assert (got[P:] == -9).all()
    return got[:P]


@pytest.mark.parametrize("name", C.DRAW_BREAKS)
def test_draw_on_a_list_that_breaks_a_promise(dev, name):
    """one test per guard of st_draw_kernel: the pairs whose lookup fails keep the uniform draw, the others draw from the lists"""
    want, kept = C.draw_want(name)
    got = _draw(dev, name)
    assert np.array_equal(got, want), (name, np.nonzero((got != want).any(-1))[0][:8])
    uniform = _draw(dev, name, n_pos=0)
    assert np.array_equal(got[kept], uniform[kept]) and kept.any() and (name == "cap" or (~kept).any())
    good = _draw(dev, None)
    assert np.array_equal(good, C.draw_want(None)[0]) and np.array_equal(got[~kept, 0], good[~kept, 0])


@pytest.mark.parametrize("P", [0, 255, 256])
def test_draw_sizes_around_a_workgroup(dev, P):
    c = C.draw_case(None)
    m, s, i = C.draw_views(c)
    got = ST.sample_scene_pairs(m[:c["M"]].copy(), s.copy(), torch.from_numpy(i.copy()).to(dev), P, P, C.DRAW_SEED)
    assert tuple(got.shape) == (P, 2) and np.array_equal(got.cpu().numpy(), TR.draw_ref(m[:c["M"]], s, i, C.DRAW_N, P, P, C.DRAW_SEED))
    if P:
        assert np.array_equal(_draw(dev, None, P), got.cpu().numpy())


def test_draw_on_a_cloud_of_one_point(dev):
    inst = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ST.sample_scene_pairs(np.zeros(1, np.int32), np.array([0, 1], np.int32), inst, 300, 150, 3).cpu().numpy()
    assert got.shape == (300, 2) and not got.any()
    got = ST.sample_scene_pairs(np.zeros(0, np.int32), np.array([0, 0], np.int32), inst, 300, 150, 3).cpu().numpy()      # and no member
    assert got.shape == (300, 2) and not got.any()


# ------------------------------------------------------------------------------------------------ D. the targets
@pytest.mark.parametrize("tr_bins,rot_bins", [(2, 2), (256, 256), (2, 256), (256, 2)])
def test_targets_at_2_and_256_bins(dev, tr_bins, rot_bins):
    """the ends of the accepted range, where a bin index is one byte: test_gpu_scene_training.py's scene, pairs and rule (within 4 x
    what torch fp32 deviates from the fp64 restatement AT THESE BINS)"""
    s = scene3_case(tr_num_bins=tr_bins, rot_num_bins=rot_bins)
    t = _np(_device_targets(s, dev, s["idx"]))
    easy = ~s["hard"]                                                             # (a value on a bin edge may fall either way: one bin)
    assert t["low"].dtype == np.uint8 and np.abs(t["low"][easy].astype(np.int64) - s["t64"]["low"][easy]).max() <= 1
    _check_against(s, t, s["t64"], s["tr64"], s["rot64"], s["hard"], f"bins {tr_bins} / {rot_bins}")


@pytest.mark.parametrize("tr_bins,rot_bins", C.EXACT_BINS)
def test_targets_on_the_exact_scene(dev, tr_bins, rot_bins):
    """values below, on and above the clamp ends, u = +-up and +-right with and without the symmetry bits, a coincident pair, NaN and
    inf coordinates: every quantity is exact in fp32, the kernel's words equal the fp32 restatement's bit for bit"""
    s = C.exact_scene()
    cfg = dataclasses.replace(CATEGORIES["bottle"], vote_range=list(C.EXACT_RANGE), tr_num_bins=tr_bins, rot_num_bins=rot_bins)
    want = C.exact_want(tr_bins, rot_bins)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = _np(ST.scene_pair_targets(d(s["pc"]), d(s["nrm"]), d(s["inst"]), d(s["idx"]), s["table"], s["flags"], cfg))
    for p, (name, k) in enumerate(s["names"]):
        got = (int(t["kind"][p]), int(t["pair_inst"][p]), t["low"][p].tolist(), t["w_low"][p].tolist(), t["aux"][p].tolist())
        exp = (int(want["kind"][p]), int(want["pair_inst"][p]), want["low"][p].tolist(), want["w_low"][p].tolist(), want["aux"][p].tolist())
        assert got == exp, (name, k, got, exp)
    assert np.array_equal(t["w_low"].view(np.uint32), want["w_low"].astype(np.float32).view(np.uint32))
    assert (want["kind"] == 1).sum() == 2 * len(C.EXACT_BY_HAND) and (want["kind"] == 0).sum() == len(s["names"]) - 2 * len(C.EXACT_BY_HAND)
