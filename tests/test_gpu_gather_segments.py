"""cppf_gather_segments (csrc/instances.hip) on the device against tests/gather_segments_ref.py, bit for bit: offsets, pts, nrm, src,
bounds and the intermediate chunk_counts, at the wave edge (63 / 64 / 65 points), the chunk edge (1023 / 1024 / 1025), in the second
and fourth chunk, for 1 / 7 / 32 / 33 / 1023 / 1024 segments and five label patterns (one label; every lane its own; runs that straddle
wave and chunk edges; labels in no segment mixed in; empty segments at the first, middle and last slot), into poisoned buffers with a
canary behind `capacity`; one row short of room; a count-only call with NULL outputs; bounds NULL; twice with identical words; against
cppf_gather_instances with one-hot masks; the refusals; segments.segment_clouds on a SceneCloud."""
import numpy as np
import pytest
import torch

import gather_segments_ref as R
from cppf_amd import _lib, scene_stage, segments
from cppf_amd._torch_util import call

pytestmark = pytest.mark.gpu
CHUNK = scene_stage.GATHER_CHUNK
GUARD = 8                                                                     # canary rows behind every buffer
MS = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 7]
SS = [1, 7, 32, 33, 1023, 1024]
EINVAL = -1


def _d(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, hi, nrm, lab, S, cap, bounds=True, null_rows=False):
    """one call into poisoned buffers, GUARD entries longer than what the call may write -> numpy, chunk_counts included"""
    d = _d(dev)
    M = hi.shape[0]
    f = lambda n, w: torch.full((n + GUARD, w), float(R.POISON_F), dtype=torch.float32, device=dev)
    i = lambda n: torch.full((n + GUARD,), int(R.POISON_I), dtype=torch.int32, device=dev)
    n_cc = S * ((M + CHUNK - 1) // CHUNK)
    out = dict(offsets=i(S + 1), pts=f(cap, 3), nrm=f(cap, 3), src=i(cap), bounds=f(S, 6), chunk_counts=i(n_cc))
    rows = (None, None, None) if null_rows else (out["pts"], out["nrm"], out["src"])
    call("cppf_gather_segments", dev, d(hi), d(nrm), d(lab), S, M, cap, out["offsets"], *rows, out["bounds"] if bounds else None,
         out["chunk_counts"])
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_equal(got, want, S, cap, tag, bounds=True):
    assert np.array_equal(got["offsets"][:S + 1], want["offsets"]), (tag, got["offsets"][:S + 1], want["offsets"])
    for key in ("pts", "nrm"):
        assert np.array_equal(R.bits(got[key][:cap]), R.bits(want[key])), (tag, key)      # rows the call leaves alone: still poison
        assert (got[key][cap:] == R.POISON_F).all(), (tag, key, "canary")
    assert np.array_equal(got["src"][:cap], want["src"]) and (got["src"][cap:] == R.POISON_I).all(), (tag, "src")
    assert (got["offsets"][S + 1:] == R.POISON_I).all(), (tag, "offsets canary")
    if bounds:
        assert np.array_equal(R.bits(got["bounds"][:S]), R.bits(want["bounds"])), (tag, "bounds")
    else:
        assert (got["bounds"][:S] == R.POISON_F).all(), (tag, "bounds untouched")
    assert (got["bounds"][S:] == R.POISON_F).all(), (tag, "bounds canary")
    cc = want["chunk_counts"].reshape(-1)
    assert np.array_equal(got["chunk_counts"][:cc.size], cc) and (got["chunk_counts"][cc.size:] == R.POISON_I).all(), (tag, "chunk_counts")


@pytest.fixture(scope="module")
def cases():
    """every (M, S, pattern): the cloud, the labels and the restatement at roomy capacity, computed once"""
    out = {}
    for M in MS:
        for S in SS:
            hi, nrm = R.cloud(M, seed=M + S)
            for pattern in R.PATTERNS:
                lab = R.labels_case(pattern, M, S, seed=M + S)
                out[M, S, pattern] = (hi, nrm, lab, R.gather_segments_ref(hi, nrm, lab, S, capacity=M + 5))
    return out


@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("M", MS)
def test_gather_equals_the_restatement(dev, cases, M, S):
    for pattern in R.PATTERNS:
        hi, nrm, lab, want = cases[M, S, pattern]
        total = int(want["offsets"][S])
        assert total == R.in_range(lab, S).sum() and (pattern != "one" or total == M)
        tag = (M, S, pattern)
        # roomy; exactly the total; the default of the wrapper (M rows)
        roomy = _run(dev, hi, nrm, lab, S, M + 5)
        _assert_equal(roomy, want, S, M + 5, tag + ("roomy",))
        _assert_equal(_run(dev, hi, nrm, lab, S, total), R.gather_segments_ref(hi, nrm, lab, S, capacity=total), S, total, tag + ("total",))
        # twice: identical words, chunk_counts included
        again = _run(dev, hi, nrm, lab, S, M + 5)
        for key in roomy:
            assert np.array_equal(roomy[key].view(np.uint32), again[key].view(np.uint32)), tag + (key, "second run")
        if total >= 1:
            # one row short: complete offsets, nothing at or beyond capacity
            short = _run(dev, hi, nrm, lab, S, total - 1)
            _assert_equal(short, R.gather_segments_ref(hi, nrm, lab, S, capacity=total - 1), S, total - 1, tag + ("short",))
            assert int(short["offsets"][S]) == total
        # count only: capacity 0 and NULL rows; and bounds NULL
        none = _run(dev, hi, nrm, lab, S, 0, null_rows=True)
        _assert_equal(none, R.gather_segments_ref(hi, nrm, lab, S, capacity=0), S, 0, tag + ("count only",))
        nb = _run(dev, hi, nrm, lab, S, M + 5, bounds=False)
        _assert_equal(nb, want, S, M + 5, tag + ("bounds NULL",), bounds=False)


def test_the_cases_reach_what_they_are_for(cases):
    """empty segments at the first, middle and last slot; a wave with 64 distinct labels; labels in no segment; bounds with -0.0 as a
    minimum beside +0.0 as a maximum, and a segment whose points are all left out"""
    hi, nrm, lab, want = cases[3 * 1024 + 7, 33, "empty"]
    n = np.diff(want["offsets"])
    assert n[0] == n[16] == n[32] == 0 and (n > 0).sum() == 30
    assert np.array_equal(R.bits(want["bounds"][[0, 16, 32]]), R.bits(np.tile(R.EMPTY_BOUNDS, (3, 1))))
    assert np.unique(cases[1025, 1024, "lanes"][2][:64]).size == 64
    mixed = cases[3 * 1024 + 7, 7, "mixed"]
    assert {-1, 7, R.INT32_MAX, R.INT32_MIN}.issubset(set(mixed[2].tolist()))
    b = R.bits(cases[3 * 1024 + 7, 1024, "mixed"][3]["bounds"])               # two points a segment: a zero is often an extreme
    assert (b[:, :3] == 0x80000000).any() and (b[:, 3:] == 0).any() and (b[:, :3] == 0).any() and (b[:, 3:] == 0x80000000).any()
    both = (b[:, :3] == 0x80000000) & (b[:, 3:] == 0)
    assert both.any()                                                         # min -0.0 beside max +0.0: the order of the zeros decides
    hi1, _, lab1, want1 = cases[1, 1, "one"]
    assert want1["offsets"].tolist() == [0, 1]


def test_zero_order_and_points_that_are_not_finite(dev):
    """the small case of tests/test_gather_segments_cpu.py on the device, and a segment whose -0.0 and +0.0 meet across workgroups"""
    z, nz, nan, inf = np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(np.inf)
    hi = np.array([[z, nz, 1.0], [nz, z, 2.0], [nan, 5.0, 5.0], [-9.0, inf, 0.0], [1.0, 1.0, -inf], [nz, nz, nz], [3.0, -4.0, 5.0]], np.float32)
    lab = np.array([0, 0, 0, 0, 1, 2, 7], np.int32)
    got = _run(dev, hi, np.zeros_like(hi), lab, 4, 7)
    want = np.array([[nz, nz, 1.0, z, z, 2.0], R.EMPTY_BOUNDS, [nz] * 6, R.EMPTY_BOUNDS], np.float32)
    assert np.array_equal(R.bits(got["bounds"][:4]), R.bits(want))
    M = 2 * CHUNK + 1
    hi = np.zeros((M, 3), np.float32)
    hi[0], hi[CHUNK + 3], hi[2 * CHUNK] = [nz, 1.0, -1.0], [z, -2.0, -3.0], [nz, nz, z]
    hi[5:9] = nan
    lab = np.full(M, -1, np.int32)
    lab[[0, CHUNK + 3, 2 * CHUNK]] = 2
    lab[5:9] = 1
    got = _run(dev, hi, np.zeros_like(hi), lab, 3, M)
    want = R.gather_segments_ref(hi, np.zeros_like(hi), lab, 3, capacity=M)
    _assert_equal(got, want, 3, M, "zeros across workgroups")
    assert np.array_equal(R.bits(got["bounds"][2]), R.bits(np.array([nz, -2.0, -3.0, z, 1.0, z], np.float32)))
    assert np.array_equal(R.bits(got["bounds"][1]), R.bits(R.EMPTY_BOUNDS))


@pytest.mark.parametrize("S", [1, 7, 32])
@pytest.mark.parametrize("M", [65, 3 * 1024 + 7])
def test_gather_equals_gather_instances_with_one_hot_masks(dev, M, S):
    """labels in [-1, S), S <= 32: offsets, pts, nrm, src equal cppf_gather_instances with owner = labels and one-hot masks"""
    d = _d(dev)
    hi, nrm = R.cloud(M, seed=3 * M + S)
    for pattern in ("lanes", "runs", "mixed"):
        lab = R.labels_case(pattern, M, S, seed=M + S)
        lab[~R.in_range(lab, S)] = -1
        old = scene_stage.gather_instances_device(d(hi), d(nrm), d(lab), torch.eye(S, dtype=torch.uint8, device=dev), capacity=M)
        got = _run(dev, hi, nrm, lab, S, M)
        T = int(got["offsets"][S])
        assert np.array_equal(got["offsets"][:S + 1], old["offsets"].cpu().numpy()) and T == (lab >= 0).sum()
        for key in ("pts", "nrm"):
            assert np.array_equal(R.bits(got[key][:T]), R.bits(old[key].cpu().numpy()[:T])), (pattern, key)
        assert np.array_equal(got["src"][:T], old["src"].cpu().numpy()[:T]), pattern


def test_refusals_launch_nothing(dev):
    hi, nrm = R.cloud(40, seed=1)
    lab = R.labels_case("mixed", 40, 2, seed=1)
    d = _d(dev)
    f = lambda n, w: torch.full((n, w), float(R.POISON_F), dtype=torch.float32, device=dev)
    i = lambda n: torch.full((n,), int(R.POISON_I), dtype=torch.int32, device=dev)
    out = dict(offsets=i(1026), pts=f(40, 3), nrm=f(40, 3), src=i(40), bounds=f(1025, 6), counts=i(1025))
    base = [d(hi), d(nrm), d(lab), 2, 40, 40, out["offsets"], out["pts"], out["nrm"], out["src"], out["bounds"], out["counts"]]

    def refused(code=EINVAL, **change):
        a = list(base)
        for j, v in change.items():
            a[int(j[1:])] = v
        assert call("cppf_gather_segments", dev, *a, ok=(code,)) == code, change
    for S in (0, 1025, -1):
        refused(_3=S)
    refused(_4=-1)                                                            # n_dense < 0
    refused(_5=-1)                                                            # capacity < 0
    refused(_4=2 ** 31)                                                       # n_dense > 2^31 - 1
    refused(_6=None)                                                          # offsets NULL
    for j in (7, 8, 9):
        refused(**{f"_{j}": None})                                            # pts / nrm / src NULL with capacity > 0
    for j in (0, 1, 2, 11):
        refused(**{f"_{j}": None})                                            # an input or chunk_counts NULL with points
    refused(code=_lib.EUNSUPPORTED, _4=CHUNK * scene_stage.GATHER_MAX_CHUNKS + 1)
    with pytest.raises(_lib.CppfError, match=r"cppf_gather_segments failed \(-1\)"):
        call("cppf_gather_segments", dev, *(base[:3] + [1025] + base[4:]))
    torch.cuda.synchronize(dev)
    for k, v in out.items():                                                  # nothing was launched
        assert (v == (float(R.POISON_F) if v.dtype == torch.float32 else int(R.POISON_I))).all(), k


def test_an_empty_cloud_writes_zero_offsets_and_empty_bounds(dev):
    for S in (1, 7, 1024):
        offsets = torch.full((S + 1 + GUARD,), int(R.POISON_I), dtype=torch.int32, device=dev)
        bounds = torch.full((S + GUARD, 6), float(R.POISON_F), dtype=torch.float32, device=dev)
        call("cppf_gather_segments", dev, None, None, None, S, 0, 0, offsets, None, None, None, bounds, None)   # every input NULL
        torch.cuda.synchronize(dev)
        o, b = offsets.cpu().numpy(), bounds.cpu().numpy()
        assert not o[:S + 1].any() and (o[S + 1:] == R.POISON_I).all()
        assert np.array_equal(R.bits(b[:S]), R.bits(np.tile(R.EMPTY_BOUNDS, (S, 1)))) and (b[S:] == R.POISON_F).all()
        call("cppf_gather_segments", dev, None, None, None, S, 0, 0, offsets, None, None, None, None, None)     # and bounds NULL


def test_segment_clouds_on_a_scene_cloud(dev):
    """the wrappers: one call, views that equal hi[hi_labels == s] by torch, bounds; a cloud without labels is refused"""
    d = _d(dev)
    M, S = 2 * CHUNK + 333, 9
    hi, nrm = R.cloud(M, seed=2, specials=False)
    lab = R.labels_case("mixed", M, S, seed=2)
    lab[lab == 4] = -1                                                        # an empty segment in the middle
    cloud = scene_stage.SceneCloud(hi=d(hi), hi_nrm=d(nrm), hi_labels=d(lab), ind=torch.arange(4, device=dev), pc=d(hi[:4]),
                                   nrm=d(nrm[:4]), labels=d(lab[:4]))
    want = R.gather_segments_ref(hi, nrm, lab, S)
    g = segments.segment_clouds(cloud, S)
    assert g["offsets"].dtype == np.int64 and np.array_equal(g["offsets"], want["offsets"]) and len(g["clouds"]) == S
    T = int(want["offsets"][S])
    assert g["pts"].shape == (T, 3) and np.array_equal(g["src"].cpu().numpy(), want["src"][:T])
    for s, (p, n) in enumerate(g["clouds"]):
        sel = cloud.hi_labels == s
        assert torch.equal(p, cloud.hi[sel]) and torch.equal(n, cloud.hi_nrm[sel])
    assert g["clouds"][4][0].shape == (0, 3)
    assert np.array_equal(R.bits(g["bounds"].cpu().numpy()), R.bits(want["bounds"]))
    dv = segments.segment_clouds_device(cloud, S, capacity=10)               # the caller's capacity: rows cut there
    assert dv["pts"].shape == (10, 3) and np.array_equal(dv["src"].cpu().numpy(), want["src"][:10])
    assert np.array_equal(dv["offsets"].cpu().numpy(), want["offsets"])
    e = segments.segment_clouds(cloud, 0)
    assert e["clouds"] == [] and e["offsets"].tolist() == [0]
    with pytest.raises(ValueError, match="labels"):
        segments.segment_clouds(cloud._replace(hi_labels=None), S)
    with pytest.raises(ValueError, match="1..1024"):
        segments.segment_clouds(cloud, 1025)
