"""Proposal masks -> instance clouds without a device: tests/instances_ref.py (the restatement scene_stage.voxel_owner and
csrc/instances.hip are held to) against plain Python loops on about 50 points, the face coordinates on which a reciprocal multiply
and the true division part, and the refusals of cppf_gather_instances that are decided on the host."""
import os

import numpy as np
import pytest

import instances_ref as R
from conftest import ROOT
from cppf_amd import _lib, scene_stage


def test_face_coordinates_separate_division_from_reciprocal_multiply():
    """float32(m q) for m = -4100..4100: both signs are there, and at q = 0.12 (4 res of the res = 0.03 configs) floor(p * (1 / q))
    puts 67 negative faces into the neighbouring voxel; at q = 0.016 the two agree everywhere (the input, not the mistake, decides)"""
    differ = {}
    for q in R.FACE_Q:
        p, m = R.face_cloud(q)
        assert (m < 0).sum() == (m > 0).sum() == 4100
        d, r = R.voxels(p, q)[:, 0], R.voxels_reciprocal(p, q)[:, 0]
        assert np.abs(d - m).max() <= 1                         # (the float32 nearest to a face lies on it or one step to a side)
        differ[q] = np.nonzero(d != r)[0]
        assert np.array_equal(R.voxels(p, q)[:, 1:], np.zeros((m.size, 2), np.int64))
    assert differ[0.12].size >= 50 and differ[0.016].size == 0
    p, m = R.face_cloud(0.12)
    at = differ[0.12]
    assert (R.voxels_reciprocal(p, 0.12)[at, 0] == R.voxels(p, 0.12)[at, 0] - 1).all() and (m[at] % 25 == 0).all()
    # and the owner map inherits it: with every point its own voxel's representative, the mistaken voxels own different points
    ind = np.arange(0, m.size, 2)
    good, wrong = R.owner_ref(p, ind, 0.12), R.owner_ref(p, ind, 0.12, voxel_fn=R.voxels_reciprocal)
    assert (good != wrong).sum() >= 25


def test_owner_restatement_equals_the_loop():
    p, q = R.small_face_cloud()
    assert 45 <= p.shape[0] <= 60
    v = R.voxels(p, q)
    assert (v[:, 0] != R.voxels_reciprocal(p, q)[:, 0]).any()                 # the small cloud holds separating faces too
    _, first = np.unique(v, axis=0, return_index=True)
    ind = np.sort(first)                                                      # sparse_quantize's choice: the lowest index per voxel
    own = R.owner_ref(p, ind, q)
    assert np.array_equal(own, R.owner_loop(p, ind, q)) and (own >= 0).all()
    assert np.array_equal(v[ind[own]], v) and np.array_equal(own[ind], np.arange(ind.size))
    assert np.bincount(own).max() >= 2                                        # several dense points in one voxel
    # a caller's own subset: voxels left out get -1, a voxel named twice belongs to the first position
    sub = np.concatenate([ind[::2], ind[:1]])
    own2 = R.owner_ref(p, sub, q)
    assert np.array_equal(own2, R.owner_loop(p, sub, q)) and (own2 == -1).any() and own2[ind[0]] == 0
    assert np.array_equal(R.owner_ref(p, np.zeros(0, np.int64), q), np.full(p.shape[0], -1))


@pytest.mark.parametrize("K", [1, 3, 7])
def test_gather_restatement_equals_the_loop(K):
    hi, nrm, owner, masks = R.case(53, K, N=20, seed=K, lone=5)
    member, offsets, pts, nr, src = R.gather_loop(hi, nrm, owner, masks)
    T = int(offsets[-1])
    g = R.gather_ref(hi, nrm, owner, masks, capacity=T + 3)
    assert not g["bad"] and np.array_equal(g["member"], member) and np.array_equal(g["offsets"], offsets)
    assert np.array_equal(g["pts"][:T], pts) and np.array_equal(g["nrm"][:T], nr) and np.array_equal(g["src"][:T], src)
    assert (g["src"][T:] == R.POISON_I).all() and (owner == -1).sum() == 5
    for k in range(K):                                                        # hi[member_k], in increasing dense index
        rows = np.nonzero((member >> np.uint32(k)) & 1)[0]
        assert np.array_equal(src[offsets[k]:offsets[k + 1]], rows) and np.array_equal(pts[offsets[k]:offsets[k + 1]], hi[rows])
    if K >= 3:
        assert offsets[1] == 0 and offsets[K] - offsets[K - 1] == (owner >= 0).sum() and (member & 6 == 6).any()
    # one row short: complete offsets, the last row dropped, nothing else moved
    s = R.gather_ref(hi, nrm, owner, masks, capacity=T - 1)
    assert np.array_equal(s["offsets"], offsets) and np.array_equal(s["src"], src[:T - 1]) and np.array_equal(s["pts"], pts[:T - 1])
    bad = owner.copy()
    bad[7] = 20
    b = R.gather_ref(hi, nrm, bad, masks)
    assert b["bad"] and b["offsets"].tolist() == [0] * K + [-1] and (b["src"] == R.POISON_I).all() and (b["pts"] == R.POISON_F).all()


def test_refusals_that_need_no_device():
    """the host's checks of cppf_gather_instances return before anything is launched; scene_stage.check_gather_args mirrors them"""
    L = _lib.lib()
    buf = np.zeros(64, np.int32)                                              # (never followed: every call below is refused)
    ptr = buf.ctypes.data
    call = lambda K, N, M, cap: L.cppf_gather_instances(ptr, ptr, ptr, ptr, K, N, M, cap, ptr, ptr, ptr, ptr, ptr, ptr, None)
    EINVAL = -1
    for K, N, M, cap in [(0, 4, 4, 4), (33, 4, 4, 4), (-1, 4, 4, 4), (2, -1, 4, 4), (2, 4, -1, 4), (2, 4, 4, -1), (1, 4, 2 ** 31, 4),
                         (32, 4, 2 ** 26, 4), (2, 2 ** 31, 4, 4)]:
        assert call(K, N, M, cap) == EINVAL, (K, N, M, cap)
        with pytest.raises(ValueError):
            scene_stage.check_gather_args(K, N, M, cap)
    assert call(1, 4, scene_stage.GATHER_CHUNK * scene_stage.GATHER_MAX_CHUNKS + 1, 4) == _lib.EUNSUPPORTED
    with pytest.raises(ValueError, match="at most"):
        scene_stage.check_gather_args(1, 4, scene_stage.GATHER_CHUNK * scene_stage.GATHER_MAX_CHUNKS + 1, 4)
    assert L.cppf_gather_instances(ptr, ptr, ptr, ptr, 2, 4, 4, 4, ptr, None, ptr, ptr, ptr, ptr, None) == EINVAL       # offsets NULL
    assert L.cppf_gather_instances(ptr, ptr, ptr, ptr, 2, 4, 4, 4, ptr, ptr, None, ptr, ptr, ptr, None) == EINVAL       # pts NULL, capacity > 0
    assert L.cppf_gather_instances(ptr, ptr, None, ptr, 2, 4, 4, 4, ptr, ptr, ptr, ptr, ptr, ptr, None) == EINVAL       # owner NULL, points
    scene_stage.check_gather_args(32, 300, scene_stage.GATHER_CHUNK * scene_stage.GATHER_MAX_CHUNKS, 0)
    hdr = open(os.path.join(ROOT, "include", "cppf.h")).read()
    assert f"#define CPPF_GATHER_CHUNK {scene_stage.GATHER_CHUNK}\n" in hdr and f"#define CPPF_GATHER_MAX_CHUNKS {scene_stage.GATHER_MAX_CHUNKS}\n" in hdr
