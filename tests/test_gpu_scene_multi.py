"""The two kernels of csrc/scene_multi.hip, bit for bit: cppf_backvote_multi against the oracle's back-vote and cppf_backvote_ws at every
centre, cppf_segment_instances against K calls of cppf_segment_instance and tests/zero_shot_ref.py:segment -- at the lane, wave-trip
(4 x 64 pairs) and workgroup-trip (4 x 256) edges, 1..32 centres, with (i, i) pairs, coincident points, pairs without rotations, a centre
outside the grid, identical centres and centres within tol of each other; the refusals; overflow of the kept-pair buffer; graph replay."""
import os
import sys

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
from cppf_amd import _lib, scene_poses, scene_stage
from cppf_amd._torch_util import stream_ptr
from cppf_amd.config import CATEGORIES
from cppf_amd.inference import grid_shape

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zero_shot_ref as Z  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = CATEGORIES["bowl"]
RES = CFG.res
P_MAX, K_MAX = 4099, 32
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099]
KS = [1, 2, 5, 32]
EINVAL, EWORKSPACE = -1, -2


def _cloud():
    """512 points of three posed bowls placed apart; points 0 and 1 coincide"""
    pcs, nrms, centers = [], [], []
    for k, n in enumerate((171, 171, 170)):
        ob = syn.make_posed_object("bowl", n, 40 + k)
        c = np.array([0.35 * k - 0.35, 0.04 * k, 0.8 + 0.05 * k])
        pcs.append((ob["pc"] - ob["center"] + c).astype(np.float32))
        nrms.append(ob["normals"])
        centers.append(c)
    pc, nrm = np.concatenate(pcs), np.concatenate(nrms)
    pc[1] = pc[0]
    owner = np.repeat(np.arange(3), (171, 171, 170))
    return pc, nrm, owner, np.array(centers)


def _pairs(pc, owner, centers, n_pairs, seed):
    """a uniform pair list with the closed-form (mu, nu) for within-object pairs and random values elsewhere; the special pairs sit
    at both ends of a wave: (i, i), the coincident points 0 / 1, nu below res / 2 pi (no rotation)"""
    rng = np.random.default_rng(seed)
    N = pc.shape[0]
    idx = rng.integers(0, N, (n_pairs, 2)).astype(np.int32)
    if n_pairs >= 72:
        idx[0] = (10, 60)                                   # (a within-object pair: P = 1 has something to decide)
        idx[3] = idx[70] = (7, 7)
        idx[5], idx[64] = (0, 1), (1, 0)
    vr = CFG.vote_range
    out = np.empty((n_pairs, 2), np.float32)
    out[:, 0] = rng.uniform(-vr[0], vr[0], n_pairs)
    out[:, 1] = rng.uniform(0, vr[1], n_pairs)
    for k in range(3):
        w = (owner[idx[:, 0]] == k) & (owner[idx[:, 1]] == k)
        out[w] = syn.closed_form_outputs(pc, centers[k], idx[w], CFG, quantise=False)
    if n_pairs >= 72:
        out[[7, 65], 1] = np.float32(RES / (2 * np.pi) * 0.9)
        out[9, 1] = 0.0
    return idx, out


def _centers(pc, centers, corner, dims):
    """32 centres: the first object's, one within tol of it, the second's, the first's again, one outside the grid, the third's, then
    random positions inside the grid"""
    rng = np.random.default_rng(5)
    tol = 3 * RES
    c = [centers[0], centers[0] + [0.5 * tol, 0, 0], centers[1], centers[0], corner - 5 * RES, centers[2]]
    hi = corner + (np.array(dims) - 1) * RES
    c += list(rng.uniform(corner, hi, (K_MAX - len(c), 3)))
    return np.ascontiguousarray(np.array(c, np.float64).astype(np.float32))


class Case:
    def __init__(self, dev, oracle):
        self.dev = dev
        self.pc, self.nrm, self.owner, self.obj_centers = _cloud()
        corners, self.dims = grid_shape(self.pc, RES)
        self.corner = corners[0]
        self.idx, self.out = _pairs(self.pc, self.owner, self.obj_centers, P_MAX, 3)
        self.centers = _centers(self.pc, self.obj_centers, self.corner.astype(np.float64), self.dims)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.d_pc, self.d_idx, self.d_out, self.d_corner, self.d_centers = d(self.pc), d(self.idx), d(self.out), d(self.corner), d(self.centers)
        self.tol = float(np.float32(3 * RES))
        self.want = {}
        for n_rots in (72, 7):                 # computed once, for the longest list and every centre: a pair's bit depends on nothing else
            bits = np.zeros(P_MAX, np.uint32)
            for k in range(K_MAX):
                _, m = oracle.backvote(self.pc, self.out, self.idx, self.corner, RES, n_rots, self.dims, self.centers[k], np.float32(3 * RES))
                single = backvote_ws(dev, self.d_pc, self.d_out, self.d_idx, self.d_corner, self.dims, self.d_centers[k], n_rots, self.tol)
                assert np.array_equal(single, m), (n_rots, k)
                bits |= m.astype(np.uint32) << np.uint32(k)
            self.want[n_rots] = bits


def backvote_ws(dev, pc, out, idx, corner, dims, center, n_rots, tol):
    P = idx.shape[0]
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    L = _lib.lib()
    _lib.check(L.cppf_backvote_ws(pc.data_ptr(), out.data_ptr(), None, idx.data_ptr(), corner.data_ptr(), RES, P, n_rots, *dims, None,
                                  center.data_ptr(), tol, mask.data_ptr(), None, stream_ptr(dev)), "cppf_backvote_ws")
    return mask.cpu().numpy().astype(bool)


@pytest.fixture(scope="module")
def case(dev, oracle):
    return Case(dev, oracle)


def _multi(case, P, K, n_rots):
    bits = torch.full((P + 8,), -1, dtype=torch.int32, device=case.dev)            # (8 guard words behind the buffer)
    scene_poses.backvote_multi(case.d_pc, case.d_out[:P], case.d_idx[:P], case.d_corner, RES, case.dims, case.d_centers[:K], n_rots,
                               out=bits)
    got = bits.cpu().numpy().view(np.uint32)
    assert (got[P:] == 0xffffffff).all()
    return got[:P]


def test_fixture_exercises_the_edges(case):
    """the special pairs and centres do what they are there for"""
    w = case.want[72]
    assert w[0] & 1 and (w & 1).sum() > 100                                     # survivors at the first object's centre
    assert ((w & 1) & ((w >> 1) & 1)).sum() > 10                                # pairs that survive at two centres within tol
    assert np.array_equal(w & 1, (w >> 3) & 1)                                  # identical centres, identical bits
    assert ((w >> 4) & 1).sum() == 0                                            # the centre outside the grid keeps nothing
    assert (w[[5, 64]] == 0).all() and (w[[7, 9, 65]] == 0).all()               # coincident points; no rotation
    assert (case.want[7] != 0).sum() > 50 and not np.array_equal(case.want[7], w)


@pytest.mark.parametrize("n_rots", [72, 7])
@pytest.mark.parametrize("P", SIZES)
def test_backvote_multi_bits(case, P, n_rots):
    for K in KS:
        mask = np.uint32(0xffffffff if K == 32 else (1 << K) - 1)
        got = _multi(case, P, K, n_rots)
        assert np.array_equal(got, case.want[n_rots][:P] & mask), (P, K, n_rots)
    assert np.array_equal(_multi(case, P, 5, n_rots), _multi(case, P, 5, n_rots))     # the same words on every run


def test_backvote_multi_large_list(case, dev):
    """2 000 003 pairs: every workgroup takes further trips of its grid-stride loop"""
    P, K = 2_000_003, 3
    idx, out = _pairs(case.pc, case.owner, case.obj_centers, P, 9)
    d_idx, d_out = torch.from_numpy(idx).to(dev), torch.from_numpy(out).to(dev)
    centers = case.d_centers[[0, 2, 5]].contiguous()
    bits = scene_poses.backvote_multi(case.d_pc, d_out, d_idx, case.d_corner, RES, case.dims, centers, 72).cpu().numpy().view(np.uint32)
    for k in range(K):
        single = backvote_ws(dev, case.d_pc, d_out, d_idx, case.d_corner, case.dims, centers[k], 72, case.tol)
        assert single.sum() > 1000
        assert np.array_equal(((bits >> k) & 1).astype(bool), single), k
    assert (bits >> K == 0).all()


def _segment_single(dev, d_idx, surv, N, min_contrib):
    L = _lib.lib()
    P = d_idx.shape[0]
    pm = torch.empty(N, dtype=torch.uint8, device=dev)
    pairs = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(L.cppf_segment_instance_workspace_bytes(N, P), 256), dtype=torch.uint8, device=dev)
    ds = torch.from_numpy(surv.astype(np.uint8)).to(dev)
    _lib.check(L.cppf_segment_instance(d_idx.data_ptr(), ds.data_ptr(), P, N, min_contrib, pm.data_ptr(), pairs.data_ptr(), cnt.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream_ptr(dev)), "cppf_segment_instance")
    return pm.cpu().numpy().astype(bool), pairs[:int(cnt.item())].cpu().numpy()


def _segment_inputs(case, source, P):
    if source == "backvote":
        return case.want[72][:P].copy()
    rng = np.random.default_rng(P)                      # dense random bits: every proposal keeps pairs in every chunk
    return (rng.random((P, 32)) < 0.3).astype(np.uint32) @ (np.uint32(1) << np.arange(32, dtype=np.uint32))


@pytest.mark.parametrize("source", ["backvote", "random"])
@pytest.mark.parametrize("P", [1, 65, 1023, 1025, 4099])
def test_segment_instances(case, dev, source, P):
    N = case.pc.shape[0]
    bits = _segment_inputs(case, source, P).astype(np.uint32)
    d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
    d_idx = case.d_idx[:P].contiguous()
    for K in KS:
        for min_contrib in (12, 0):
            masks, pairs, offsets = scene_poses.segment_instances(d_idx, d_bits, N, K, min_contrib)
            masks, pairs, offsets = masks.cpu().numpy().astype(bool), pairs.cpu().numpy(), offsets.cpu().numpy()
            assert offsets[0] == 0 and offsets.shape == (K + 1,)
            for k in range(K):
                surv = ((bits >> np.uint32(k)) & 1).astype(bool)
                pm, pos = Z.segment(case.idx[:P], surv, N, min_contrib)
                lst = pairs[offsets[k]:offsets[k + 1]] if offsets[K] <= P else None
                assert np.array_equal(masks[k], pm), (K, k, min_contrib)
                assert offsets[k + 1] - offsets[k] == pos.size
                if K == 5 or k in (0, K - 1):           # the single-proposal kernel on the same bit (every k at K = 5)
                    pm1, pos1 = _segment_single(dev, d_idx, surv, N, min_contrib)
                    assert np.array_equal(pm1, pm) and np.array_equal(pos1, pos)
                if lst is not None:
                    assert np.array_equal(lst, pos), (K, k, min_contrib)
            if offsets[K] > P:                          # more kept items than pairs: the documented retry
                _, pairs2, off2 = scene_poses.segment_instances(d_idx, d_bits, N, K, min_contrib, capacity=int(offsets[K]))
                pairs2, off2 = pairs2.cpu().numpy(), off2.cpu().numpy()
                assert np.array_equal(off2, offsets)
                for k in range(K):
                    surv = ((bits >> np.uint32(k)) & 1).astype(bool)
                    assert np.array_equal(pairs2[off2[k]:off2[k + 1]], Z.segment(case.idx[:P], surv, N, min_contrib)[1])


def test_segment_proposals_groups(case, dev):
    """scene_stage.segment_proposals = K x (cppf_backvote_ws + cppf_segment_instance) -- every mask, list and count -- with one,
    exactly one, two and three groups of 32 centres.  The centres: the fixture's 32, then the first two objects' centres (positions
    32, 33), random positions inside the grid, and the third object's centre at position 64, so that the second and the third group
    hold real objects (asserted on the single route's results: a grouping error cannot hide behind empty output).  One case runs
    with capacity = 1, which makes every group that keeps more than one item take the retry."""
    N, K_ALL = case.pc.shape[0], 65
    rng = np.random.default_rng(6)
    lo = case.corner.astype(np.float64)
    rand = rng.uniform(lo, lo + (np.array(case.dims) - 1) * RES, (K_ALL - 35, 3))
    centers = np.concatenate([case.centers, case.obj_centers[:2], rand, case.obj_centers[2:]]).astype(np.float32)
    assert centers.shape == (K_ALL, 3)
    d_centers = torch.from_numpy(np.ascontiguousarray(centers)).to(dev)
    for P in (257, 4099):
        d_idx, d_out = case.d_idx[:P].contiguous(), case.d_out[:P].contiguous()
        surv = [backvote_ws(dev, case.d_pc, d_out, d_idx, case.d_corner, case.dims, d_centers[k], 72, case.tol) for k in range(K_ALL)]
        for min_contrib in (0, 12):
            want = [_segment_single(dev, d_idx, m, N, min_contrib) for m in surv]           # once per (P, min_contrib), for every K
            if P == P_MAX and min_contrib == 0:
                assert all(want[k][0].any() and want[k][1].size > 0 for k in (32, 33, 64))
            for K in (1, 32, 33, 65):
                for cap in ((None, 1) if (P, K, min_contrib) == (P_MAX, 65, 0) else (None,)):
                    masks, pairs, offsets, counts, bits = scene_stage.segment_proposals(
                        case.d_pc, d_out, d_idx, case.d_corner, RES, case.dims, centers[:K], 72, None, min_contrib, capacity=cap)
                    masks, pairs, counts = masks.cpu().numpy().astype(bool), pairs.cpu().numpy(), counts.cpu().numpy()
                    assert masks.shape == (K, N) and counts.shape == (K,) and offsets.shape == (K + 1,) and offsets[0] == 0
                    assert len(bits) == (K + 31) // 32
                    for k in range(K):
                        assert np.array_equal(masks[k], want[k][0]), (P, K, k, min_contrib, cap)
                        assert np.array_equal(pairs[offsets[k]:offsets[k + 1]], want[k][1]), (P, K, k, min_contrib, cap)
                        assert counts[k] == want[k][1].size == offsets[k + 1] - offsets[k]


def test_segment_instances_small_capacity(case, dev):
    """capacity below the total: the true offsets, nothing written at or beyond capacity, success after the retry"""
    L = _lib.lib()
    P, K, N = P_MAX, 5, case.pc.shape[0]
    bits = case.want[72].copy()
    d_bits = torch.from_numpy(bits.view(np.int32)).to(dev)
    total = sum(Z.segment(case.idx, ((bits >> np.uint32(k)) & 1).astype(bool), N, 0)[1].size for k in range(K))
    cap = total // 2
    assert cap > 10
    masks = torch.empty((K, N), dtype=torch.uint8, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.cppf_segment_instances_workspace_bytes(N, P, K), dtype=torch.uint8, device=dev)

    def run(capacity, buf):
        _lib.check(L.cppf_segment_instances(case.d_idx.data_ptr(), d_bits.data_ptr(), P, N, K, 0, masks.data_ptr(), buf.data_ptr(), capacity,
                                            offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(dev)), "cppf_segment_instances")
        return offsets.cpu().numpy()
    buf = torch.full((cap + 64,), -7, dtype=torch.int32, device=dev)
    off = run(cap, buf)
    assert off[K] == total > cap
    got = buf.cpu().numpy()
    assert (got[cap:] == -7).all() and (got[:cap] >= 0).all()
    buf2 = torch.full((total + 64,), -7, dtype=torch.int32, device=dev)
    off2 = run(int(off[K]), buf2)
    got2 = buf2.cpu().numpy()
    assert np.array_equal(off2, off) and (got2[total:] == -7).all() and np.array_equal(got2[:cap], got[:cap])
    for k in range(K):
        assert np.array_equal(got2[off[k]:off[k + 1]], Z.segment(case.idx, ((bits >> np.uint32(k)) & 1).astype(bool), N, 0)[1])


def test_refusals(case, dev):
    L = _lib.lib()
    st = stream_ptr(dev)
    P, N = 64, case.pc.shape[0]
    bits = torch.zeros(P, dtype=torch.int32, device=dev)
    good = dict(points=case.d_pc.data_ptr(), outputs=case.d_out.data_ptr(), idx=case.d_idx.data_ptr(), corner=case.d_corner.data_ptr(),
                n=P, n_rots=72, centers=case.d_centers.data_ptr(), K=5, bits=bits.data_ptr())

    def bv(**kw):
        a = dict(good, **kw)
        return L.cppf_backvote_multi(a["points"], a["outputs"], a["idx"], a["corner"], RES, a["n"], a["n_rots"], *case.dims, a["centers"],
                                     a["K"], case.tol, a["bits"], None, st)
    assert bv() == 0
    for kw in (dict(K=0), dict(K=33), dict(K=-1), dict(n_rots=0), dict(points=None), dict(outputs=None), dict(idx=None), dict(corner=None),
               dict(centers=None), dict(bits=None), dict(n=1 << 27), dict(n=-1)):
        assert bv(**kw) == EINVAL, kw
    bits.fill_(-1)
    assert bv(n=0) == 0                                                         # launches nothing, writes nothing
    torch.cuda.synchronize()
    assert (bits.cpu().numpy() == -1).all()

    masks = torch.empty((5, N), dtype=torch.uint8, device=dev)
    pairs = torch.empty(P, dtype=torch.int32, device=dev)
    off = torch.empty(6, dtype=torch.int32, device=dev)
    ws = torch.empty(L.cppf_segment_instances_workspace_bytes(N, P, 5), dtype=torch.uint8, device=dev)
    sgood = dict(idx=case.d_idx.data_ptr(), bits=bits.data_ptr(), P=P, N=N, K=5, masks=masks.data_ptr(), pairs=pairs.data_ptr(), cap=P,
                 off=off.data_ptr(), ws=ws.data_ptr(), wsb=ws.numel())

    def seg(**kw):
        a = dict(sgood, **kw)
        return L.cppf_segment_instances(a["idx"], a["bits"], a["P"], a["N"], a["K"], 12, a["masks"], a["pairs"], a["cap"], a["off"], a["ws"],
                                        a["wsb"], st)
    bits.zero_()
    assert seg() == 0
    for kw in (dict(K=0), dict(K=33), dict(idx=None), dict(bits=None), dict(masks=None), dict(pairs=None), dict(off=None), dict(N=0),
               dict(P=-1), dict(cap=-1)):
        assert seg(**kw) == EINVAL, kw
    assert seg(ws=None) == EWORKSPACE and seg(wsb=ws.numel() - 1) == EWORKSPACE
    assert L.cppf_segment_instances_workspace_bytes(N, P, 0) == 0 and L.cppf_segment_instances_workspace_bytes(N, P, 33) == 0
    assert seg(P=0) == 0                                                        # no pairs: empty lists
    assert (off.cpu().numpy() == 0).all() and not masks.cpu().numpy().any()


def test_graph_replay_equals_eager(case, dev):
    P, K, N = P_MAX, 5, case.pc.shape[0]
    centers = case.d_centers[:K].contiguous()
    bits = torch.empty(P, dtype=torch.int32, device=dev)

    def chain():
        scene_poses.backvote_multi(case.d_pc, case.d_out, case.d_idx, case.d_corner, RES, case.dims, centers, 72, out=bits)
        return scene_poses.segment_instances(case.d_idx, bits, N, K, 12)
    eager = [t.cpu().numpy().copy() for t in chain()]                          # (also the warm-up: scratch allocated outside the capture)
    e_bits = bits.cpu().numpy().copy()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            outs = chain()
    bits.fill_(-1)
    for t in outs:
        t.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy(), e_bits) and np.array_equal(e_bits.view(np.uint32), case.want[72] & np.uint32(31))
    total = eager[2][K]
    assert np.array_equal(outs[0].cpu().numpy(), eager[0]) and np.array_equal(outs[2].cpu().numpy(), eager[2])
    assert np.array_equal(outs[1].cpu().numpy()[:total], eager[1][:total])
