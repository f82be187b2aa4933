"""cppf_gather_instances (csrc/instances.hip) and scene_stage.voxel_owner on the device against tests/instances_ref.py, bit for bit:
member, offsets, pts, nrm, src on three chunks with a ragged last one and on a single point, for 1 / 7 / 32 proposals (an empty mask,
one that owns every point, two that share points, points without an owner), into poisoned buffers with a canary behind `capacity`;
one row short of room; an owner out of range; the refusals; the owner map on a cloud put through sparse_quantize."""
import numpy as np
import pytest
import torch

import instances_ref as R
from cppf_amd import _lib, scene_stage
from cppf_amd._torch_util import call
from cppf_amd.utils.util import sparse_quantize

pytestmark = pytest.mark.gpu
CHUNK = scene_stage.GATHER_CHUNK
GUARD = 8                                                                     # canary rows behind every buffer


def _d(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _buffers(dev, K, M, cap):
    """poisoned output buffers, GUARD entries longer than what the call may write"""
    f = lambda n: torch.full((n + GUARD, 3), float(R.POISON_F), dtype=torch.float32, device=dev)
    i = lambda n: torch.full((n + GUARD,), int(R.POISON_I), dtype=torch.int32, device=dev)
    return dict(member=i(M), offsets=i(K + 1), pts=f(cap), nrm=f(cap), src=i(cap))


def _run(dev, hi, nrm, owner, masks, cap):
    d = _d(dev)
    K, M = masks.shape[0], hi.shape[0]
    out = _buffers(dev, K, M, cap)
    scene_stage.gather_instances_device(d(hi), d(nrm), d(owner), d(masks), capacity=cap, out=out)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_equal(got, want, K, M, cap, tag):
    assert np.array_equal(got["offsets"][:K + 1], want["offsets"]), (tag, got["offsets"], want["offsets"])
    assert np.array_equal(got["member"][:M].view(np.uint32), want["member"]), tag
    for key in ("pts", "nrm"):
        assert np.array_equal(_bits(got[key][:cap]), _bits(want[key])), (tag, key)       # rows the call leaves alone: still poison
        assert (got[key][cap:] == R.POISON_F).all(), (tag, key, "canary")
    assert np.array_equal(got["src"][:cap], want["src"]) and (got["src"][cap:] == R.POISON_I).all(), tag
    assert (got["member"][M:] == R.POISON_I).all() and (got["offsets"][K + 1:] == R.POISON_I).all(), (tag, "canary")


@pytest.mark.parametrize("K", [1, 7, 32])
@pytest.mark.parametrize("M", [2 * CHUNK + 333, 1], ids=["three_chunks", "one_point"])
def test_gather_equals_the_restatement(dev, M, K):
    hi, nrm, owner, masks = R.case(M, K, N=301, seed=10 * K + (M > 1))
    total = int(R.gather_ref(hi, nrm, owner, masks)["offsets"][K])
    if M > 1:
        assert (owner == -1).sum() == 8
        if K >= 3:
            m = R.gather_ref(hi, nrm, owner, masks)["member"]
            assert (m & 1 == 0).all() and ((m >> np.uint32(K - 1)) & 1).sum() == M - 8 and (m & 6 == 6).any()
    # roomy: room for every row
    roomy = _run(dev, hi, nrm, owner, masks, total + 5)
    _assert_equal(roomy, R.gather_ref(hi, nrm, owner, masks, capacity=total + 5), K, M, total + 5, "roomy")
    # the default capacity, M rows: enough for any one proposal, the packed rows are cut there
    _assert_equal(_run(dev, hi, nrm, owner, masks, M), R.gather_ref(hi, nrm, owner, masks), K, M, M, "capacity M")
    if total >= 1:
        # one row short: complete offsets, canary intact, and the caller's second call equals the roomy one
        short = _run(dev, hi, nrm, owner, masks, total - 1)
        _assert_equal(short, R.gather_ref(hi, nrm, owner, masks, capacity=total - 1), K, M, total - 1, "short")
        assert int(short["offsets"][K]) == total > total - 1
        again = _run(dev, hi, nrm, owner, masks, int(short["offsets"][K]))
        for key in ("pts", "nrm", "src"):
            assert np.array_equal(_bits(again[key][:total]), _bits(roomy[key][:total])), key
    # no room at all: offsets only
    none = _run(dev, hi, nrm, owner, masks, 0)
    _assert_equal(none, R.gather_ref(hi, nrm, owner, masks, capacity=0), K, M, 0, "capacity 0")


def test_the_wrapper_reads_offsets_once_and_calls_again(dev):
    hi, nrm, owner, masks = R.case(2 * CHUNK + 333, 7, N=301, seed=5)
    d = _d(dev)
    want = R.gather_ref(hi, nrm, owner, masks, capacity=10 ** 6)
    T = int(want["offsets"][7])
    assert T > hi.shape[0]                                                    # more rows than the default capacity: the second call
    for cap in (None, 3, T):
        pts, nr, src, off, member = scene_stage.gather_instances(d(hi), d(nrm), d(owner), d(masks), capacity=cap)
        assert off.dtype == np.int64 and np.array_equal(off, want["offsets"]) and pts.shape == (T, 3) and src.shape == (T,)
        assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want["pts"][:T])) and np.array_equal(src.cpu().numpy(), want["src"][:T])
        assert np.array_equal(_bits(nr.cpu().numpy()), _bits(want["nrm"][:T]))
        assert np.array_equal(member.cpu().numpy().view(np.uint32), want["member"])
        for k in range(7):                                                    # hi[member_k] on the host
            rows = np.nonzero((want["member"] >> np.uint32(k)) & 1)[0]
            assert np.array_equal(pts[int(off[k]):int(off[k + 1])].cpu().numpy(), hi[rows])


@pytest.mark.parametrize("where,value", [(0, 301), (CHUNK + 5, 2 ** 31 - 1), (2 * CHUNK + 332, 302)])
def test_an_owner_out_of_range_is_reported_and_nothing_is_gathered(dev, where, value):
    hi, nrm, owner, masks = R.case(2 * CHUNK + 333, 7, N=301, seed=9)
    owner[where] = value
    K, M = 7, hi.shape[0]
    got = _run(dev, hi, nrm, owner, masks, 4 * M)
    assert got["offsets"][:K + 1].tolist() == [0] * K + [-1]
    for key in ("pts", "nrm"):
        assert (got[key] == R.POISON_F).all(), key
    assert (got["src"] == R.POISON_I).all() and (got["member"][M:] == R.POISON_I).all()
    d = _d(dev)
    with pytest.raises(ValueError, match="owner"):
        scene_stage.gather_instances(d(hi), d(nrm), d(owner), d(masks))


def test_refusals(dev):
    hi, nrm, owner, _ = R.case(40, 2, N=20, seed=1)
    d = _d(dev)
    masks33 = torch.zeros((33, 20), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="1..32"):
        scene_stage.gather_instances(d(hi), d(nrm), d(owner), masks33)
    out = _buffers(dev, 33, 40, 40)
    counts = torch.zeros(33, dtype=torch.int32, device=dev)
    args = lambda K, cap: (d(hi), d(nrm), d(owner), masks33, K, 20, 40, cap, out["member"], out["offsets"], out["pts"], out["nrm"], out["src"], counts)
    assert call("cppf_gather_instances", dev, *args(33, 40), ok=(-1,)) == -1
    assert call("cppf_gather_instances", dev, *args(0, 40), ok=(-1,)) == -1
    assert call("cppf_gather_instances", dev, *args(2, -1), ok=(-1,)) == -1
    with pytest.raises(_lib.CppfError, match=r"cppf_gather_instances failed \(-1\)"):
        call("cppf_gather_instances", dev, *args(33, 40))
    torch.cuda.synchronize(dev)
    assert (out["src"] == int(R.POISON_I)).all() and (out["offsets"] == int(R.POISON_I)).all()        # nothing was launched
    with pytest.raises(ValueError, match="expected"):
        scene_stage.gather_instances(d(hi), d(nrm), d(owner)[:-1], masks33[:2])
    # an empty dense cloud: offsets all zero
    e = scene_stage.gather_instances(d(hi)[:0], d(nrm)[:0], d(owner)[:0], masks33[:3])
    assert e[3].tolist() == [0, 0, 0, 0] and e[0].shape == (0, 3)


def test_voxel_owner_on_a_quantised_cloud(dev):
    """a cloud with coordinates ON voxel faces (where a reciprocal multiply parts from the division) through sparse_quantize: every
    point has an owner, the map equals the restatement, and a mask with ONE sparse point set gathers exactly that voxel's dense
    points, found by fp64 floor on the host"""
    q = R.FACE_Q[0]
    faces, m = R.face_cloud(q, 4100)
    rng = np.random.default_rng(4)
    keep = np.concatenate([np.nonzero(m % 25 == 0)[0], rng.integers(0, m.size, 400)])
    a = faces[keep].copy()
    a[:, 1:] = (rng.uniform(-1.5, 1.5, (a.shape[0], 2)) * q).astype(np.float32)
    hi = np.concatenate([a, a + np.float32(0.2 * q) * rng.random((a.shape[0], 3), dtype=np.float32),
                         (rng.uniform(-3, 3, (1500, 3)) * q).astype(np.float32)])
    hi = hi[rng.permutation(hi.shape[0])]
    v = R.voxels(hi, q)
    assert (v[:, 0] != R.voxels_reciprocal(hi, q)[:, 0]).sum() >= 20          # the input tells the two apart
    d = _d(dev)
    hi_d = d(hi)
    _, ind = sparse_quantize(hi_d, return_index=True, quantization_size=q)
    owner = scene_stage.voxel_owner(hi_d, ind, q)
    assert owner.dtype == torch.int32 and owner.device == hi_d.device and owner.shape == (hi.shape[0],)
    own, ind_h = owner.cpu().numpy(), ind.cpu().numpy()
    assert (own >= 0).all() and np.array_equal(own, R.owner_ref(hi, ind_h, q))
    assert not np.array_equal(own, R.owner_ref(hi, ind_h, q, voxel_fn=R.voxels_reciprocal))
    assert np.array_equal(v[ind_h[own]], v) and np.bincount(own).max() >= 2
    nrm = rng.standard_normal(hi.shape).astype(np.float32)
    sep = np.nonzero(v[:, 0] != R.voxels_reciprocal(hi, q)[:, 0])[0]
    for j in (int(own[sep[0]]), int(own[sep[-1]]), 0, ind_h.size - 1):        # two voxels with a separating face point among them
        mask = np.zeros((1, ind_h.size), np.uint8)
        mask[0, j] = 1
        pts, nr, src, off, _ = scene_stage.gather_instances(hi_d, d(nrm), owner, d(mask))
        rows = np.nonzero((v == v[ind_h[j]]).all(1))[0]
        assert off.tolist() == [0, rows.size] and np.array_equal(src.cpu().numpy(), rows)
        assert np.array_equal(pts.cpu().numpy(), hi[rows]) and np.array_equal(nr.cpu().numpy(), nrm[rows])
    # a caller's own subset: voxels it leaves out have no owner
    sub = ind[::2].contiguous()
    own2 = scene_stage.voxel_owner(hi_d, sub, q).cpu().numpy()
    assert np.array_equal(own2, R.owner_ref(hi, sub.cpu().numpy(), q)) and (own2 == -1).any() and (own2 >= 0).any()
