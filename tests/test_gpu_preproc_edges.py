"""Pre-processing on the device at its edges: cppf_voxel_dedupe, cppf_knn (+ _dyn and the batched
launch), cppf_estimate_normals and the frame stage cppf_frame_cloud_dyn{,_batch}, each against the oracle bit for bit AND against
numpy definitions that share nothing with either (tests/preproc_cases.py: int64 index triples, a stable argsort, np.linalg.eigh of
a two-pass fp64 covariance).  The oracle is held to the same definitions on the CPU in tests/test_oracle_golden.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from cppf_amd import _lib
from cppf_amd._torch_util import call, scratch, stream_ptr
from cppf_amd.utils.util import backproject, estimate_normals, sparse_quantize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preproc_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------- voxel de-duplication
def _dedupe_everywhere(dev, oracle, pc, res, tag):
    """numpy in, device in and the oracle: all equal np.unique over the int64 index triples; coords are those triples"""
    want = PC.unique_first(pc, res)
    coords, idx = sparse_quantize(pc, return_index=True, quantization_size=res)
    assert np.array_equal(idx, want), (tag, "device vs np.unique", idx.size, want.size)
    assert np.array_equal(idx, oracle.voxel_dedupe(pc, res)), (tag, "device vs oracle")
    assert np.array_equal(coords, PC.voxel_index(pc, res).astype(np.int64)[want].astype(np.int32)), tag
    _, t_idx = sparse_quantize(torch.from_numpy(pc).to(dev), quantization_size=res)
    assert t_idx.is_cuda and np.array_equal(t_idx.cpu().numpy(), want), (tag, "device input")
    return want


@pytest.mark.parametrize("res", [0.004, 0.01, 0.03, 0.1])
def test_voxel_dedupe_on_voxel_faces(dev, oracle, res):
    """4000 points whose coordinates are float32(m * res) or one float32 step to either side: floor((double)p / res) decides"""
    _dedupe_everywhere(dev, oracle, PC.faces_cloud(res), res, res)


@pytest.mark.parametrize("res", [0.004, 0.01])
def test_voxel_dedupe_signs_around_the_origin(dev, oracle, res):
    """-0.0, +0.0 and every mix of signs: exactly the eight voxels around the origin"""
    assert _dedupe_everywhere(dev, oracle, PC.signs_cloud(res), res, res).size == 8


def test_voxel_dedupe_keeps_the_extreme_indices_apart(dev, oracle):
    """res = 0.5: indices -2^20 and 2^20 - 1 on every axis are in range and distinct from -2^20 + 1 and 2^20 - 2"""
    pc = PC.range_edge_cloud()
    assert PC.in_range(pc, PC.RANGE_RES)
    assert _dedupe_everywhere(dev, oracle, pc, PC.RANGE_RES, "range edges").size == 13


def _refused_not_merged(dedupe, pc, res, finite, tag):
    """`dedupe(pc, res)` must raise ValueError.  If it returns instead, its result is first compared with np.unique over the int64
    index triples, so that silently merged voxels are reported as what they are."""
    try:
        keep = dedupe(pc, res)
    except ValueError as e:
        return str(e)
    keep = np.asarray(keep.cpu() if hasattr(keep, "cpu") else keep)
    if finite:
        want = PC.unique_first(pc, res)
        assert np.array_equal(keep, want), (tag, "distinct voxels were merged", keep.tolist(), want.tolist())
    pytest.fail(f"{tag}: a cloud with a point out of the voxel range was not refused (kept {keep.size} of {pc.shape[0]})")


@pytest.mark.parametrize("case", range(10))
def test_voxel_dedupe_refuses_what_the_key_cannot_hold(dev, oracle, case):
    """indices 2^20 and -2^20 - 1 on each axis (res = 0.5; a masked key would alias them with -2^20 and 2^20 - 1, which the cloud
    also holds), the four points of which masking kept two, NaN, +inf, -inf: cppf_voxel_dedupe reports count = -1,
    sparse_quantize raises ValueError naming quantization_size and the extent for numpy and device input, the oracle raises; the
    next call on the same workspace is served as usual"""
    name, pc, res, finite = PC.refused_clouds()[case]
    assert not PC.in_range(pc, res), name
    for tag, fn in (("numpy input", lambda p, r: sparse_quantize(p, quantization_size=r)[1]),
                    ("device input", lambda p, r: sparse_quantize(torch.from_numpy(p).to(dev), quantization_size=r)[1])):
        msg = _refused_not_merged(fn, pc, res, finite, (name, tag))
        assert "quantization_size" in msg and f"{2 ** 20 * res:g}" in msg, msg
    with pytest.raises(ValueError):
        oracle.voxel_dedupe(pc, res)
    # the C entry point itself: count[0] = -1, decided on the stream
    t = torch.from_numpy(pc).to(dev)
    n = t.shape[0]
    keep = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.full((1,), 77, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.lib().cppf_voxel_dedupe_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    call("cppf_voxel_dedupe", dev, t, n, float(res), keep, count, scratch(ws))
    assert int(count.item()) == -1, name
    ok = PC.range_edge_cloud()[:n]                         # the flag word of that workspace does not outlive the call
    call("cppf_voxel_dedupe", dev, torch.from_numpy(ok).to(dev), ok.shape[0], PC.RANGE_RES, keep, count, scratch(ws))
    want = PC.unique_first(ok, PC.RANGE_RES)
    assert int(count.item()) == want.size and np.array_equal(keep[:want.size].cpu().numpy(), want), name


@pytest.mark.parametrize("n", PC.SIZES)
def test_voxel_dedupe_at_block_edges(dev, oracle, n):
    """N around the 256-thread blocks and the 1 024-byte compaction chunks: one voxel (one survivor, index 0), all distinct (all survive)"""
    one, distinct = PC.size_clouds(n)
    assert _dedupe_everywhere(dev, oracle, one, 0.004, (n, "one voxel")).tolist() == [0]
    assert _dedupe_everywhere(dev, oracle, distinct, 0.004, (n, "distinct")).size == n


# ----------------------------------------------------------------------------------------------- the frame stage
def _frame_buffers(L, dev, H, W, cap, k):
    z = lambda *s_, dt=torch.float32: torch.full(s_, -7, dtype=dt, device=dev)
    return dict(pc=z(cap, 3), nrm=z(cap, 3), corner=z(3), shape=z(4, dt=torch.int32), nbrs=z(cap, k, dt=torch.int32),
                ws=torch.zeros(int(L.cppf_frame_cloud_workspace_bytes(H, W, cap, k)), dtype=torch.uint8, device=dev),
                slot=torch.zeros(2, dtype=torch.int64, device=dev))


def _frame_batch(L, dev, bufs, spec, dd, u16, ld, H, W, kinv, divisor):
    """cppf_frame_cloud_dyn_batch over u8 labels; member j reads bit j; spec = [(cap, res, k, k_min)]"""
    arr = (_lib.FrameCloudItem * len(spec))()
    for j, (a, b, (cap, res, k, k_min)) in enumerate(zip(arr, bufs, spec)):
        b["slot"].copy_(torch.tensor([j, 0], dtype=torch.int64))
        a.label_bit_dev, a.seed_dev = b["slot"].data_ptr(), b["slot"].data_ptr() + 8
        a.pc_out, a.nrm_out, a.corner_out, a.shape_out, a.nbrs_out = (b[n].data_ptr() for n in ("pc", "nrm", "corner", "shape", "nbrs"))
        a.workspace, a.workspace_bytes = b["ws"].data_ptr(), b["ws"].numel()
        a.res, a.n_pairs, a.knn_k, a.k_min, a.n_cap, a.idx_is_i64 = res, 0, k, k_min, cap, 0
    with torch.cuda.device(dev):
        _lib.check(L.cppf_frame_cloud_dyn_batch(len(spec), C.cast(arr, C.c_void_p), dd.data_ptr(), u16, ld.data_ptr(), 1, H, W,
                                                kinv.ctypes.data, float(divisor), stream_ptr(dev)), "cppf_frame_cloud_dyn_batch")
    torch.cuda.synchronize()


def _frame_single(L, dev, b, spec, bit, dd, u16, ld, H, W, kinv, divisor):
    """cppf_frame_cloud_dyn, the bit by value"""
    cap, res, k, k_min = spec
    with torch.cuda.device(dev):
        _lib.check(L.cppf_frame_cloud_dyn(dd.data_ptr(), u16, ld.data_ptr(), 1, bit, H, W, kinv.ctypes.data, float(divisor), res, k, k_min,
                                          cap, b["pc"].data_ptr(), b["nrm"].data_ptr(), b["corner"].data_ptr(), b["shape"].data_ptr(),
                                          b["nbrs"].data_ptr(), b["ws"].data_ptr(), b["ws"].numel(), stream_ptr(dev)), "cppf_frame_cloud_dyn")
    torch.cuda.synchronize()


def _eager_cloud(dd, K, mask, divisor, res, k, k_min):
    """the four single calls (test_real_frame._eager_frame_cloud): backproject -> / divisor -> flips -> sparse_quantize -> cppf_knn ->
    estimate_normals, inference.grid_shape"""
    from cppf_amd.inference import grid_shape
    pts, _ = backproject(dd, K, mask, return_device=True)
    pc = pts / float(divisor)
    pc = torch.stack([-pc[:, 0], -pc[:, 1], pc[:, 2]], -1)
    _, keep = sparse_quantize(pc.float(), return_index=True, quantization_size=res)
    pc = pc[keep].float().contiguous()
    assert pc.shape[0] >= k_min
    nbrs = torch.empty((pc.shape[0], k), dtype=torch.int32, device=pc.device)
    call("cppf_knn", pc.device, pc, None, pc.shape[0], k, nbrs)
    corners, dims = grid_shape(pc.cpu().numpy(), res)
    return dict(pc=pc, nrm=estimate_normals(pc, k), nbrs=nbrs, corner=corners[0], dims=dims)


def _assert_member_equals(b, e, tag):
    n = e["pc"].shape[0]
    assert b["shape"].tolist() == [n, *e["dims"]], (tag, b["shape"], n, e["dims"])
    assert torch.equal(b["pc"][:n], e["pc"]) and torch.all(b["pc"][n:] == -7), tag
    assert torch.equal(b["nrm"][:n], e["nrm"]) and torch.all(b["nrm"][n:] == -7), tag
    assert torch.equal(b["nbrs"][:n], e["nbrs"]) and torch.all(b["nbrs"][n:] == -7), tag
    assert np.array_equal(b["corner"].cpu().numpy(), e["corner"]), tag


def _assert_member_refused(b, tag):
    assert b["shape"].tolist() == [0, 1, 1, 1] and b["corner"].tolist() == [0.0, 0.0, 0.0], (tag, b["shape"], b["corner"])
    assert torch.all(b["nrm"] == -7) and torch.all(b["nbrs"] == -7), tag


def test_frame_stage_refuses_a_member_out_of_range_and_no_other(dev):
    """One float-depth frame, kinv = I, divisor = 1 (a point is (u z, v z, z)), three members in one batched launch: one with a single
    pixel 5000 deep (voxel index 1 250 000 at res = 0.004), one with an inf depth pixel, one ordinary.  The first two report
    shape_out[0] = 0 -- the "fewer than k_min points" outcome, which every consumer skips -- where the eager path raises; the third
    equals the eager path bit for bit.  The single entry point refuses likewise, and serves the ordinary member next from the same
    workspace (the mark is cleared per launch)."""
    L = _lib.lib()
    H, W, res, k = 32, 64, 0.004, 16
    r, c = np.mgrid[0:H, 0:W]
    depth = (0.7 + 0.0005 * ((r * 7 + c * 3) % 11)).astype(np.float32)
    depth[3, 17] = 5000.0
    depth[14, 40] = np.inf
    labels = np.where(r < 10, 1, np.where(r < 20, 2, 4)).astype(np.uint8)
    K = np.eye(3)
    kinv = np.ascontiguousarray(np.eye(3))
    dd, ld = torch.from_numpy(depth).to(dev), torch.from_numpy(labels).to(dev)
    spec = [(1024, res, k, k + 1)] * 3
    bufs = [_frame_buffers(L, dev, H, W, 1024, k) for _ in spec]
    _frame_batch(L, dev, bufs, spec, dd, 0, ld, H, W, kinv, 1.0)
    for j in (0, 1):
        _assert_member_refused(bufs[j], ("batch", j))
        with pytest.raises(ValueError):
            _eager_cloud(dd, K, ((labels >> j) & 1).astype(np.uint8), 1.0, res, k, k + 1)
    want = _eager_cloud(dd, K, ((labels >> 2) & 1).astype(np.uint8), 1.0, res, k, k + 1)
    assert want["pc"].shape[0] > 700
    _assert_member_equals(bufs[2], want, "batch, ordinary member")
    one = _frame_buffers(L, dev, H, W, 1024, k)
    for j in (0, 1):
        _frame_single(L, dev, one, spec[j], j, dd, 0, ld, H, W, kinv, 1.0)
        _assert_member_refused(one, ("single", j))
    one["pc"].fill_(-7)
    _frame_single(L, dev, one, spec[2], 2, dd, 0, ld, H, W, kinv, 1.0)
    _assert_member_equals(one, want, "single, after two refusals")


@pytest.mark.parametrize("case", ["three_voxels", "all_distinct"])
def test_frame_stage_table_against_numpy_unique(dev, case):
    """The frame stage's voxel table at its two extremes, n_cap = 2 048 valid pixels each: all of them in 3 voxels (every insert
    walks the same probe chain and 2 045 atomicMin land on three slots) and all in distinct voxels (the table at its design load
    of one half).  The cloud it leaves = the points of np.unique's first occurrences over int64 index triples, in index order."""
    L = _lib.lib()
    H, W, res, cap = 32, 64, 0.004, 2048
    r, c = np.mgrid[0:H, 0:W]
    if case == "three_voxels":
        k, k_min, s = 1, 1, 1e-9                                         # kinv = diag(s, s, 1): x = s u z, y = s v z stay in voxel 0
        depth = (0.70 + 0.01 * ((r * W + c) % 3)).astype(np.float32)      # z in three voxels
    else:
        k, k_min, s = 30, 31, 1.0                                        # x = 0.7 u, y = 0.7 v: 175 voxels apart
        depth = np.full((H, W), 0.7, np.float32)
    kinv = np.ascontiguousarray(np.diag([s, s, 1.0]))
    z = depth.astype(np.float64).reshape(-1)
    pts = np.stack([(s * c.reshape(-1)) * z / 1.0, (s * r.reshape(-1)) * z / 1.0, z], -1).astype(np.float32)      # fp64, then .float()
    first = PC.unique_first(pts, res)
    assert first.size == (3 if case == "three_voxels" else cap) and PC.in_range(pts, res)
    dd, ld = torch.from_numpy(depth).to(dev), torch.ones((H, W), dtype=torch.uint8, device=dev)
    b = _frame_buffers(L, dev, H, W, cap, k)
    _frame_batch(L, dev, [b], [(cap, res, k, k_min)], dd, 0, ld, H, W, kinv, 1.0)
    n = first.size
    assert int(b["shape"][0]) == n, (b["shape"], n)
    assert np.array_equal(b["pc"][:n].cpu().numpy(), pts[first]) and torch.all(b["pc"][n:] == -7)
    assert np.array_equal(b["nbrs"][:n].cpu().numpy(), PC.knn_numpy(pts[first], k)[0])
    one = _frame_buffers(L, dev, H, W, cap, k)
    _frame_single(L, dev, one, (cap, res, k, k_min), 0, dd, 0, ld, H, W, kinv, 1.0)
    for name in ("pc", "nrm", "nbrs", "shape", "corner"):
        assert torch.equal(one[name], b[name]), name


# ----------------------------------------------------------------------------------------------- neighbour search
_KNN_CASES = [("clusters", 60), ("clusters", 16), ("clusters", 1), ("lattice", 30)] + [("small", nk) for nk in PC.SMALL_NK]
_knn_memo = {}


def _knn_case(name, arg):
    """(cloud, k, numpy's neighbour sets, candidates per query), computed once"""
    if (name, arg) not in _knn_memo:
        pc, k = (PC.small_cloud(arg[0]), arg[1]) if name == "small" else ({"clusters": PC.clusters_cloud, "lattice": PC.lattice_cloud}[name](), arg)
        want, key = PC.knn_numpy(pc, k)
        _knn_memo[(name, arg)] = (pc, k, want, PC.knn_candidates(key, k))
    return _knn_memo[(name, arg)]


@pytest.mark.parametrize("name,arg", _KNN_CASES)
def test_knn_against_a_stable_argsort(dev, oracle, name, arg):
    """cppf_knn and cppf_knn_dyn (capacity > N, NaN beyond N, the count in device memory) against float32 keys + stable argsort in
    numpy, and the oracle.  64 interleaved clusters at k = 60: every query has > 512 candidates under the pruning bound, none of
    them duplicates, so the re-streaming path runs on distinct keys; k = 16 and 1: the LDS path on the same cloud.  The raster-ordered
    lattice at k = 30: exact ties on both paths.  Clouds of 1 .. 100 points: fewer points than lanes, k = N."""
    pc, k, want, n_cand = _knn_case(name, arg)
    if name == "clusters":
        assert (n_cand.min() > 512) if k == 60 else (n_cand.max() <= 512), (k, n_cand.min(), n_cand.max())
    if name == "lattice":
        assert n_cand.min() <= 512 < n_cand.max()
    n = pc.shape[0]
    t = torch.from_numpy(pc).to(dev)
    got = torch.full((n, k), -5, dtype=torch.int32, device=dev)
    call("cppf_knn", dev, t, None, n, k, got)
    assert np.array_equal(got.cpu().numpy(), want), "cppf_knn vs numpy"
    assert np.array_equal(want, oracle.knn(pc, k)), "oracle vs numpy"
    cap = n + 67
    tc = torch.full((cap, 3), float("nan"), device=dev)
    tc[:n] = t
    got = torch.full((cap, k), -5, dtype=torch.int32, device=dev)
    call("cppf_knn_dyn", dev, tc, cap, torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev), k, got)
    got = got.cpu().numpy()
    assert np.array_equal(got[:n], want) and np.all(got[n:] == -5), "cppf_knn_dyn vs numpy"


def test_knn_as_members_of_one_batched_launch(dev):
    """The same clouds as members of ONE cppf_point_encoder_forward_batch launch (the search body picks its cloud, capacity and count
    by blockIdx.y): the clusters beside the lattice beside clouds of 64, 65 and 100 points, k = 60, capacities above the counts"""
    from cppf_amd.models.model import PointEncoder, point_encoder_forward_batch
    k = 60
    torch.manual_seed(3)
    enc = PointEncoder(k=k, spfcs=[32, 64, 32, 32], num_layers=1, out_dim=32).eval().to(dev)
    clouds = [PC.clusters_cloud(), PC.lattice_cloud(), PC.small_cloud(64), PC.small_cloud(65), PC.small_cloud(100)]
    members = []
    for pc in clouds:
        n, cap = pc.shape[0], pc.shape[0] + 61
        pcd, nrmd = torch.full((cap, 3), 7.0, device=dev), torch.zeros((cap, 3), device=dev)
        pcd[:n] = torch.from_numpy(pc).to(dev)
        nrmd[:, 2] = 1.0
        members.append(dict(encoder=enc, pc=pcd, nrm=nrmd, n_dev=torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev),
                            out=torch.full((cap, 40), -3.0, device=dev), nbrs=torch.full((cap, k), -5, dtype=torch.int32, device=dev)))
    assert point_encoder_forward_batch(members) is not None
    for i, (pc, m) in enumerate(zip(clouds, members)):
        nb = m["nbrs"].cpu().numpy()
        n = pc.shape[0]
        assert np.array_equal(nb[:n], PC.knn_numpy(pc, k)[0]) and np.all(nb[n:] == -5), i


# ----------------------------------------------------------------------------------------------- normals
_NORMAL_CLOUDS = PC.normal_clouds()


@pytest.mark.parametrize("case", range(len(_NORMAL_CLOUDS)), ids=[c[0] for c in _NORMAL_CLOUDS])
def test_normals_every_point_against_eigh(dev, oracle, case):
    """cppf_knn + cppf_estimate_normals, EVERY point: bit-equal to the oracle, and s = |n x e| against np.linalg.eigh of the two-pass
    fp64 covariance of the same neighbour set within 2^-23 + (k + 3) 2^-53 ||E[pp^T]||_F / (l1 - l0) (preproc_cases.normal_errors); unit
    length to 2^-23, largest component positive, finite.  The offset planes are what an fp32 accumulation anywhere in the covariance
    fails by orders of magnitude (fp32 cumulants give s = 1.0 there).  Worst s measured on an MI355X, equal to the oracle's on the CPU:
    plane at the origin 3.8e-8, at (0.3, -0.2, 1.2) 4.1e-8, in millimetres 4.1e-8, offset 1000 6.4e-6 (bound 6.2e-4), x10 offset 3e4
    6.0e-5 (bound 5.6e-3), depth-quantised 4.4e-8, sphere 4.4e-8, crease 4.0e-8, cube 4.0e-8, k = 3 4.0e-8, k = 4 4.2e-8, k = 64 3.2e-8."""
    name, pc, k, surface = _NORMAL_CLOUDS[case]
    nb = PC.knn_numpy(pc, k)[0]
    nr = estimate_normals(pc, k)
    assert np.array_equal(nr, oracle.estimate_normals(pc, nb)), name
    PC.check_normals(nr, pc, nb, surface, "device " + name)


def test_normals_where_there_is_no_normal_and_the_sign_tie(dev, oracle):
    """k = 2 and a straight line at k = 10: a unit vector orthogonal to the segment / the line (|n . d| <= 2^-23); k = 1 and 100 copies
    of one point: a finite unit vector, the oracle's; the lattice plane x + y = 0, whose two largest components are equal:
    (0.707107, 0.707107, 0) for every point, bit for bit the oracle's"""
    for pc, k in ((PC.small_cloud(300), 2), (PC.line_cloud(), 10)):
        nb = PC.knn_numpy(pc, k)[0]
        nr = estimate_normals(pc, k)
        assert np.array_equal(nr, oracle.estimate_normals(pc, nb)), k
        d = pc[nb[:, -1]].astype(np.float64) - pc[nb[:, 0]].astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        assert np.abs((nr.astype(np.float64) * d).sum(1)).max() <= 2.0 ** -23, k
        assert np.abs(np.linalg.norm(nr.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -23, k
    for pc, k in ((PC.small_cloud(100), 1), (np.repeat(PC.small_cloud(1), 100, 0), 30)):
        nr = estimate_normals(pc, k)
        assert np.array_equal(nr, oracle.estimate_normals(pc, PC.knn_numpy(pc, k)[0])), k
        assert np.isfinite(nr).all() and np.abs(np.linalg.norm(nr.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -23, k
    pc = PC.tie_plane_cloud()
    nr = estimate_normals(pc, 30)
    assert np.array_equal(nr, oracle.estimate_normals(pc, PC.knn_numpy(pc, 30)[0]))
    r = np.float32(np.sqrt(0.5))
    assert np.all(np.abs(nr - np.array([r, r, 0], np.float32)) <= 2.0 ** -23) and (nr[:, :2] > 0).all()


@pytest.mark.parametrize("case", ["offset_surface", "depth_quantised"])
def test_frame_stage_normals_against_eigh(dev, case):
    """fcb_finish_kernel is its own instantiation of the normals body: the frame stage's normals, every point, against eigh of the
    neighbour sets it reports (themselves against numpy's), same bound.  A float-depth surface 1000 units from the origin on every
    axis (only fp64 cumulants survive that) and a u16 millimetre frame of a sloped surface through a pinhole camera."""
    L = _lib.lib()
    H, W, k = 48, 60, 30
    r, c = np.mgrid[0:H, 0:W]
    if case == "offset_surface":
        depth = (1000.0 + 0.0008 * c + 0.0004 * r).astype(np.float32)
        kinv = np.ascontiguousarray(np.array([[4e-6, 0, 1.0], [0, 4e-6, 1.0], [0, 0, 1.0]]))       # x = (4e-6 u + 1) z: 4 mm pitch at 1000
        u16, dd, divisor, res = 0, torch.from_numpy(depth).to(dev), 1.0, 0.004
    else:
        depth = np.round(700 + 0.8 * r + 0.5 * c).astype(np.uint16)
        kinv = np.ascontiguousarray(np.linalg.inv(np.array([[591.0, 0, 30.0], [0, 590.0, 24.0], [0, 0, 1.0]])))
        u16, dd, divisor, res = 1, torch.from_numpy(depth.view(np.int16)).to(dev), 1000.0, 0.001     # (pixels are 1.2 mm apart at 0.7 m)
    cap = H * W
    b = _frame_buffers(L, dev, H, W, cap, k)
    _frame_batch(L, dev, [b], [(cap, res, k, k + 1)], dd, u16, torch.ones((H, W), dtype=torch.uint8, device=dev), H, W, kinv, divisor)
    n = int(b["shape"][0])
    assert n > cap // 2, n
    pc, nb, nr = b["pc"][:n].cpu().numpy(), b["nbrs"][:n].cpu().numpy(), b["nrm"][:n].cpu().numpy()
    if case == "offset_surface":
        assert np.abs(pc).min() > 999.0
    assert np.array_equal(nb, PC.knn_numpy(pc, k)[0])
    PC.check_normals(nr, pc, nb, True, "frame stage " + case)
