"""The device's statements of the vote grid's dims and corners against the float64 reference of tests/grid_dims_cases.py -- exactly:
  cppf_grid_setup     (grid_setup_kernel, pose_tail.hip: one block of 1024 threads) -- what put() asks for a device tensor's dims
  cppf_stage_batch    (fc_grid_body, preproc.hip, in a block of 256 threads) -- the shape record a staged chain's vote runs on
The frame stage's fcb_finish_kernel calls the same fc_grid_body with the same block size as cppf_stage_batch and is covered by it.
(cppf_grid_from_raw, for all its name, converts a vote's integer image to floats and computes no dims: there is nothing of it to hold
to this reference.)

The host's grid_shape chooses the pipeline -- tile class and capacity -- from ITS dims, the vote runs on the DEVICE's: one cell of
disagreement at a class boundary is a refused instance.  On random clouds the quotient never sits near an integer, so the cases put
it there: extents k * res +-3 ulp, every one of them that a reciprocal-multiply or an unrounded double quotient gets wrong, and a
thinned rest.  The placement matrix moves the minimum and the maximum through the lanes, waves and trips of the block reduction."""
import numpy as np
import pytest
import torch

import grid_dims_cases as G
from cppf_amd import _lib
from cppf_amd._torch_util import stream_ptr

pytestmark = pytest.mark.gpu


def _pack(cases, dev):
    """all clouds in one device buffer -> (buffer, [float offset of every cloud])"""
    offs, total = [], 0
    for c in cases:
        offs.append(total)
        total += 3 * c["pc"].shape[0]
    host = np.concatenate([np.ascontiguousarray(c["pc"], np.float32).ravel() for c in cases])
    assert host.size == total
    return torch.from_numpy(host).to(dev), offs


def _compare(cases, corner, dims, entry):
    """corner f32[n,3] / dims i32[n,3] as the device wrote them against every case's reference"""
    bad = []
    for j, c in enumerate(cases):
        if tuple(int(v) for v in dims[j]) != c["dims"] or not G.corners_equal(corner[j], c["corners"][0], c["by_value"]):
            bad.append((c["name"], tuple(int(v) for v in dims[j]), c["dims"], corner[j].tolist(), c["corners"][0].tolist()))
    assert not bad, (entry, len(bad), bad[:5])


def run_grid_setup(cases, dev):
    L = _lib.lib()
    src, offs = _pack(cases, dev)
    out = torch.full((len(cases), 8), -7, dtype=torch.int32, device=dev)        # corner f32[3] (bits) | pad | dims i32[3] | pad
    st = stream_ptr(dev)
    for j, c in enumerate(cases):
        n = c["pc"].shape[0]
        assert offs[j] + 3 * n <= src.numel()
        _lib.check(L.cppf_grid_setup(src.data_ptr() + 4 * offs[j], n, float(np.float32(c["res"])), out[j].data_ptr(),
                                     out[j].data_ptr() + 16, st), "cppf_grid_setup")
    host = out.cpu().numpy()
    assert (host[:, 3] == -7).all() and (host[:, 7] == -7).all()                # the words between and behind stay untouched
    return host[:, 0:3].copy().view(np.float32), host[:, 4:7]


def run_stage_batch(cases, dev):
    """eight clouds per launch; every member copies its cloud into a slot of its own (capacity = the largest cloud) and draws nothing"""
    L = _lib.lib()
    src, offs = _pack(cases, dev)
    n = len(cases)
    cap = max(c["pc"].shape[0] for c in cases)
    desc_host = np.zeros((n, _lib.STAGE_DESC_WORDS), np.uint64)
    for j, c in enumerate(cases):
        p = src.data_ptr() + 4 * offs[j]
        desc_host[j] = (p, p, 0, c["pc"].shape[0], j, j)                        # (the cloud stands in for its normals: only copied)
    desc = torch.from_numpy(desc_host.view(np.int64)).to(dev)
    slots = torch.zeros((8, 2, cap, 3), dtype=torch.float32, device=dev)
    corner = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
    shape = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    for g in range(0, n, 8):
        m = min(8, n - g)
        arr = (_lib.StageItem * m)()
        for q in range(m):
            a, c = arr[q], cases[g + q]
            a.desc = desc[g + q].data_ptr()
            a.pc, a.nrm, a.feat = slots[q, 0].data_ptr(), slots[q, 1].data_ptr(), None
            a.corner, a.shape = corner[g + q].data_ptr(), shape[g + q].data_ptr()
            a.idx, a.u_tr, a.u_rot = None, None, None
            a.n_pairs, a.n_cap, a.F, a.res, a.idx_is_i64 = 0, c["pc"].shape[0], 0, float(np.float32(c["res"])), 1
            assert a.n_cap <= cap
        _lib.check(L.cppf_stage_batch(m, arr, st), "cppf_stage_batch")
    corner, shape = corner.cpu().numpy(), shape.cpu().numpy()
    assert (corner[:, 3] == -7.0).all()
    assert shape[:, 0].tolist() == [c["pc"].shape[0] for c in cases]            # the record's point count
    last = cases[(n - 1) // 8 * 8]                                              # (slot 0 still holds the last launch's first cloud)
    assert np.array_equal(slots[0, 0, :last["pc"].shape[0]].cpu().numpy(), last["pc"])
    return corner[:, :3], shape[:, 1:4]


ENTRIES = {"cppf_grid_setup": (run_grid_setup, 1024), "cppf_stage_batch": (run_stage_batch, 256)}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_device_dims_at_the_division_edges_equal_the_reference(dev, entry):
    """every case that differs under either mistake, for every resolution, plus every 16th of the rest and the further cases"""
    assert all(c in G.DEVICE_CASES for c in G.CASES if c["biting"])
    corner, dims = ENTRIES[entry][0](G.DEVICE_CASES, dev)
    _compare(G.DEVICE_CASES, corner, dims, entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_device_reduction_finds_the_extremes_wherever_they_sit(dev, entry):
    """N in {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049}; minimum and maximum, independently, at index 0, 63, 64, N - 1 and
    the last index of the block's first trip, the rest strictly inside: a lost lane, wave or second trip moves a corner or the dims"""
    run, block = ENTRIES[entry]
    cases = G.placement_cases(block)
    corner, dims = run(cases, dev)
    _compare(cases, corner, dims, entry)


def test_runner_host_dims_and_device_dims_agree_at_biting_extents(dev):
    """three objects of ~600 points whose x extent is a biting case at the object's own resolution, as a host-array batch through
    BatchPoseRunner's staged path (the HOST's dims choose the pipelines, the device's shape record is what the vote sees): nobody
    is refused, every pipeline's device shape words equal the host's grid_shape, and the records equal those of a fresh runner fed
    the same objects as device tensors through put(), whose dims the DEVICE computes"""
    import cppf_amd.synthetic as syn
    from cppf_amd.batch import BatchPoseRunner
    from cppf_amd.config import NOCS_CATEGORIES
    from cppf_amd.inference import grid_shape
    from test_gpu_configs import make_encoder, seeded_sd
    sd = seeded_sd(3, 4.0)
    cats = ("bottle", "laptop", "mug")                                       # res 0.004, 0.01, 0.004
    encoders = {c: make_encoder(sd, dev) for c in NOCS_CATEGORIES}
    objects = []
    for j, cat in enumerate(cats):
        ob = syn.make_object(cat, 600, 900 + j)
        pc = np.ascontiguousarray(ob["pc"], np.float32).copy()
        r = np.float32(ob["cfg"].res)
        i_lo, i_hi = int(pc[:, 0].argmin()), int(pc[:, 0].argmax())
        # the minimum moves down to a multiple of 2^-10 (less than a millimetre), so that lo + e is a float32 for the extents around;
        # the maximum to the biting extent nearest above the rest of the cloud for which it is: a few cells at most
        lo = pc[i_lo, 0] = np.float32(np.floor(np.float64(pc[i_lo, 0]) * 1024) / 1024)
        second = np.sort(pc[:, 0])[-2]
        pick = None
        for e in sorted(G.BITING[float(r)]["extents"]):
            h = np.float32(np.float64(lo) + np.float64(e))
            if h > second and np.float32(h - lo) == e and np.float64(h) == np.float64(lo) + np.float64(e):
                pick = (e, h)
                break
        assert pick is not None, cat
        pc[i_hi, 0] = pick[1]
        assert np.float32(pc[:, 0].max() - pc[:, 0].min()) == pick[0]
        want_x = G.ref_dims_axis(pick[0], r)
        assert want_x != G.recip_dims_axis(pick[0], r) or want_x != G.double_dims_axis(pick[0], r)
        assert grid_shape(pc, r)[1] == G.reference(pc, r)[1] and grid_shape(pc, r)[1][0] == want_x
        objects.append(dict(pc=pc, normals=ob["normals"], feat=ob["feat"], cfg=ob["cfg"], n_pairs=20000))
    runner = BatchPoseRunner(encoders, dev)
    rec = runner.run(objects, seed=5)
    assert rec.is_cuda                                                       # the staged path
    rec = rec.cpu().numpy()
    ran = runner._checks[-1]["ran"]                                          # the batch's chains and the rows they served
    runner.check()
    assert (rec[:, 12] >= 0).all(), rec[:, 12]
    shapes = {}
    for chain, slots in ran:
        for pipe, s in zip(chain.pipes, slots):
            shapes[s] = [int(v) for v in pipe.shape.cpu()]
    for j, o in enumerate(objects):
        assert shapes[j] == [o["pc"].shape[0], *grid_shape(o["pc"], o["cfg"].res)[1]], (j, shapes[j])
    fresh = BatchPoseRunner(encoders, dev)
    on_dev = [dict(o, pc=torch.from_numpy(o["pc"]).to(dev), normals=torch.from_numpy(o["normals"]).to(dev),
                   feat=torch.from_numpy(o["feat"]).to(dev)) for o in objects]
    res = fresh.put(on_dev)
    assert [o["dims"] for o in res] == [grid_shape(o["pc"], o["cfg"].res)[1] for o in objects]
    np.testing.assert_array_equal(fresh.run(res, seed=5).cpu().numpy(), rec)
    fresh.check()
