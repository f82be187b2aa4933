"""csrc/mesh_stats.hip at its edges on the MI355X, bit for bit against the restatement (tests/mesh_stats_ref.py): end counts that
decrease behind a block boundary, the face loops, the pair loop and ms_final_kernel beyond their first trip or workgroup, the block
edges of the stated summation order, every status leg, the mesh counter at 2^32 - 1 and the host refusals.  Cases:
tests/mesh_stats_cases.py; that each reaches its edge: tests/test_mesh_stats_cases_cpu.py.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import mesh_stats_cases as C
import mesh_stats_ref as SR
from cppf_amd import _lib
from cppf_amd import mesh_stats as MS
from cppf_amd._torch_util import call, scratch

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy()


def _check_batch(dev, meshes, n, seed, first_mesh=0):
    """one batched call against the restatement, mesh by mesh; returns the device points"""
    pts, fid, status = MS.sample_surface_batch(meshes, n, seed=seed, first_mesh=first_mesh, device=dev)
    assert _np(status).tolist() == [0] * len(meshes)
    p, t = _np(pts), _np(fid)
    for m, (v, f) in enumerate(meshes):
        ref, rt, _, ok = SR.sample_surface(v, f, n, seed, first_mesh + m)
        assert ok
        assert np.array_equal(t[m], rt), (m, f.shape[0], n, np.flatnonzero(t[m] != rt)[:5])
        assert np.array_equal(p[m], ref), (m, f.shape[0], n)
    return pts


# ------------------------------------------------------------------------------------------------ 1. the face rule
@pytest.mark.parametrize("i", range(len(C.DIP_CASES)))
def test_points_behind_a_decreasing_end_count(dev, i):
    case = C.DIP_CASES[i]
    v, f, _, E = C.dip_case(i)
    ref, rt = C.dip_sample(i)
    pts, fid = MS.sample_surface(v, f, case["N"], seed=C.DIP_SEED, device=dev, return_faces=True)
    t = _np(fid)
    ks = C.dip_points(E, case["t"])
    assert np.array_equal(t, rt), (f"E decreases at face {case['t']}: points k = E_t+1 - 1, E_t+1, E_t - 1 = {ks} lie on faces "
                                   f"{t[ks].tolist()}, the first faces with E > k are {rt[ks].tolist()}; "
                                   f"{int((t != rt).sum())} face ids differ")
    assert np.array_equal(_np(pts), ref), ks


# ------------------------------------------------------------------------------------------------ 2. second trips
def test_face_loops_beyond_one_trip(dev):
    _check_batch(dev, C.face_trip_batch(), 2048, 11)


@pytest.mark.parametrize("name", list(C.PAIR_CASES))
def test_pair_loop_beyond_one_trip(dev, name):
    c = C.PAIR_CASES[name]
    want = C.pair_rows(name)["full"]
    pts = torch.from_numpy(C.pair_points(name)).to(dev)
    st, status = MS.vote_stats_batch(pts, c["P"], seed=c["seed"])
    st = _np(st)
    assert _np(status).tolist() == [0] * c["M"]
    assert np.array_equal(st, want), np.flatnonzero((st != want).any(1))[:8]
    if name == "three_trips":                     # ms_final_kernel beyond 256 meshes: a row does not depend on its place
        for m in (0, 255, 256, 257, 300, 383, 384, 511):
            sm, _ = MS.vote_stats_batch(pts[m:m + 1], c["P"], seed=c["seed"], first_mesh=m)
            assert np.array_equal(_np(sm)[0], want[m]), m


# ------------------------------------------------------------------------------------------------ 3. block edges
@pytest.mark.parametrize("n", C.EDGE_NS)
def test_block_edges_of_the_summation_order(dev, n):
    _check_batch(dev, C.edge_meshes(), n, 13)


# ------------------------------------------------------------------------------------------------ 5. status legs
def test_sampling_status_words(dev):
    meshes, n, seed = C.status_batch(), 2048, 17
    pts, fid, status = MS.sample_surface_batch(meshes, n, seed=seed, device=dev)
    assert _np(status).tolist() == C.STATUS_WORDS          # (a face index outside: bit 2, and bit 1 through the NaN area)
    p, t = _np(pts), _np(fid)
    for m, ((v, f), word) in enumerate(zip(meshes, C.STATUS_WORDS)):
        if word:
            assert np.isnan(p[m]).all() and (t[m] == -1).all(), m
            continue
        ref, rt, _, ok = SR.sample_surface(v, f, n, seed, m)
        assert ok and np.array_equal(p[m], ref) and np.array_equal(t[m], rt), m
        pm, fm, sm = MS.sample_surface_batch([meshes[m]], n, seed=seed, first_mesh=m, device=dev)
        assert int(sm.item()) == 0 and torch.equal(pm[0], pts[m]) and torch.equal(fm[0], fid[m]), m


@pytest.mark.parametrize("N", C.BAD_NS)
def test_one_bad_coordinate_flags_its_row_alone(dev, N):
    sets, want = C.bad_point_batch(N)
    st, status = MS.vote_stats_batch(torch.from_numpy(sets).to(dev), 1000, seed=19)
    st = _np(st)
    assert _np(status).tolist() == want
    for m, w in enumerate(want):
        if w:
            assert np.isnan(st[m]).all(), m
        else:
            assert np.array_equal(st[m], SR.vote_stats(sets[m], 1000, 19, m)), m


def test_one_point_and_identical_points(dev):
    for pts in (np.array([[[0.3, -0.2, 0.7]]]), np.tile(np.array([0.3, -0.2, 0.7]), (1, 100, 1))):
        st, status = MS.vote_stats_batch(torch.from_numpy(pts).to(dev), 500, seed=23)
        want = SR.vote_stats(pts[0], 500, 23, 0)
        assert int(status.item()) == 0 and want[0] == 0 and (want[3:] == 0).all()
        assert np.array_equal(_np(st)[0], want), (_np(st)[0], want)


# ------------------------------------------------------------------------------------------------ 6. counter and host edges
def test_mesh_counter_at_its_top(dev):
    meshes, n, seed, top = C.edge_meshes()[2:5], 300, 29, C.FIRST_MESH_TOP
    pts = _check_batch(dev, meshes, n, seed, first_mesh=top)
    assert top + len(meshes) - 1 == 2 ** 32 - 1
    st, status = MS.vote_stats_batch(pts, 700, seed=seed, first_mesh=top)
    assert _np(status).tolist() == [0, 0, 0]
    for m in range(3):
        pm, _, _ = MS.sample_surface_batch([meshes[m]], n, seed=seed, first_mesh=top + m, device=dev)
        assert torch.equal(pm[0], pts[m]), m
        sm, _ = MS.vote_stats_batch(pm, 700, seed=seed, first_mesh=top + m)
        want = SR.vote_stats(_np(pts[m]), 700, seed, top + m)
        assert np.array_equal(_np(sm)[0], want) and np.array_equal(_np(st)[m], want), m
    one, status = MS.vote_stats_batch(pts[:1], 1, seed=seed, first_mesh=top)             # n_pairs = 1
    assert int(status.item()) == 0 and np.array_equal(_np(one)[0], SR.vote_stats(_np(pts[0]), 1, seed, top))


def test_host_refusals_leave_the_outputs_alone(dev):
    L = _lib.lib()
    meshes = C.edge_meshes()[1:4]
    verts, faces, voff, foff = MS.upload_meshes(meshes, dev)
    M, n = len(meshes), 64
    ws = torch.empty(L.cppf_surface_sample_workspace_bytes(M, int(foff[-1])), dtype=torch.uint8, device=dev)
    pts = torch.full((M, n, 3), -7.0, dtype=torch.float64, device=dev)
    fid = torch.full((M, n), -7, dtype=torch.int32, device=dev)
    status = torch.full((M,), -7, dtype=torch.int32, device=dev)

    def sample(vo=voff, fo=foff, m=M, n_points=n, first=0):
        return call("cppf_surface_sample_batch", dev, verts, faces, np.ascontiguousarray(vo), np.ascontiguousarray(fo), m, n_points, 31,
                    first, pts, fid, status, scratch(ws), ok=(C.EINVAL,))

    shifted = foff.copy()
    shifted[0] = 1
    empty = foff.copy()
    empty[2] = empty[1]
    refused = dict(no_meshes=dict(m=0), offsets_from_one=dict(fo=shifted), vertex_offsets_from_one=dict(vo=voff + 1),
                   mesh_without_faces=dict(fo=empty), no_points=dict(n_points=0), too_many_points=dict(n_points=2 ** 31),
                   counter_overflow=dict(first=2 ** 32 + 1 - M), negative_counter=dict(first=-1))
    for why, kw in refused.items():
        assert sample(**kw) == C.EINVAL, why
    torch.cuda.synchronize(dev)
    assert (pts == -7).all() and (fid == -7).all() and (status == -7).all()
    assert sample(first=2 ** 32 - M) == 0 and (status == 0).all()                        # the largest counter is taken
    assert L.cppf_surface_sample_workspace_bytes(0, 10) == 0 and L.cppf_surface_sample_workspace_bytes(3, 2) == 0

    p = torch.from_numpy(np.random.default_rng(3).normal(0, 0.1, (M, n, 3))).to(dev)
    stats = torch.full((M, 6), -7.0, dtype=torch.float64, device=dev)
    vstatus = torch.full((M,), -7, dtype=torch.int32, device=dev)
    vws = torch.empty(L.cppf_mesh_vote_stats_workspace_bytes(M, n, 1000), dtype=torch.uint8, device=dev)

    def stat(m=M, n_points=n, pairs=1000, first=0):
        return call("cppf_mesh_vote_stats_batch", dev, p, m, n_points, pairs, 31, first, stats, vstatus, scratch(vws), ok=(C.EINVAL,))

    refused = dict(no_meshes=dict(m=0), no_points=dict(n_points=0), too_many_points=dict(n_points=2 ** 31), no_pairs=dict(pairs=0),
                   too_many_pairs=dict(pairs=2 ** 32), counter_overflow=dict(first=2 ** 32 + 1 - M), negative_counter=dict(first=-1))
    for why, kw in refused.items():
        assert stat(**kw) == C.EINVAL, why
    torch.cuda.synchronize(dev)
    assert (stats == -7).all() and (vstatus == -7).all()
    assert L.cppf_mesh_vote_stats_workspace_bytes(M, n, 2 ** 32) == 0 and L.cppf_mesh_vote_stats_workspace_bytes(M, n, 2 ** 32 - 1) > 0
    assert stat(first=2 ** 32 - M) == 0 and (vstatus == 0).all()
