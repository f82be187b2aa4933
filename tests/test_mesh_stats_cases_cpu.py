"""That every case of tests/mesh_stats_cases.py reaches the edge of csrc/mesh_stats.hip it is named for, shown on the CPU with the
restatement (tests/mesh_stats_ref.py) alone: end counts that decrease behind a block boundary and the face rule there, batches
beyond one trip of the face loops, pair counts whose later trips hold the maxima, the block edges of the stated summation order,
the status words -- and the restated counts against exact rational arithmetic, so that the restatement cannot drift together with
the kernel."""
import itertools

import numpy as np
import pytest

import mesh_stats_cases as C
import mesh_stats_ref as SR


# ------------------------------------------------------------------------------------------------ 1. the face rule
@pytest.mark.parametrize("i", range(len(C.DIP_CASES)))
def test_end_counts_decrease_and_the_first_face_rule_holds(i):
    case = C.DIP_CASES[i]
    v, f, Cc, E = C.dip_case(i)
    N, t = case["N"], case["t"]
    assert f.shape[0] == case["F"] and N < 2 ** 22
    assert E[t] == E[t + 1] + 1 and (t + 1) % -(-case["F"] // SR.LANES) == 0          # a decrease, behind a block boundary
    pts, face = C.dip_sample(i)
    for k in C.dip_points(E, t):
        assert face[k] == np.argmax(E > k), (k, face[k], np.argmax(E > k))
    k = int(E[t + 1])
    assert face[k] == case["first"] <= t and (E[t + 1:t + 2] <= k).all()               # k's face lies before the dip, not behind it
    cnt = np.bincount(face, minlength=f.shape[0])
    assert np.array_equal(cnt, SR.open3d_counts(Cc, N)) and cnt.sum() == N
    assert (cnt[SR.areas(v, f) == 0] == 0).all()
    # the kernel's bisection of E itself, as it stood: right or wrong by where its probes fall
    assert C.kernel_bisection(E, k) == (case["first"] if case["late"] is None else case["late"])
    p0, p1, p2 = (v[f[face, j]] for j in range(3))
    nrm = np.cross(p1 - p0, p2 - p0)
    assert np.abs(np.einsum("ij,ij->i", pts - p0, nrm)).max() < 1e-12                  # the points lie in their faces' planes


def test_some_fixed_case_sends_the_old_bisection_to_a_later_face():
    late = [c for c in C.DIP_CASES if c["late"] is not None]
    assert late and all(c["late"] > c["t"] + 1 for c in late)


def test_the_search_finds_the_fixed_case():
    """search_dips on the cheapest fixed case (its N is found in the first block of the search)"""
    case = min(C.DIP_CASES, key=lambda c: c["N"])
    got = list(C.search_dips(case["F"], [case["seed"]], **case["kw"]))
    assert [(g["N"], g["t"]) for g in got] == [(case["N"], case["t"])]


# ------------------------------------------------------------------------------------------------ 2. second trips
def test_face_batch_straddles_one_trip_of_the_face_loops():
    meshes = C.face_trip_batch()
    off = C.face_offsets(meshes)
    trip = C.FACE_GRID_CAP * C.THREADS
    assert off[1] == 2_095_104 and off[1] < trip < off[2]
    v, f = meshes[1]
    _, t, _, ok = SR.sample_surface(v, f, 2048, 11, 1)
    assert ok and (off[1] + t < trip).any() and (off[1] + t >= trip).any()


@pytest.mark.parametrize("name", list(C.PAIR_CASES))
def test_pair_cases_need_their_later_trips(name):
    c = C.PAIR_CASES[name]
    assert C.pair_blocks(c["M"], c["P"]) == c["nb"] and -(-c["P"] // (c["nb"] * C.THREADS)) == c["trips"]
    assert c["P"] % (c["nb"] * C.THREADS) != 0                                          # a ragged last trip
    r = C.pair_rows(name)
    changed = (r["first"][:, 1:3] != r["full"][:, 1:3]).any(1)
    in_tail = (r["whole"][:, 1:3] != r["full"][:, 1:3]).any(1)
    assert np.array_equal(r["first"][:, [0, 3, 4, 5]], r["full"][:, [0, 3, 4, 5]])
    if c["M"] == 1:
        assert changed.all()
    else:
        assert changed.sum() * 4 >= c["M"] and in_tail.sum() >= 1, (changed.sum(), in_tail.sum())
    if name == "three_trips":
        assert c["M"] > 2 * C.THREADS - 1 and changed[C.THREADS:].any()                 # ms_final_kernel's second workgroup


def test_grid_cap_needs_many_points():
    """with 97 points 1 048 576 pairs exhaust every (i, j): the later trips could not change the row"""
    from cppf_amd import mesh_stats as MS
    idx = MS.stats_pairs(7, 0, C.PAIR_CASES["grid_cap"]["nb"] * C.THREADS, 97)
    assert np.unique(idx[:, 0] * 97 + idx[:, 1]).size == 97 * 97


# ------------------------------------------------------------------------------------------------ 3. block edges
def test_edge_meshes_reach_the_block_edges():
    meshes = C.edge_meshes()
    assert [f.shape[0] for _, f in meshes] == list(C.EDGE_FS)
    assert [-(-F // SR.LANES) for F in C.EDGE_FS] == [1, 1, 1, 1, 2, 2, 2, 3]
    first0 = [SR.areas(v, f)[0] == 0 for v, f in meshes]
    last0 = [SR.areas(v, f)[-1] == 0 for v, f in meshes]
    assert sum(first0) >= 3 and sum(last0) >= 2
    for n in C.EDGE_NS:
        for m, (v, f) in enumerate(meshes):
            _, t, E, ok = SR.sample_surface(v, f, n, 13, m)
            assert ok and E[-1] == n and np.array_equal(np.bincount(t, minlength=f.shape[0]), np.diff(np.concatenate([[0], E])))
            if n == 257 and f.shape[0] >= 1023:
                assert np.unique(t).size == 257
            a = SR.areas(v, f)
            assert (a[t] > 0).all()


# ------------------------------------------------------------------------------------------------ 4. exact arithmetic
def _exact_ints(a):
    """the float areas as integers over a common power of two"""
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    e0 = int(e[mi != 0].min())
    return [int(x) << (int(s) - e0) if x else 0 for x, s in zip(mi.tolist(), e.tolist())]


def _assert_counts_near_exact(v, f, n):
    """|E_t - N C*_t| <= 1/2 + N (K + 1024) 2^-52 for t < F - 1, C* the exact cumulative fraction of the float areas: one rounding
    to an integer, plus the worst-case rounding of a blocked sum of non-negative terms (K terms inside a block, 1024 block totals,
    for the total and again for the cumulative sum)"""
    a = SR.areas(v, f)
    F = a.shape[0]
    K = -(-F // SR.LANES)
    E = SR.counts_end(SR.blocked_cumsum(a / SR.blocked_total(a)), n)
    ints = _exact_ints(a)
    cum = np.array(list(itertools.accumulate(ints)), dtype=object)
    tot = int(cum[-1])
    # times tot 2^53:  |E tot - N cum| 2^53 <= tot (2^52 + 2 N (K + 1024))
    lhs = np.abs(np.array(E.tolist(), dtype=object) * tot - n * cum) * (1 << 53)
    rhs = tot * ((1 << 52) + 2 * n * (K + SR.LANES))
    assert (lhs[:F - 1] <= rhs).all(), (F, n, int(np.argmax(lhs[:F - 1] > rhs)))
    assert E[-1] == n


def test_restated_counts_against_exact_arithmetic():
    for i, case in enumerate(C.DIP_CASES):
        v, f, _, _ = C.dip_case(i)
        _assert_counts_near_exact(v, f, case["N"])
    for v, f in C.face_trip_batch():
        _assert_counts_near_exact(v, f, 2048)
    for v, f in C.edge_meshes():
        for n in C.EDGE_NS:
            _assert_counts_near_exact(v, f, n)
    for (v, f), word in zip(C.status_batch(), C.STATUS_WORDS):
        if word == 0 and np.isfinite(v).all():
            _assert_counts_near_exact(v, f, 2048)


# ------------------------------------------------------------------------------------------------ 5. status legs
def test_status_words_of_the_restatement():
    meshes = C.status_batch()
    assert [SR.sample_status(v, f) for v, f in meshes] == C.STATUS_WORDS == [0, 3, 3, 1, 1, 0, 0]
    v, f = meshes[1]
    assert f.min() == -1 and meshes[2][1].max() == v.shape[0]
    v, f = meshes[3]
    assert np.isnan(v).sum() == 1 and np.isnan(SR.areas(v, f)).any()
    v, f = meshes[4]
    with np.errstate(over="ignore", invalid="ignore"):
        assert not np.isfinite(SR.areas(v, f)).all() and np.isfinite(v).all()
    v, f = meshes[5]
    assert not np.isfinite(v[-1]).all() and f.max() < v.shape[0] - 1                    # not referenced
    for (v, f), word in zip(meshes, C.STATUS_WORDS):
        pts, t, _, ok = SR.sample_surface(v, f, 64, 17, 0)
        assert ok == (word == 0) and np.isnan(pts).all() == (word != 0) and (t == -1).all() == (word != 0)


@pytest.mark.parametrize("N", C.BAD_NS)
def test_bad_point_sets_hold_one_bad_coordinate(N):
    pts, status = C.bad_point_batch(N)
    assert pts.shape[1:] == (N, 3) and status[0] == status[-1] == 0 and sum(status) == 3 * len({a % N for a in C.BAD_AT if -N <= a < N})
    bad = ~np.isfinite(pts)
    assert bad.reshape(len(status), -1).sum(1).tolist() == status
    assert set(np.flatnonzero(bad.any((0, 2))).tolist()) == {a % N for a in C.BAD_AT if -N <= a < N}
