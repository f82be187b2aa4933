"""The conditions of tests/scene_limits_cases.py without a device: from the restatements alone, every case reaches the loop trip,
the cap or the guard it is named for -- what tests/test_gpu_scene_limits.py relies on -- and the refusals of cppf_gather_instances
and cppf_depth_segments that are decided on the host leave poisoned outputs alone."""
import numpy as np
import pytest

import instances_ref as IR
import scene_limits_cases as C
import scene_training_ref as TR
import segments_ref as SR
from cppf_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3


# ------------------------------------------------------------------------------------------------ A. instance gather
def test_gather_edge_sizes_straddle_a_wave_and_a_chunk():
    assert {m - 64 for m in C.EDGE_MS[:3]} == {m - C.CHUNK for m in C.EDGE_MS[3:]} == {-1, 0, 1}
    assert [-(-m // C.CHUNK) for m in C.EDGE_MS] == [1, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("K", C.FAR_KS)
@pytest.mark.parametrize("M", C.FAR_MS)
def test_gather_far_cases_fill_the_second_trip_of_the_table_sum(M, K):
    want, total = C.gather_far_ref(M, K)
    table = IR.chunk_counts_ref(want["member"], K, C.CHUNK)
    n_chunks = table.shape[1]
    assert n_chunks == -(-M // C.CHUNK) and not want["bad"] and table.sum() == total == want["offsets"][K]
    assert [-(-K // C.GI_WAVES), K % C.GI_WAVES] in ([1, 0], [2, 1], [2, 0])        # one trip of the row loop, a ragged second, two full
    if M == C.FAR_MS[0]:
        assert n_chunks == C.TABLE_LANES                                            # exactly one full trip: no column 64
        return
    assert n_chunks > C.TABLE_LANES and M - 1 >= C.FAR_START
    near, far = table[:, :C.TABLE_LANES].sum(-1), table[:, C.TABLE_LANES:].sum(-1)
    both = [k for k in range(K) if k not in C.far_rows(K) and k != C.NEAR_ONLY_ROW]
    assert (near[both] > 0).all() and (far[both] > 0).all()
    assert (table[both][:, C.TABLE_LANES:] > 0).all()                               # every column >= 64 of those rows is populated
    assert C.far_rows(K) and all(near[r] == 0 and far[r] > 0 for r in C.far_rows(K))
    assert near[C.NEAR_ONLY_ROW] > 0 and far[C.NEAR_ONLY_ROW] == 0
    if K > C.GI_WAVES:                                                              # the rows of the second trip of the row loop
        late = [k for k in both if k >= C.GI_WAVES]
        assert late and (table[late][:, C.TABLE_LANES:] > 0).all() and (near[late] > 0).all()
        assert K == 17 or any(r >= C.GI_WAVES for r in C.far_rows(K))
    # a workgroup >= 64 places its rows behind the members of chunks 0..63: dropping the second trip moves every such row
    src = want["src"][:total]
    assert (src >= C.FAR_START).sum() == far.sum() > 0
    # one row short: the last row is a point of the last chunk
    assert src[-1] // C.CHUNK == n_chunks - 1


def test_gather_bad_owner_positions_lie_in_chunk_64_and_in_the_last_chunk():
    M = C.FAR_MS[2]
    assert -(-M // C.CHUNK) == 66
    assert (C.FAR_START + 5) // C.CHUNK == 64 and (M - 1) // C.CHUNK == 65 and C.FAR_MS[1] - 1 == C.FAR_START
    hi, nrm, owner, masks = C.gather_far_case(M, 17)
    for where in (C.FAR_START + 5, M - 1):
        bad = owner.copy()
        bad[where] = C.N_SPARSE
        assert IR.gather_ref(hi, nrm, bad, masks, capacity=4)["offsets"].tolist() == [0] * 17 + [-1]


def test_gather_cap_case_is_at_the_cap():
    hi, nrm, owner, masks = C.gather_cap_case()
    M = hi.shape[0]
    assert M == C.MAX_CHUNKS * C.CHUNK == 8388608 and -(-M // C.CHUNK) == C.MAX_CHUNKS and -(-(M + 1) // C.CHUNK) == C.MAX_CHUNKS + 1
    assert np.isfinite(hi).all() and np.isfinite(nrm).all() and hi.min() >= 0.5 and np.unique(hi[::4099].view(np.uint32)).size == hi[::4099].size
    g = IR.gather_ref(hi, nrm, owner, masks, capacity=64)
    T = int(g["offsets"][1])
    assert 20 <= T <= 64 and g["src"][0] == 0 and g["src"][T - 1] == M - 1 and C.FAR_START in g["src"] and C.CHUNK in g["src"]
    has = owner >= 0
    assert has.sum() > T and np.array_equal(np.nonzero(g["member"])[0], g["src"][:T])


def _host_gather(M, K, out):
    """cppf_gather_instances on host buffers (the call must be refused before anything is launched)"""
    buf = np.zeros(64, np.int32)
    p, o = buf.ctypes.data, [a.ctypes.data for a in out]
    return _lib.lib().cppf_gather_instances(p, p, p, p, K, 4, M, 4, o[0], o[1], o[2], o[3], o[4], p, None)


def test_gather_refusals_at_the_caps_leave_the_outputs_alone():
    """8193 chunks: CPPF_EUNSUPPORTED; n_dense n_props > INT32_MAX: CPPF_EINVAL; the largest acceptable sizes pass the wrapper's
    mirror of the checks.  Decided on the host: the outputs are host arrays, still poison afterwards."""
    from cppf_amd import scene_stage
    out = [np.full(64, IR.POISON_I, np.int32) for _ in range(5)]                    # member, offsets, pts, nrm, src
    assert _host_gather(C.CAP_M + 1, 1, out) == EUNSUPPORTED == _lib.EUNSUPPORTED
    assert _host_gather(C.CAP_M + C.CHUNK, 1, out) == EUNSUPPORTED
    for M, K in [((2 ** 31 - 1) // 32 + 1, 32), (2 ** 30, 2), (2 ** 31 - 1, 2)]:
        assert M * K > 2 ** 31 - 1 >= M and _host_gather(M, K, out) == EINVAL, (M, K)
    assert all((a == IR.POISON_I).all() for a in out)
    scene_stage.check_gather_args(1, 4, C.CAP_M, 4)
    scene_stage.check_gather_args(32, 4, C.CAP_M, 4)                                 # 2^28 rows: inside the int32 offsets
    with pytest.raises(ValueError, match="at most"):
        scene_stage.check_gather_args(1, 4, C.CAP_M + 1, 4)
    with pytest.raises(ValueError, match="int32"):
        scene_stage.check_gather_args(32, 4, (2 ** 31 - 1) // 32 + 1, 4)


# ------------------------------------------------------------------------------------------------ B. depth segments
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_segment_counts_around_the_cap(n):
    d = C.cap_image(n)
    w = SR.segments_ref(d, min_pixels=1, capacity=C.SEG_MAX)
    assert w["counts"].tolist() == [n, n, n, 0] and w["overflow"] == (n > C.SEG_MAX)
    if n <= C.SEG_MAX:
        assert (w["sizes"][:n] == 1).all() and (w["first"][n:] == -1).all() and (w["first"] >= 0).sum() == n
        assert np.array_equal(np.sort(w["labels"][d > 0]), np.arange(n))
    else:
        assert (w["labels"] == -1).all() and (w["first"] == -1).all() and not w["sizes"].any() and (w["comp_size"][d > 0] == 1).all()


@pytest.mark.parametrize("n_kept", [256, 257])
def test_staging_images_interleave_kept_and_dropped_roots(n_kept):
    d = C.staging_image(n_kept)
    assert d.shape[1] == C.STAGING_WIDTH and d.shape[1] % 64
    w = SR.segments_ref(d, capacity=C.SEG_MAX, **C.STAGING_FILTER)
    S, n_comp = int(w["counts"][0]), int(w["counts"][1])
    assert S == n_kept and n_comp > S + 100 and not w["overflow"]
    assert (n_kept > C.SEG_STAGE) == (n_kept == 257)                                # the staging loop's second trip holds one entry
    flat, size = w["labels"].reshape(-1), w["comp_size"].reshape(-1)
    live = d.reshape(-1) > 0
    assert not (live[:-d.shape[1]] & live[d.shape[1]:]).any()                       # no two live pixels above each other
    roots = np.nonzero(live & ((np.arange(d.size) % d.shape[1] == 0) | ~np.roll(live, 1)))[0]
    assert roots.shape[0] == n_comp                                                 # (a component is a run along a row: it starts at its root)
    kept = flat[roots] >= 0
    assert kept.sum() == S and np.array_equal(roots[kept], w["first"][:S])
    assert set(size[roots[~kept]].tolist()) == {2, 7} and set(size[roots[kept]].tolist()) == {3, 4, 5, 6}
    assert np.abs(np.diff(kept.astype(int))).sum() > 100                            # kept and dropped roots alternate over 100 times
    ordinal = np.nonzero(kept)[0]                                                   # a kept root's ordinal among ALL roots ...
    assert (ordinal[S // 2:] > np.arange(S)[S // 2:] + 50).all() and ordinal[-1] != S - 1      # ... is far from its rank
    assert flat[w["first"][S - 1]] == S - 1 and (flat == S - 1).sum() == w["sizes"][S - 1]      # the last entry labels its pixels


def test_link_rule_at_the_ends_of_the_ranges():
    for row, tol, slope, comps in C.LINK_ENDS:
        assert max(row) <= 65535 and 0 <= tol <= 65535 and 0 <= slope <= 1000
        w = SR.segments_ref(np.array([row], np.uint16), tol_mm=tol, slope_permille=slope, min_pixels=1)
        f = SR.flood_ref(np.array([row], np.uint16), tol_mm=tol, slope_permille=slope, min_pixels=1)
        assert w["counts"][1] == f["counts"][1] == comps, (row, tol, slope)
    assert {max(r) for r, *_ in C.LINK_ENDS} >= {65535} and {t for _, t, *_ in C.LINK_ENDS} >= {65535} and 1000 * 65535 < 2 ** 31
    assert -(-C.LONG_ROW // 64) == 1025 and C.LONG_ROW % 64 == 1
    w = SR.segments_ref(np.full((1, C.LONG_ROW), 1000, np.uint16), min_pixels=1)
    assert w["counts"].tolist() == [1, 1, C.LONG_ROW, 0] and w["sizes"][0] == C.LONG_ROW


def test_segment_refusals_leave_the_outputs_alone():
    """H W = 2^24 + 1, capacity 1025, slope 1001, tol 65536, min_pixels 0: CPPF_EINVAL each, decided on the host -- the five output
    arrays (host memory here) are still poison; the values one step inside are accepted by the wrapper's mirror of the checks"""
    from cppf_amd import segments as SG
    L = _lib.lib()
    buf = np.zeros(64, np.int16)
    out = [np.full(64, -77, np.int32) for _ in range(5)]                            # labels, comp_size, first, sizes, counts
    good = dict(H=1, W=4, tol=10, slope=10, mn=1, mx=0, cap=4)
    for key, value in C.SEG_REFUSALS:
        a = dict(good, **{key: value})
        rc = L.cppf_depth_segments(buf.ctypes.data, None, a["H"], a["W"], a["tol"], a["slope"], a["mn"], a["mx"], a["cap"],
                                   *[o.ctypes.data for o in out], None)
        assert rc == EINVAL, (key, value)
        with pytest.raises(ValueError):
            SG.check_segment_args(a["H"], a["W"], a["tol"], a["slope"], a["mn"], a["mx"], a["cap"])
    assert all((o == -77).all() for o in out)
    assert {k for k, _ in C.SEG_REFUSALS} == {"W", "cap", "slope", "tol", "mn"}
    SG.check_segment_args(1, C.SEG_PIXELS_MAX, 65535, 1000, 1, 0, C.SEG_MAX)


# ------------------------------------------------------------------------------------------------ C. plane RANSAC
@pytest.mark.parametrize("N", C.PLANE_NS)
def test_plane_clouds_have_inliers_of_the_best_plane_in_the_tail(N):
    """the best plane's count over all N points is larger than over the points in front of the last 65: a second (third) trip that
    was dropped, or a straddling wave that was left out, changes best[1]"""
    pts = C.plane_case(N)
    assert pts.shape == (N, 3) and N >= C.PR_TRIP and (N - C.PR_TRIP) % C.PR_TRIP in (0, 1, 65)
    planes = SR.planes_ref(pts, C.PLANE_HYP, seed=N)
    counts = SR.counts_ref(pts, planes, C.PLANE_THRESH)
    best = SR.best_ref(planes, counts)
    assert best[0] >= 0 and best[1] > 0.5 * N
    head = SR.counts_ref(pts[:N - C.PLANE_TAIL], planes[best[0]:best[0] + 1], C.PLANE_THRESH)[0]
    assert 10 <= best[1] - head <= C.PLANE_TAIL
    if N > C.PR_TRIP:                                                               # and in the later trips alone
        trip = SR.counts_ref(pts[:(N - 1) // C.PR_TRIP * C.PR_TRIP], planes[best[0]:best[0] + 1], C.PLANE_THRESH)[0]
        assert trip < best[1]
    runner_up = np.sort(counts)[-2] if (counts == best[1]).sum() == 1 else best[1]
    print(f"N = {N}: best {best.tolist()}, without the tail {head}, runner-up {runner_up}")


# ------------------------------------------------------------------------------------------------ D. the draw
def _draw_loop(members, cap, seg_off, n_inst, inst, n_points, P, n_pos, seed):
    """st_draw_kernel line by line (a Python loop over the pairs); negative or too large an index raises instead of wrapping"""
    def at(arr, j):
        assert 0 <= j < len(arr), j
        return int(arr[j])
    p = np.arange(P, dtype=np.uint64)
    w = TR.syn.philox4x32_10([p, 0 * p, 0 * p + np.uint64(TR.STREAM), 0 * p], seed)
    out = []
    for q in range(P):
        wx, wy = int(w[0][q]), int(w[1][q])
        a, b = (wx * n_points) >> 32, (wy * n_points) >> 32
        M = at(seg_off, n_inst)
        if q < n_pos and 0 < M <= cap:
            am = at(members, (wx * M) >> 32)
            if 0 <= am < n_points:
                k = at(inst, am)
                if 0 <= k < n_inst:
                    s0, s1 = at(seg_off, k), at(seg_off, k + 1)
                    if s0 >= 0 and s1 > s0 and s1 <= M:
                        a, b = am, at(members, s0 + ((wy * (s1 - s0)) >> 32))
        out.append((a, b))
    return np.array(out, np.int32).reshape(P, 2)


def test_lenient_draw_equals_the_plain_draw_on_well_formed_lists():
    c = C.draw_case(None)
    m, s, i = C.draw_views(c)
    for n_pos in (0, 100, C.DRAW_P):
        idx, kept = TR.draw_ref_lenient(m, c["cap"], s, i, C.DRAW_N, C.DRAW_P, n_pos, C.DRAW_SEED)
        assert not kept.any() and np.array_equal(idx, TR.draw_ref(m[:c["M"]], s, i, C.DRAW_N, C.DRAW_P, n_pos, C.DRAW_SEED))
    assert s[2] == s[1] and s[0] == 0 and s[C.DRAW_K] == c["M"] > 100 and np.all(np.diff(s) >= 0)


@pytest.mark.parametrize("name", C.DRAW_BREAKS)
def test_each_broken_promise_reaches_its_guard(name):
    c = C.draw_case(name)
    m, s, i = C.draw_views(c)
    P, N, K, M = C.DRAW_P, C.DRAW_N, C.DRAW_K, c["M"]
    idx, kept = C.draw_want(name)
    assert np.array_equal(idx, _draw_loop(m, c["cap"], s, K, i, N, P, P, C.DRAW_SEED))
    good = C.draw_want(None)[0]                                                     # the well-formed lists' draw
    uniform = TR.draw_ref_lenient(m, c["cap"], s, i, N, P, 0, C.DRAW_SEED)[0]       # every pair uniform
    assert np.array_equal(idx[kept], uniform[kept]) and kept.any()
    assert (uniform[kept] != good[kept]).any(-1).sum() > 0.9 * kept.sum()           # (keeping the uniform draw shows)
    if name == "cap":
        assert kept.all() and s[K] == c["cap"] + 1                                  # M > members_cap spares nobody: the whole stratum
        return
    assert (~kept).any() and kept.sum() >= 20 and (~kept).sum() >= 20
    # the junk around the arrays is in range: a guard that failed would have read a point, an offset or a label
    mb, sb, ib = c["members_buf"], c["seg_buf"], c["inst_buf"]
    outside = lambda buf, off, n: np.concatenate([buf[:off], buf[off + n:]])
    assert outside(mb, C.M_OFF, M).min() >= 0 and outside(mb, C.M_OFF, M).max() < N and min(C.M_OFF, C.S_OFF, C.I_OFF) >= 1
    assert outside(sb, C.S_OFF, K + 1).min() >= 0 and outside(sb, C.S_OFF, K + 1).max() <= M
    assert outside(ib, C.I_OFF, N).min() >= 0 and outside(ib, C.I_OFF, N).max() < K
    # the unaffected pairs: the well-formed draw, but for b where the drawn position holds an altered member
    same_b = idx[~kept, 1] == good[~kept, 1]
    assert np.array_equal(idx[~kept, 0], good[~kept, 0])
    if c["bad"] is None:
        assert same_b.all()
    else:
        assert (idx[~kept, 1][~same_b] == c["bad"]).all() and same_b.sum() > 0.5 * same_b.size
    # ... and each case breaks what it says
    base = C.draw_views(C.draw_case(None))
    changed = [not np.array_equal(m[:M], base[0][:M]), not np.array_equal(s, base[1]), not np.array_equal(i, base[2])]
    want = dict(member_n=[1, 0, 0], member_neg=[1, 0, 0], empty_seg=[1, 0, 0], label_K=[0, 0, 1], label_neg=[0, 0, 1], seg_neg=[0, 1, 0],
                seg_past_M=[0, 1, 0])[name]
    assert changed == [bool(v) for v in want]
    if name == "member_n":
        assert (m[:M] == N).sum() >= 20
    if name == "label_K":
        assert (i == K).sum() >= 20
    if name == "label_neg":
        assert (i[base[0][:M]] == -1).sum() >= 20
    if name == "seg_neg":
        assert s[2] == -1 and set(base[2][idx[~kept, 0]].tolist()) == {0, 3}
    if name == "seg_past_M":
        assert s[3] == M + 1 and s[K] == M and set(base[2][idx[~kept, 0]].tolist()) == {0}
    if name == "empty_seg":
        assert i[c["bad"]] == 1 and s[1] == s[2]


def test_draw_sizes_and_the_one_point_cloud():
    c = C.draw_case(None)
    m, s, i = C.draw_views(c)
    for P in (0, 255, 256):
        assert TR.draw_ref_lenient(m, c["cap"], s, i, C.DRAW_N, P, P, C.DRAW_SEED)[0].shape == (P, 2)
    idx, kept = TR.draw_ref_lenient([0], 1, [0, 1], [0], 1, 300, 150, 3)
    assert not idx.any() and not kept.any()


# ------------------------------------------------------------------------------------------------ D. the targets
def test_exact_scene_reaches_every_clamp_end_and_branch():
    s = C.exact_scene()
    fin = np.isfinite(s["pc"])
    assert np.array_equal(s["pc"][fin] * 4, np.round(s["pc"][fin] * 4)) and np.abs(s["pc"][fin]).max() < 16      # exact in fp32
    t = C.exact_want(3, 3)
    t64 = TR.targets_ref(s["pc"], s["nrm"], s["inst"], s["idx"], s["table"], s["flags"], C.EXACT_RANGE, 3, 3)
    heads = ("mu", "nu", "up", "right")
    seen = set()
    for p, (name, k) in enumerate(s["names"]):
        if name in C.EXACT_BY_HAND and k in (0, 1):
            assert t["kind"][p] == 1 and t["pair_inst"][p] == k, (name, k)
            for h, head in enumerate(heads):
                want = C.EXACT_BY_HAND[name][head]
                want = want[k] if h >= 2 else want
                assert (int(t["low"][p, h]), float(t["w_low"][p, h])) == want, (name, k, head)
            seen.add(name)
        else:                                                                       # another category, across instances, not finite
            assert t["kind"][p] == 0 and t["pair_inst"][p] == -1 and t["low"][p].tolist() == [0, 1, 0, 0], (name, k)
            assert t["w_low"][p].tolist() == [1, 0, 1, 1] and not t["aux"][p].any()
            assert name in ("across", "nan_a", "nan_b", "inf_a", "inf_b") or k == 2
    assert seen == set(C.EXACT_BY_HAND)
    assert np.array_equal(t["kind"], t64["kind"])                                   # fp64 agrees on who is a positive
    # the unclamped values, in fp64: below 0 / above 2 v0, on both ends, above v1 and on it; cos = +-1
    v0, v1 = C.EXACT_RANGE
    a = s["pc"].astype(np.float64)[s["idx"][:, 0]] - s["table"].astype(np.float64)[np.maximum(s["inst"][s["idx"][:, 0]], 0), :3]
    b = s["pc"].astype(np.float64)[s["idx"][:, 1]] - s["table"].astype(np.float64)[np.maximum(s["inst"][s["idx"][:, 1]], 0), :3]
    row = {n: p for p, (n, k) in enumerate(s["names"]) if k == 0}
    with np.errstate(invalid="ignore"):
        u = (a - b) / np.maximum(np.linalg.norm(a - b, axis=-1, keepdims=True), 1e-300)
        proj = (a * u).sum(-1)
        dist = np.linalg.norm(a - proj[:, None] * u, axis=-1)
    assert proj[row["mu_above"]] + v0 > 2 * v0 and proj[row["mu_below"]] + v0 < 0
    assert proj[row["mu_at_0"]] + v0 == 0 and proj[row["mu_at_top"]] + v0 == 2 * v0
    assert dist[row["nu_above"]] > v1 and dist[row["nu_at_top"]] == v1
    assert u[row["mu_above"], 1] == 1 and u[row["mu_below"], 1] == -1 and u[row["right_par"], 0] == 1 and u[row["right_anti"], 0] == -1
    assert np.all(a[row["coincident"]] == b[row["coincident"]])
    # |a - b| + 1e-7 rounds to |a - b| in fp32 and not in fp64: why the restatement runs in fp32 here
    assert np.float32(2) + np.float32(1e-7) == np.float32(2) and 2.0 + 1e-7 != 2.0
    # aux: the normal is turned to u's side first
    assert t["aux"][row["mu_above"]].tolist() == [1, 0] and t["aux"][row["mu_below"]].tolist() == [0, 0]
    assert t["aux"][row["mu_at_0"]].tolist() == [0, 1] and t["aux"][row["right_par"]].tolist() == [1, 0]
    p = row["nu_at_top"]
    assert (s["nrm"][s["idx"][p, 0]] * u[p]).sum() < 0 and t["aux"][p].tolist() == [1, 0]      # turned: n.up = -1 became + 1
    # two bins: every index is 0 and the weight carries everything
    t2 = C.exact_want(2, 2)
    pos = t2["kind"] == 1
    assert np.array_equal(t2["kind"], t["kind"]) and not t2["low"].any() and set(np.unique(t2["w_low"][pos]).tolist()) == {0.0, 0.5, 1.0}


@pytest.mark.parametrize("tr_bins,rot_bins", [(2, 2), (256, 256)])
def test_scene3_at_the_ends_of_the_bin_range(tr_bins, rot_bins):
    """the restatement of test_gpu_scene_training.py's scene at 2 and 256 bins: in range, both bins of a head carry weight, and at
    256 bins every head reaches an index above 127 (a byte that a signed read would turn negative)"""
    from test_gpu_scene_training import scene3_case
    s = scene3_case(tr_num_bins=tr_bins, rot_num_bins=rot_bins)
    t, pos = s["t64"], s["pos"]
    assert pos.sum() > 500 and s["cfg"].tr_num_bins == tr_bins and s["cfg"].rot_num_bins == rot_bins
    top = np.array([tr_bins - 2] * 2 + [rot_bins - 2] * 2)
    assert (t["low"] >= 0).all() and (t["low"] <= top).all() and (t["w_low"] >= 0).all() and (t["w_low"] <= 1).all()
    assert (t["w_low"][pos].min(0) < 0.5).all() and (t["w_low"][pos].max(0) > 0.5).all()
    assert (t["low"][pos].max(0) > 127).all() if tr_bins == 256 else not t["low"][pos].any()
    assert (t["low"][~pos] == [0, tr_bins - 2, 0, 0]).all()
    assert 0 < s["dev_tr"] < 1e-3 and 0 < s["dev_rot"] < 1e-3
