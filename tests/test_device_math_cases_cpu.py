"""CPU side of the device-arithmetic tests (tests/test_gpu_device_math.py): the case families of tests/device_math_cases.py are what
their docstrings say, the oracle's exp2w / sincos / rot_cs / tan meet the bounds the device is held to (so "same bits as the oracle"
plus these bounds is a statement about the device), and the numpy restatement of bv_arc has both properties the device must have on
the generated tuples -- and loses rotations once its load-bearing slack terms are set to zero.  No GPU."""
import os
import re

import numpy as np
import pytest

import device_math_cases as DM

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def has(x, v):
    """v (bit pattern and all: -0 is not +0) occurs in the float32 array x"""
    return bool((DM.bits(x) == DM.bits(np.array([v], F))[0]).any())


# ------------------------------------------------------------------------------------ the families
def test_fma32_is_the_correctly_rounded_fma():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = DM.from_bits(rng.integers(0x30000000, 0x4F000000, 4000).astype(np.uint32))
    b = DM.from_bits(rng.integers(0x30000000, 0x4F000000, 4000).astype(np.uint32))
    c = -(a.astype(D) * b.astype(D) * (1 + rng.uniform(-1e-7, 1e-7, 4000))).astype(F)      # cancellation: the sum's low bits matter
    c[:100] = 0
    got = DM.fma32(a, b, c)
    for i in range(4000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = float(np.nextafter(got[i], F(-np.inf))), float(np.nextafter(got[i], F(np.inf)))
        g = Fraction(float(got[i]))
        assert abs(exact - g) <= abs(exact - Fraction(lo)) and abs(exact - g) <= abs(exact - Fraction(hi))


def test_division_families_stay_in_their_stated_domains():
    p = DM.div_ppf()
    assert not np.isnan(p["a"]).any() and (np.abs(p["a"]) <= p["d"]).all()
    assert p["den"].min() == F(1e-7) and p["den"].max() <= F(2.0) + F(1e-7) and has(p["d"], 0.0)
    d = np.unique(p["d"])
    for e in range(-30, 1):
        for m in DM.EDGE_MANT:
            assert has(d, DM.from_bits(np.array([((e + 127) << 23) | m], np.uint32))[0])
        assert ((d >= 2.0 ** e) & (d < 2.0 ** (e + 1))).sum() == 5 + 64
    for v in np.unique(p["d"])[[1, 100, -1]]:                                   # the numerators of one distance
        a = p["a"][p["d"] == v]
        assert has(a, v) and has(a, -v) and has(a, DM.TINY) and has(a, -DM.TINY) and has(a, 0.0) and a.size == 7 + 16
    for l_max in (4.0, 1.0):
        q = DM.div_pair_frame(l_max)
        assert not np.isnan(q["a"]).any() and (np.abs(q["a"]) <= q["d"]).all()
        assert q["d"].astype(D).min() >= 1e-7 and float(np.nextafter(q["d"].min(), F(0))) < 1e-7 and q["d"].max() == F(l_max)
        assert (q["den"] == (q["d"].astype(D) + 1e-7).astype(F)).all()
    v = DM.div_vote()
    res = DM.vote_res()
    from cppf_amd.config import CATEGORIES
    assert all(has(res, F(c.res)) for c in CATEGORIES.values()) and all(has(res, F(r)) for r in DM.DIV_CHECK_RES) and res.size == 13
    assert np.abs(v["a"]).min() == F(2.0 ** -40) and np.abs(v["a"]).max() < F(2.0 ** 7) and (v["a"] < 0).sum() * 2 == v["a"].size
    assert v["a"].size == res.size * 47 * (5 + 32) * 2 <= 1 << 21


def test_sqrt_families():
    x = DM.sqrt_in_range()
    assert has(x, 0.0) and has(x, F(2.0 ** -96)) and has(x, F(2.0 ** 40)) and not np.isnan(x).any() and (x >= 0).all()
    for e in (-96, -1, 0, 39):
        for m in DM.EDGE_MANT:
            assert has(x, DM.from_bits(np.array([((e + 127) << 23) | m], np.uint32))[0])
    for k in (1.0, 3.0, 4096.0):
        assert has(x, F(k * k)) and has(x, np.nextafter(F(k * k), F(0))) and has(x, np.nextafter(F(k * k), F(np.inf)))
    lo = DM.sqrt_below_range()
    assert (lo > 0).all() and (lo < F(2.0 ** -96)).all() and has(lo, DM.TINY)
    r = DM.inv_sqrt()
    assert r.min() == F(2.0 ** -20) and r.max() == F(2.0 ** 20) and has(r, F(1e-5)) and has(r, F(1) + F(1e-5)) and has(r, F(1e4) + F(1e-5))


def test_exp2_family_reaches_its_edges():
    c = DM.exp2w()
    y = c["y"]
    assert not np.isnan(y).any() and y.min() >= -1500 and c["l"].size <= 1 << 21
    for v in range(-200, 3):
        assert has(y, F(v)) and has(y, np.nextafter(F(v), F(-np.inf))) and has(y, np.nextafter(F(v), F(np.inf)))
    assert has(y, -0.0) and has(y, 0.0) and has(y, -DM.TINY) and has(y, -F(2.0 ** -25))
    assert ((y >= -150) & (y <= -125)).sum() >= 1 << 13
    real = c["kind"] == 4
    assert real.sum() == 16 * 1024 and (y[real] <= F(1e-5)).all()                   # y <= 0 up to the rounding of the product
    first = np.nonzero(real)[0][::1024]
    assert (np.abs(y[first]) <= 1e-5).all()                                      # the row maximum: weight ~ 1
    assert y[real].min() < -1400                                                  # spread 1000: far below the last subnormal


def test_trig_families():
    x = DM.sincos_x()
    assert np.abs(x).max() <= 2 * np.pi + 1e-15 and not np.isnan(x).any()
    for k in range(-8, 9):
        q = k * (np.pi / 4)
        assert (x == q).any() and (x == np.nextafter(q, -np.inf)).any() and (x == np.nextafter(q, np.inf)).any()
    i, n = DM.rot_pairs()
    assert i.size == sum(k + 1 for k in range(1, 361)) and n.min() == 1 and n.max() == 360 and ((i >= 0) & (i <= n)).all()
    assert ((i == n).sum(), (i == 0).sum()) == (360, 360)
    t = DM.tan_x()
    h = np.nextafter(F(np.pi / 2), F(0))
    assert list(t[:6]) == [F(0), h, -h, F(-0.7), F(np.pi / 2), -F(np.pi / 2)] and np.abs(t).max() <= F(np.pi / 2)
    a = DM.atan01_x()
    assert a.min() == 0 and a.max() == 1 and has(a, DM.TINY) and not np.isnan(a).any() and a.size <= 1 << 21
    u = DM.acos_x()
    assert u.min() == -1 and u.max() == 1 and has(u, -0.0) and has(u, 0.0) and has(u, -DM.TINY) and has(u, DM.prev(F(1)))
    c = DM.atan2_yx()
    assert c["y"].size <= 1 << 21 and not np.isnan(c["y"]).any() and not np.isnan(c["x"]).any()
    zz = c["kind"] == 2
    pairs = {(float(np.copysign(1, a)) * (1 + abs(float(a))), float(np.copysign(1, b)) * (1 + abs(float(b)))) for a, b in zip(c["y"][zz], c["x"][zz])}
    assert len(pairs) == 4 + 4 + 4                                              # (+-0, +-0), (+-0, +-1), (+-1, +-0): signs told apart
    for m in DM.ATAN2_MAGS:
        diag = (c["kind"] == 3) & (np.abs(c["x"]) == F(m))
        assert (np.abs(c["y"][diag]) == F(m)).sum() == 4 and diag.sum() == 12
    mags = np.maximum(np.abs(c["x"]), np.abs(c["y"]))[c["kind"] == 0]
    assert mags.min() >= F(1e-30) * F(0.7) and mags.max() <= F(1e6) * F(1.0001)


def test_order_and_wave_families():
    s = DM.ordered_floats()
    assert (np.diff(s.astype(D))[np.diff(s.astype(D)) != 0] > 0).all() and np.isinf(s[[0, -1]]).all()
    k = s.size // 2
    assert DM.bits(s)[k - 1] == 0x80000000 and DM.bits(s)[k] == 0                 # -0 right before +0
    keys = DM.f2ord_np(s)
    assert (np.diff(keys.astype(np.int64)) > 0).all()                            # the definition restated: a total order
    b = DM.random_bit_patterns()
    assert not np.isnan(DM.from_bits(b)).any() and b.size > (1 << 20) * 0.99
    ints, keys = DM.wave_blocks()
    assert ints.size == keys.size == 5 * 256 and (ints[512:768] == 7).all() and np.unique(keys[512:768]).size == 1
    w3, w4 = keys[768:1024].reshape(4, 64), keys[1024:].reshape(4, 64)
    assert (w3.argmax(1) == 0).all() and (w4.argmax(1) == 63).all()


def test_probe_shares_the_flag_lines_of_the_pair_kernels():
    """csrc/Makefile: the second build of the probe sits on the very target lists that give pair_mlp.o its additional flags, and both
    builds use the library's CXXFLAGS: the probe cannot be compiled under other flags than the kernels it stands for"""
    mk = open(os.path.join(ROOT, "cppf_amd", "csrc", "Makefile")).read()
    extra = [ln for ln in mk.splitlines() if re.match(r"^[^#\t].*:\s*CXXFLAGS\s*\+=", ln)]
    with_pair = [ln for ln in extra if re.search(r"\bpair_mlp\.o\b", ln.split(":")[0])]
    assert len(with_pair) == 3 and all("$(PROBE_NONANS)" in ln.split(":")[0] for ln in with_pair)
    assert not [ln for ln in extra if "$(PROBE_NONANS)" in ln.split(":")[0] and ln not in with_pair]
    assert mk.count("$(HIPCC) $(CXXFLAGS) -DPROBE_PREFIX=probe_nonans_ -c $< -o $@") == 1
    assert "math_probe" not in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)   # never part of libcppf_hip.so


# ------------------------------------------------------------------------------------ the oracle meets the bounds
@pytest.fixture(scope="module")
def rot_reference():
    i, n = DM.rot_pairs()
    ang = DM.rot_angles(i, n)
    ms, mc = DM.mp_sincos(ang.astype(D))
    return i, n, DM.mp_round_f32(mc), DM.mp_round_f32(ms)


def test_oracle_exp2w_within_its_stated_error(oracle):
    c = DM.exp2w()
    w = oracle.exp2w(c["l"], c["c"])
    assert (w[c["y"] == 0] == F(1.000002623)).all() and (c["y"] == 0).sum() >= 3      # p(0), for y = -0 as for +0
    y = c["y"].astype(D)
    normal = y >= -126
    ref = DM.mp_exp2(c["y"][normal])
    rel = np.abs(w[normal].astype(D) - ref) / ref
    print(f"orc_exp2w: max relative error {rel.max():.4g} on {normal.sum()} normal results")
    assert rel.max() <= 2.7e-6
    sub = (y < -126) & (y >= -150)
    exact = np.exp2(y[sub] - np.floor(y[sub])) * np.exp2(np.floor(y[sub]))       # (both factors exact to fp64 rounding; the product exact)
    assert (np.abs(w[sub].astype(D) - exact) <= 2.0 ** -150 + 2.7e-6 * exact).all()
    assert (w[y < -151] == 0).all() and (w >= 0).all()


def test_oracle_sincos_below_one_ulp(oracle):
    x = DM.sincos_x()
    sc = np.array([oracle.sincos(v) for v in x], D)
    ms, mc = DM.mp_sincos(x)
    es, ec = DM.mp_abs_err(sc[:, 0], ms), DM.mp_abs_err(sc[:, 1], mc)
    print(f"orc_sincos on [-2 pi, 2 pi]: max abs error sin {es.max() * 2.0 ** 53:.3f}, cos {ec.max() * 2.0 ** 53:.3f} x 2^-53")
    assert max(es.max(), ec.max()) <= 2.0 ** -52


def test_oracle_rot_cs_is_the_correctly_rounded_fp32(oracle, rot_reference):
    i, n, rc, rs = rot_reference
    got = np.array([oracle.rot_cs(int(a), int(b)) for a, b in zip(i, n)], F)
    miss = (DM.bits(got[:, 0]) != DM.bits(rc)) | (DM.bits(got[:, 1]) != DM.bits(rs))
    missed = {(int(a), int(b)) for a, b in zip(i[miss], n[miss])}
    print(f"orc_rot_cs: {len(missed)} of {i.size} (i, n) differ from the correctly rounded cos / sin: {sorted(missed)}")
    assert missed == set(DM.ROT_CS_BOUNDARY) and len(DM.ROT_CS_BOUNDARY) <= 1e-3 * i.size
    one_ulp = lambda a, b: np.abs(DM.f2ord_np(a).astype(np.int64) - DM.f2ord_np(b).astype(np.int64)) <= 1
    assert one_ulp(got[:, 0], rc).all() and one_ulp(got[:, 1], rs).all()


def test_oracle_tan_sign_branch(oracle):
    t = DM.tan_x()
    v = np.array([oracle.tanf(float(a)) for a in t], F)
    assert v[0] == 0 and v[1] > 1e7 and v[2] < -1e7 and v[4] < -1e7 and v[5] > 1e7      # float(pi/2) > pi/2: the tangent is negative
    dense = np.abs(t) < 1.5
    assert np.allclose(v[dense], np.tan(t[dense].astype(D)), rtol=2e-7, atol=0)


def test_numpy_restatements_of_the_approximations_meet_the_stated_bounds():
    x = DM.atan01_x()
    e01 = np.abs(DM.atan01_np(x).astype(D) - np.arctan(x.astype(D))).max()
    c = DM.atan2_yx()
    live = (c["x"] != 0) | (c["y"] != 0)
    e2 = np.abs(DM.atan2_np(c["y"], c["x"]).astype(D) - np.arctan2(c["y"].astype(D), c["x"].astype(D)))
    # (-0, x < 0): -pi where arctan2 gives -pi as well; (+0, x < 0): +pi
    u = DM.acos_x()
    ea = np.abs(DM.acos_np(u).astype(D) - np.arccos(u.astype(D))).max()
    print(f"numpy fp32 restatements: atan01 {e01:.3g}, atan2 {e2[live].max():.3g}, acos {ea:.3g}")
    assert e01 < 2e-5 and e2[live].max() < 1e-4 and ea < 1e-4


# ------------------------------------------------------------------------------------ bv_arc
@pytest.fixture(scope="module")
def arcs(oracle):
    c = DM.arc_tuples()
    return c, DM.arc_passing(oracle, c)


def test_arc_tuples_cover_the_regimes(arcs):
    c, S = arcs
    assert len(c["n"]) <= 1 << 21 and set(np.unique(c["n"])) == set(DM.ARC_NS)
    for k in ("cc", "gt", "x", "y", "tol", "L2", "w", "cmax"):
        assert np.isfinite(c[k]).all(), k
    x, y = c["x"].astype(D), c["y"].astype(D)
    nx, ny = np.linalg.norm(x, axis=-1), np.linalg.norm(y, axis=-1)
    assert (np.abs((x * y).sum(-1)) <= 1e-6 * nx * ny).all() and (np.abs(nx - ny) <= 3e-4 * nx).all()      # x _|_ y, |x| = |y| (1 - 1e-7 / L)
    assert (c["L2"] < F(1e-6)).sum() > 1000 and (c["L2"] >= F(1e-6)).sum() > 1000
    lo, cnt = DM.bv_arc_np(c)
    reg = DM.arc_regimes(c, cnt)
    print("bv_arc tuples:", len(c["n"]), reg, "with a passing rotation:", int(S.any(1).sum()))
    assert min(reg.values()) >= 400                                              # full scan, empty and proper arc all occur
    _, M = DM.arc_exact_span(c)
    assert (M == 0).sum() > 50 and ((M > 0) & (M < 1e-30)).sum() > 50 and (M > 1e-3).sum() > 1000
    edge = c["group"] == 1
    far = np.linalg.norm(c["gt"][edge].astype(D), axis=-1)                        # |cc| = 8.5, gt at most rho + tol = 0.32 further out
    assert far.min() > 8.0 and far.max() < 9.0
    assert c["tol"][edge].max() <= F(3 * 4e-3)
    assert (S.any(1) & edge).sum() > 1000 and (~S.any(1) & edge).sum() > 1000     # tol on both sides of the nearest sample's distance


def test_arc_restatement_is_a_superset_and_not_vacuous(arcs):
    c, S = arcs
    lo, cnt = DM.bv_arc_np(c)
    dropped = S & ~DM.arc_member(lo, cnt, c["n"], S.shape[1])
    assert dropped.sum() == 0
    alpha, M = DM.arc_exact_span(c)
    sel = (c["n"] >= 16) & (c["L2"] >= F(1e-6)) & (M > 1e-3) & ~(alpha > np.pi / 2)
    assert sel.sum() > 1000 and (cnt[sel] < c["n"][sel]).all()


@pytest.mark.parametrize("term", ["lower", "dc_scale"])
def test_arc_tuples_tell_the_load_bearing_slack_terms_from_zero(arcs, term):
    """Without the lowering of K, or without its (tol + dc) dc part alone, the restated screen loses passing rotations on these
    tuples: they reach the margins that decide.  (The 8e-4 rad and the index of margin cannot be told from zero by any input at
    n <= 360: floor / ceil alone leave at least one index = 2 pi / 360 = 1.7e-2 rad on either side, twenty times all the angular
    errors together -- those two terms only matter where the arc would come out EMPTY, which is what the lowering of K and the
    1.0005 cut prevent.)"""
    c, S = arcs
    lo, cnt = DM.bv_arc_np(c, **{term: 0.0})
    assert (S & ~DM.arc_member(lo, cnt, c["n"], S.shape[1])).any()
    for kw in (dict(slack=0.0), dict(margin=0.0)):
        lo, cnt = DM.bv_arc_np(c, **kw)
        assert not (S & ~DM.arc_member(lo, cnt, c["n"], S.shape[1])).any()
