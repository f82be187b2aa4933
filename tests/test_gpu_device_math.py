"""The shared device arithmetic (csrc/cppf_math.h, csrc/vote_common.h, csrc/backvote_common.h) held to the contracts its comments
state, on the device, one primitive at a time.  csrc/probe/math_probe.hip includes the three headers and maps each primitive over
arrays (libcppf_probe.so, built twice: default flags, symbols probe_*; pair_mlp.o's additional flags, symbols probe_nonans_*); the
inputs are the families of tests/device_math_cases.py; the references are numpy's IEEE fp32 operations, numpy fp64, mpmath at 120
bits and the oracle -- none of them the project's device code.  tests/test_device_math_cases_cpu.py holds the CPU half.
Run with -s for the measured worst cases (DESIGN.md section 4 quotes them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import device_math_cases as DM
from cppf_amd.models import voting
from cppf_amd._torch_util import stream_ptr

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cppf_amd", "csrc")
BUILDS = ("probe_", "probe_nonans_")
PI_F = F(3.14159265)


@pytest.fixture(scope="module")
def probe(dev):
    """libcppf_probe.so: the one in the tree when it is newer than what it is made of, else `make libcppf_probe.so`; no library is a
    failure, not a skip"""
    so = os.path.join(CSRC, "libcppf_probe.so")
    srcs = [os.path.join(CSRC, f) for f in ("cppf_math.h", "vote_common.h", "backvote_common.h", os.path.join("probe", "math_probe.hip"))]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        p = subprocess.run(["make", "-j8", "-C", CSRC, "libcppf_probe.so"], capture_output=True, text=True)
        assert p.returncode == 0, "libcppf_probe.so does not build:\n" + p.stdout[-2000:] + p.stderr[-4000:]
    lib = C.CDLL(so)

    class Probe:
        def __init__(self):
            self.dev = dev

        def dev_arr(self, a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        def call(self, build, name, *args):
            """tensors go as pointers, ints as int64, floats as float; the stream is the current one"""
            conv = []
            for a in args:
                if isinstance(a, torch.Tensor):
                    conv.append(C.c_void_p(a.data_ptr()))
                elif isinstance(a, (C.c_float, C.c_uint32, C.c_uint64, C.c_int)):
                    conv.append(a)
                else:
                    conv.append(C.c_int64(int(a)))
            rc = getattr(lib, build + name)(*conv, C.c_void_p(stream_ptr(dev)))
            assert rc == 0, f"{build}{name}: hip error {rc}"

        def map(self, build, name, ins, outs, n=None):
            """ins: numpy arrays; outs: dtypes (or (dtype, width)) -> numpy arrays of n elements"""
            n = len(ins[0]) if n is None else n
            d_in = [self.dev_arr(a) for a in ins]
            d_out = [torch.zeros((n,) + ((o[1],) if isinstance(o, tuple) else ()), dtype=(o[0] if isinstance(o, tuple) else o), device=dev) for o in outs]
            self.call(build, name, *d_in, *d_out, n)
            torch.cuda.synchronize(dev)
            res = [t.cpu().numpy() for t in d_out]
            return res[0] if len(res) == 1 else res

        def both(self, name, ins, outs, n=None):
            """the two builds must give the same bits; -> the default build's result"""
            a = self.map(BUILDS[0], name, ins, outs, n)
            b = self.map(BUILDS[1], name, ins, outs, n)
            for u, v in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
                assert u.tobytes() == v.tobytes(), f"{name}: the default and the -fno-honor-nans build differ"
            return a

        def sweep(self, build, name, *args):
            """-> (mismatches, smallest mismatching operand or None)"""
            out = torch.zeros(2, dtype=torch.int64, device=dev)
            self.call(build, name, *args, out)
            torch.cuda.synchronize(dev)
            bad, first = (int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().tolist())
            return bad, (None if first == 0xFFFFFFFFFFFFFFFF else first)

    return Probe()


def bits_equal(a, b):
    return DM.bits(a) == DM.bits(b)


def fbits(v):
    return int(DM.bits(np.array([v], F))[0])


# ------------------------------------------------------------------------------------ div_by / sqrt_rn / inv_sqrt_rn
@pytest.mark.parametrize("family", ["ppf", "pair_frame_ab", "pair_frame_xdir", "vote"])
def test_div_by_same_bits_as_ieee_division(probe, family):
    """every call site's operands (device_math_cases.div_*): div_by(a, b, refined_rcp(b)) == numpy's fp32 a / b, bit for bit, wherever
    the quotient is zero or a normal number.  The numerator -0 is not in these families: test_div_by_negative_zero_numerator.
    Found by this test on the MI355X and now stated in csrc/cppf_math.h: where the IEEE quotient is a non-zero SUBNORMAL (the
    numerator +-2^-149 of these families: |a / b| < 2^-126) div_by may be one subnormal quantum off -- its residuals are not
    representable there, which is what the compiler's operand scaling is for.  Some hundred of the 49 243 PPF operands, all with
    |a| = 2^-149 (the count is printed); pinned below as "at most 2^-149 away", never further."""
    c = {"ppf": DM.div_ppf, "pair_frame_ab": DM.div_pair_frame, "pair_frame_xdir": lambda: DM.div_pair_frame(1.0, seed=22), "vote": DM.div_vote}[family]()
    assert (DM.bits(c["a"]) != 0x80000000).all()
    q = probe.both("div_by", [c["a"], c["den"]], [torch.float32])
    ref = (c["a"] / c["den"]).astype(F)
    bad = ~bits_equal(q, ref)
    sub = DM.subnormal_quotient(c["a"], c["den"])
    print(f"div_by[{family}]: {c['a'].size} quotients, {(bad & ~sub).sum()} differ from a / b; of the {sub.sum()} subnormal quotients {(bad & sub).sum()} differ, "
          f"by at most {np.abs(q[sub].astype(D) - ref[sub].astype(D)).max() / 2.0 ** -149 if sub.any() else 0:.0f} quanta")
    bad &= ~sub
    assert not bad.any(), [(float(a), float(b), float(x), float(y)) for a, b, x, y in zip(c["a"][bad][:5], c["den"][bad][:5], q[bad][:5], ref[bad][:5])]
    assert (np.abs(q[sub].astype(D) - ref[sub].astype(D)) <= 2.0 ** -149).all()
    assert (np.abs(c["a"][sub]) < F(2.0 ** -120)).all()                           # only numerators no metric cloud holds


def test_div_by_negative_zero_numerator(probe):
    """The one documented exception: div_by(-0, b) is +0 where IEEE gives -0.  It cannot be reached through a difference of equal
    coordinates -- sub3(p, p) is +0 in every component for every sign and size of the coordinate -- which is what every numerator
    of div_by is made from; so the exclusion is a stated one, not a silent one."""
    den = np.concatenate([DM.vote_res(), [F(1e-7), F(1.0), F(2.0) + F(1e-7)]]).astype(F)
    q = probe.both("div_by", [np.full(den.size, -0.0, F), den], [torch.float32])
    assert (DM.bits(q) == 0).all()                                               # +0, not the -0 of (-0.0 / den)
    assert (DM.bits((np.full(den.size, -0.0, F) / den).astype(F)) == 0x80000000).all()
    v = np.array([0.0, -0.0, 1.5, -2.0, 8.5, -1e-30, DM.TINY, -DM.TINY, 3e38, -3e38], F)
    p = np.stack([np.repeat(v, v.size), np.tile(v, v.size), np.repeat(v[::-1], v.size)], 1)
    d = probe.both("sub3", [p.reshape(-1), p.reshape(-1).copy()], [(torch.float32, 3)], n=len(p))
    assert (DM.bits(d.reshape(-1)) == 0).all()
    z = probe.both("sub3", [np.array([-0.0, -0.0, 0.0], F), np.array([0.0, -0.0, -0.0], F)], [(torch.float32, 3)], n=1)
    assert list(DM.bits(z.reshape(-1))) == [0x80000000, 0, 0]                     # only (-0) - (+0) is -0


def test_sqrt_rn_and_inv_sqrt_rn_same_bits_as_ieee(probe):
    x = DM.sqrt_in_range()
    s = probe.both("sqrt_rn", [x], [torch.float32])
    assert bits_equal(s, np.sqrt(x).astype(F)).all()
    lo = DM.sqrt_below_range()
    sl = probe.both("sqrt_rn", [lo], [torch.float32])
    off = ~bits_equal(sl, np.sqrt(lo).astype(F))
    print(f"sqrt_rn below 2^-96 (outside its domain, reported only): {off.sum()} of {lo.size} differ from sqrtf ({100.0 * off.mean():.2f} %), "
          f"{(off & (lo >= F(2.0 ** -126))).sum()} of them normal arguments")
    r = DM.inv_sqrt()
    v = probe.both("inv_sqrt_rn", [r], [torch.float32])
    assert bits_equal(v, (F(1.0) / np.sqrt(r).astype(F)).astype(F)).all()         # two roundings


def test_exhaustive_sweeps_against_the_device_operations(probe):
    """On the device, against the compiler's own IEEE `/`, sqrtf and 1.0f / sqrtf: every float of sqrt_rn's range [2^-96, 2^40] and
    0, every float of inv_sqrt_rn's [2^-20, 2^20] (both builds), every numerator magnitude in [2^-40, 2^7) with both signs for each
    `res` (the vote's flags), and for the PPF (pair_mlp.o's flags) every distance d in [2^-30, 2] and d = 0 against 4096 numerators
    +-d (1 - k / 2048) each.  Zero mismatches."""
    report = []
    for b in BUILDS:
        report.append((b + "sqrt_rn", probe.sweep(b, "sweep_sqrt_rn", C.c_uint32(fbits(2.0 ** -96)), C.c_uint64((136 << 23) + 1))))
        report.append((b + "sqrt_rn(0)", probe.sweep(b, "sweep_sqrt_rn", C.c_uint32(0), C.c_uint64(1))))
        report.append((b + "inv_sqrt_rn", probe.sweep(b, "sweep_inv_sqrt_rn", C.c_uint32(fbits(2.0 ** -20)), C.c_uint64((40 << 23) + 1))))
    for res in DM.vote_res():
        report.append((f"div_by(a, {res:.9g})", probe.sweep(BUILDS[0], "sweep_div_by", C.c_float(float(res)), C.c_uint32(fbits(2.0 ** -40)), C.c_uint64(47 << 23))))
    report.append(("ppf d = 0", probe.sweep(BUILDS[1], "sweep_div_ppf", C.c_uint32(0), C.c_uint64(1), C.c_int(2048))))
    report.append(("ppf d in [2^-30, 2]", probe.sweep(BUILDS[1], "sweep_div_ppf", C.c_uint32(fbits(2.0 ** -30)), C.c_uint64((31 << 23) + 1), C.c_int(2048))))
    for name, (bad, first) in report:
        print(f"sweep {name}: {bad} mismatches" + ("" if first is None else f", first operand bits {first:#x}"))
    assert all(bad == 0 for _, (bad, _) in report)


# ------------------------------------------------------------------------------------ det_exp2w
def test_det_exp2w_is_the_oracles_and_within_its_stated_error(probe, oracle):
    c = DM.exp2w()
    w = probe.both("det_exp2w", [c["l"], c["c"]], [torch.float32])
    assert bits_equal(w, oracle.exp2w(c["l"], c["c"])).all()
    y = c["y"].astype(D)
    normal = y >= -126
    ref = DM.mp_exp2(c["y"][normal])
    rel = np.abs(w[normal].astype(D) - ref) / ref
    print(f"det_exp2w on the device: max relative error {rel.max():.4g} against 2^y (mpmath), {normal.sum()} normal results")
    assert rel.max() <= 2.7e-6
    sub = (y < -126) & (y >= -150)
    exact = np.exp2(y[sub] - np.floor(y[sub])) * np.exp2(np.floor(y[sub]))
    assert (np.abs(w[sub].astype(D) - exact) <= 2.0 ** -150 + 2.7e-6 * exact).all()      # half a subnormal quantum + the relative error
    assert (w[y < -151] == 0).all() and (DM.bits(w) >> 31 == 0).all()              # exactly +0 below the last subnormal


# ------------------------------------------------------------------------------------ det_sincos / rot_cs / det_tanf
def test_det_sincos_is_the_oracles_and_below_one_ulp(probe, oracle):
    x = DM.sincos_x()
    s, c = probe.both("det_sincos", [x], [torch.float64, torch.float64])
    o = np.array([oracle.sincos(v) for v in x], D)
    assert (s.view(np.uint64) == o[:, 0].view(np.uint64)).all() and (c.view(np.uint64) == o[:, 1].copy().view(np.uint64)).all()
    ms, mc = DM.mp_sincos(x)
    es, ec = DM.mp_abs_err(s, ms), DM.mp_abs_err(c, mc)
    print(f"det_sincos on the device, [-2 pi, 2 pi]: max abs error sin {es.max() * 2.0 ** 53:.3f}, cos {ec.max() * 2.0 ** 53:.3f} (x 2^-53)")
    assert max(es.max(), ec.max()) <= 2.0 ** -52


def test_rot_cs_is_the_oracles_and_the_correctly_rounded_fp32(probe, oracle):
    """every (i, n), n = 1 .. 360, i = 0 .. n: the oracle's bits, and the correctly rounded fp32 cos / sin of the fp32 angle (mpmath);
    device_math_cases.ROT_CS_BOUNDARY names the pairs for which that is relaxed to one ulp (none)"""
    i, n = DM.rot_pairs()
    cs, sn = probe.both("rot_cs", [i, n], [torch.float32, torch.float32])
    o = np.array([oracle.rot_cs(int(a), int(b)) for a, b in zip(i, n)], F)
    assert bits_equal(cs, o[:, 0]).all() and bits_equal(sn, o[:, 1]).all()
    ms, mc = DM.mp_sincos(DM.rot_angles(i, n).astype(D))
    rc, rs = DM.mp_round_f32(mc), DM.mp_round_f32(ms)
    relaxed = np.array([(int(a), int(b)) in set(DM.ROT_CS_BOUNDARY) for a, b in zip(i, n)])
    exact = bits_equal(cs, rc) & bits_equal(sn, rs)
    ulp = lambda a, b: np.abs(DM.f2ord_np(a).astype(np.int64) - DM.f2ord_np(b).astype(np.int64))
    print(f"rot_cs on the device: {(~exact).sum()} of {i.size} (i, n) differ from the correctly rounded value")
    assert exact[~relaxed].all() and (ulp(cs, rc) <= 1).all() and (ulp(sn, rs) <= 1).all()


def test_det_tanf_is_the_oracles_with_the_sign_branch(probe, oracle):
    t = DM.tan_x()
    v = probe.both("det_tanf", [t], [torch.float32])
    assert bits_equal(v, np.array([oracle.tanf(float(a)) for a in t], F)).all()
    # the branch of voting.py:142 as tests/ref_vote_cases.py expects it: float(pi/2) lies beyond pi/2, its tangent is negative
    assert v[0] == 0 and v[1] > 0 and v[2] < 0 and v[3] < 0 and v[4] < 0 and v[5] > 0 and np.isfinite(v).all()


# ------------------------------------------------------------------------------------ approximate inverse trigonometry
def test_atan01_and_acos_within_their_stated_bounds(probe):
    x = DM.atan01_x()
    e = np.abs(probe.both("atan01_approx", [x], [torch.float32]).astype(D) - np.arctan(x.astype(D)))
    u = DM.acos_x()
    a = probe.both("acos_approx", [u], [torch.float32])
    ea = np.abs(a.astype(D) - np.arccos(u.astype(D)))
    print(f"on the device: atan01_approx max error {e.max():.4g} (stated 2e-5), acos_approx {ea.max():.4g} (stated 1e-4)")
    assert e.max() < 2e-5 and ea.max() < 1e-4
    assert (a >= 0).all() and (a <= PI_F).all()


def test_atan2_bound_range_and_signed_zeros(probe):
    """|error| < 1e-4 against numpy's fp64 arctan2 from length 1e-30 (below what bv_arc lets through) to 1e6 (the callers: <= 2^7), the
    result in [-pi, pi], atan2(+-0, +-0) = 0.
    (-0, x < 0) gives -pi and (+0, x < 0) gives +pi: the comment in csrc/vote_common.h says so, and it is harmless because both
    callers turn the angle into a rotation INDEX modulo n: axis_arc_mask (csrc/vote.hip) wraps f = atan2 * n / 2 pi into [0, n) before
    it builds the mask, and bv_arc reduces i_lo modulo n after adding one index of margin on either side, so -n/2 and +n/2 name the
    same rotation up to that margin -- test_bv_arc_superset_and_not_vacuous runs tuples with B = -0 and B = +0, A < 0, side by side."""
    c = DM.atan2_yx()
    r = probe.both("atan2_approx", [c["y"], c["x"]], [torch.float32])
    zero = (c["x"] == 0) & (c["y"] == 0)
    err = np.where(zero, 0.0, np.abs(r.astype(D) - np.arctan2(c["y"].astype(D), c["x"].astype(D))))
    for m in DM.ATAN2_MAGS:
        sel = (c["kind"] == 0) & (np.abs(np.hypot(c["x"].astype(D), c["y"].astype(D)) / m - 1) < 1e-3)
        print(f"atan2_approx on the device at length {m:g}: max error {err[sel].max():.4g}")
    print(f"atan2_approx on the device, all {r.size} cases: max error {err.max():.4g} (stated 1e-4)")
    assert err.max() < 1e-4
    assert np.isfinite(r).all() and (np.abs(r) <= PI_F).all()
    assert zero.sum() == 4 and (r[zero] == 0).all()
    neg_x = (c["kind"] == 2) & (c["x"] == -1) & (c["y"] == 0)
    got = {fbits(y): fbits(v) for y, v in zip(c["y"][neg_x], r[neg_x])}
    assert got == {fbits(0.0): fbits(PI_F), fbits(-0.0): fbits(-PI_F)}


# ------------------------------------------------------------------------------------ f2ord / ord2f and the arg-max keys
def test_f2ord_is_strictly_monotone_and_ord2f_inverts_it(probe):
    s = DM.ordered_floats()
    k = probe.both("f2ord", [s], [torch.int32]).view(np.uint32)
    assert (np.diff(k.astype(np.int64)) > 0).all() and (k == DM.f2ord_np(s)).all()
    b = DM.random_bit_patterns()
    kk = probe.both("f2ord", [DM.from_bits(b)], [torch.int32]).view(np.uint32)
    back = probe.both("ord2f", [kk.view(np.int32)], [torch.float32])
    assert (DM.bits(back) == b).all() and (kk == DM.f2ord_np(DM.from_bits(b))).all()


def signed_zero_grids():
    """grids whose maximum is 0: a -0 before a +0, the reverse, and -0 alone -> (grid, index of the first zero)"""
    out = []
    for n in (65, 1000):
        g = -np.abs(np.random.default_rng(n).normal(size=n)).astype(F) - 1
        a, b = n // 3, n // 3 + 40
        for za, zb in ((-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
            h = g.copy()
            h[a], h[b] = za, zb
            out.append((h, a))
    return out


def test_grid_argmax_ties_signed_zeros_as_numpy_does(dev):
    """f2ord orders -0 below +0 (test_f2ord_is_strictly_monotone_and_ord2f_inverts_it), yet the library's arg-max has numpy's tie rule
    for signed zeros as well: reduce_argmax_kernel adds its sum of votes, +0 at least, to the cell before it takes the key, and
    -0 + +0 = +0.  include/cppf.h says so; pinned here: the first zero wins whatever its sign, and the value comes back as +0."""
    for g, first in signed_zero_grids():
        assert int(np.argmax(g)) == first
        oi, ov = voting.grid_argmax(torch.from_numpy(g).to(dev))
        assert int(oi.item()) == first and int(ov.cpu().numpy().view(np.uint32)[0]) == 0


def test_vote_argmax_accumulate_has_no_negative_zero(dev, oracle):
    """cppf_vote_argmax with CPPF_VOTE_ACCUMULATE adds the votes (>= +0) to every cell, and -0 + +0 = +0: the accumulated grid holds no
    -0, and its arg-max is numpy's on the grid it leaves, whatever zeros the caller put in"""
    import cppf_amd.synthetic as syn
    ob = syn.make_object("can", 64, 3)
    corner, dims = oracle.grid_setup(ob["pc"], ob["cfg"].res)
    idx = np.stack([np.arange(32), np.arange(32)], 1).astype(np.int32)             # a == b: no pair votes
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        g = np.full(int(np.prod(dims)), -1.0, F)
        a, b = g.size // 3, g.size // 3 + 77
        g[a], g[b] = first, second
        grid = d(g.reshape(tuple(int(v) for v in dims)))
        oi, ov = voting.vote_argmax(d(ob["pc"]), d(np.zeros((32, 2), F)), d(np.ones(64, F)), d(idx), grid, d(corner), ob["cfg"].res, 72, True,
                                    accumulate=True)
        left = grid.cpu().numpy().reshape(-1)
        rest = np.ones(g.size, bool)
        rest[[a, b]] = False
        assert (DM.bits(left[[a, b]]) == 0).all() and (left[rest] == -1).all()
        assert int(oi.item()) == int(np.argmax(left)) == a and int(ov.cpu().numpy().view(np.uint32)[0]) == 0


# ------------------------------------------------------------------------------------ wave helpers
def test_wave_scan_and_wave_max(probe):
    ints, keys = DM.wave_blocks()
    sc = probe.both("wave_incl_scan", [ints], [torch.int32])
    assert (sc.reshape(-1, 64) == np.cumsum(ints.reshape(-1, 64), axis=1, dtype=np.int32)).all()
    mx = probe.both("wave_max_u64", [keys.view(np.int64)], [torch.int64]).view(np.uint64)
    assert (mx.reshape(-1, 64) == keys.reshape(-1, 64).max(1, keepdims=True)).all()


# ------------------------------------------------------------------------------------ bv_arc
def test_bv_arc_superset_and_not_vacuous(probe, oracle):
    """"A superset ... never a dropped vote": every rotation that passes the loop's own fp32 test (voting.py:101, restated in the
    reference's operation order with oracle.rot_cs) lies in [lo, lo + cnt) modulo n -- zero dropped, no tolerance; and the screen
    screens: for n >= 16, L2 >= 1e-6, M > 1e-3 and an exact span of at most half the circle, cnt < n (cnt ~ 2 (alpha + 8e-4) n / 2 pi
    + 3).  The tuples include B = -0 / +0 with A < 0, where atan2_approx returns -pi / +pi."""
    c = DM.arc_tuples()
    S = DM.arc_passing(oracle, c)
    lo, cnt = probe.both("bv_arc", [c["L2"], c["w"].reshape(-1), c["x"].reshape(-1), c["y"].reshape(-1), c["tol"], c["n"], c["cmax"]],
                         [torch.int32, torch.int32])
    assert ((lo >= 0) & (lo < np.maximum(c["n"], 1)) & (cnt >= 0) & (cnt <= c["n"])).all()
    dropped = S & ~DM.arc_member(lo, cnt, c["n"], S.shape[1])
    lo_np, cnt_np = DM.bv_arc_np(c)
    print(f"bv_arc on the device: {len(c['n'])} tuples {DM.arc_regimes(c, cnt)}, {int(S.sum())} passing rotations, {int(dropped.sum())} dropped; "
          f"{int((cnt != cnt_np).sum())} counts differ from the numpy restatement")
    assert dropped.sum() == 0
    alpha, M = DM.arc_exact_span(c)
    sel = (c["n"] >= 16) & (c["L2"] >= F(1e-6)) & (M > 1e-3) & ~(alpha > np.pi / 2)
    assert sel.sum() > 1000 and (cnt[sel] < c["n"][sel]).all()
    z = c["group"] == 3
    assert (S[z].any(1)).sum() > 100                                             # the signed-zero tuples do have rotations to keep
