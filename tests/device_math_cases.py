"""Inputs for the shared device arithmetic of csrc/cppf_math.h, csrc/vote_common.h and csrc/backvote_common.h, one family per
primitive (and, for div_by, per call site), plus the plain references and numpy restatements the tests compare against.  Shared by
tests/test_device_math_cases_cpu.py (the families are what they say; the oracle's functions and the restatement of bv_arc meet the
same bounds) and tests/test_gpu_device_math.py (the device, through csrc/probe/math_probe.hip).  Deterministic; not a test module.
Every family holds at most 2^21 elements.

Conventions: float32 arrays unless said otherwise; "edge mantissas" of a binade 2^e are EDGE_MANT (the binade's first two and last
two floats and its middle); "binades [2^a, 2^b]" means e = a .. b - 1 plus the single value 2^b.
"""
import numpy as np

from oracle import voting_numpy as VN

F, D = np.float32, np.float64
U32 = np.uint32
EDGE_MANT = (0, 1, 0x400000, 0x7FFFFE, 0x7FFFFF)
TINY = F(2.0 ** -149)                      # the smallest positive float
LOG2E = F(1.44269504088896341)
# the `res` of every category of cppf_amd/config.py and the twelve of profiles/microbench/div_check.hip
DIV_CHECK_RES = (4e-3, 1e-2, 3e-2, 2e-3, 1.2e-3, 0.0123, 0.1, 1.5e-2, 8e-3, 1e-3, 0.25, 7.77e-3)


def vote_res():
    from cppf_amd.config import CATEGORIES, YAML_DEFAULTS
    vals = {float(F(c.res)) for c in CATEGORIES.values()} | {float(F(YAML_DEFAULTS["res"]))} | {float(F(r)) for r in DIV_CHECK_RES}
    return np.array(sorted(vals), F)


def bits(x):
    return np.ascontiguousarray(x, F).view(U32)


def from_bits(b):
    return np.ascontiguousarray(b, U32).view(F)


def binades(e_lo, e_hi, n_random, rng, closed=True):
    """floats m 2^e for e = e_lo .. e_hi - 1 with the EDGE_MANT mantissas and n_random random ones each; closed: plus 2^e_hi"""
    e = np.arange(e_lo, e_hi, dtype=np.int64)[:, None] + 127
    assert e.min() >= 1 and e.max() <= 254
    m = np.concatenate([np.broadcast_to(np.array(EDGE_MANT, np.int64), (len(e), len(EDGE_MANT))),
                        rng.integers(0, 1 << 23, (len(e), n_random))], 1)
    out = from_bits(((e << 23) | m).astype(U32).reshape(-1))
    return np.concatenate([out, [F(2.0) ** F(e_hi)]]).astype(F) if closed else out


def prev(x):
    """the float next to x towards 0"""
    return np.nextafter(np.asarray(x, F), F(0))


# ------------------------------------------------------------------------------------ exact fp32 fma
def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in fp64, the sum is rounded to odd in fp64 (TwoSum) and
    then to nearest in fp32 -- 53 >= 2 * 24 + 2 bits, so the double rounding is innocuous"""
    a, b, c = (np.asarray(v, F).astype(D) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    with np.errstate(invalid="ignore"):
        s = np.where((err != 0) & even & np.isfinite(s), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


# ------------------------------------------------------------------------------------ div_by
def _numerators(d, n_random, rng):
    """for each denominator-side bound d >= 0: +-d, +-d (1 - 2^-24), +-the smallest float (where d > 0), 0 and n_random random |a| <= d"""
    d = np.asarray(d, F)
    d1 = (d * F(1 - 2.0 ** -24)).astype(F)
    tiny = np.where(d > 0, TINY, F(0)).astype(F)
    cols = [d, -d, d1, -d1, tiny, -tiny, np.zeros_like(d)]
    r = rng.uniform(-1.0, 1.0, (n_random, d.size))
    cols += [np.clip((d.astype(D) * r[k]).astype(F), -d, d) for k in range(n_random)]
    return (np.stack(cols, 1).astype(F) + F(0)).astype(F)           # (-0 -> +0: div_by's stated exception has its own test)


def subnormal_quotient(a, den):
    """the IEEE quotient a / den is a non-zero subnormal: outside "the normal range" div_by is written for"""
    q = np.abs((np.asarray(a, F) / np.asarray(den, F)).astype(F))
    return (q > 0) & (q < F(2.0 ** -126))


def div_ppf(seed=1):
    """ppf_from (csrc/pair_mlp_common.h): xy / (d + 1e-7f), d = |xy|'s fp32 length, so |xy_i| <= d; "den in [1e-7, ~2]".
    d in {0} and every binade [2^-30, 2] with the edge mantissas and 64 random ones -> a f32[n], den f32[n], d f32[n]"""
    rng = np.random.default_rng(seed)
    d = np.concatenate([[F(0)], binades(-30, 1, 64, rng)]).astype(F)
    a = _numerators(d, 16, rng)
    den = (d + F(1e-7)).astype(F)
    return dict(a=a.reshape(-1), den=np.repeat(den, a.shape[1]), d=np.repeat(d, a.shape[1]))


def div_pair_frame(l_max=4.0, seed=2):
    """pair_frame (csrc/cppf_math.h): ab / den and co / den, den = (float)((double)L + 1e-7) -- "denominators in [1e-7, ~2]", L (lc)
    from the smallest float >= 1e-7 up to l_max (4 for the pair distance; 1 for |co|, a part of the unit ab), numerators |a| <= L"""
    rng = np.random.default_rng(seed)
    l0 = F(1e-7) if float(F(1e-7)) >= 1e-7 else np.nextafter(F(1e-7), F(1))
    L = binades(-24, int(np.log2(l_max)), 64, rng)
    L = np.concatenate([[l0, np.nextafter(l0, F(1))], L[L.astype(D) >= 1e-7]]).astype(F)
    a = _numerators(L, 16, rng)
    den = (L.astype(D) + 1e-7).astype(F)
    return dict(a=a.reshape(-1), den=np.repeat(den, a.shape[1]), d=np.repeat(L, a.shape[1]))


def div_vote(seed=3):
    """the vote's a / res (csrc/vote.hip, pose_tail.hip, scene_multi.hip): "|a| <= a few metres over res ~ 1e-3..1e-1", checked range
    |a| in [2^-40, 2^7): every binade with the edge mantissas and 32 random ones, both signs, for every res of vote_res()"""
    rng = np.random.default_rng(seed)
    mag = binades(-40, 7, 32, rng, closed=False)
    a = np.concatenate([mag, -mag])
    res = vote_res()
    return dict(a=np.tile(a, res.size), den=np.repeat(res, a.size))


def inv_sqrt(seed=4):
    """inv_sqrt_rn: "x >= 2^-20" (the LayerNorm's var + eps): every binade [2^-20, 2^20] with edge mantissas and 32 random ones, and
    var + 1e-5f for var in {0, 1e-30, 1e-5, 1, 1e4}"""
    rng = np.random.default_rng(seed)
    var = np.array([0, 1e-30, 1e-5, 1, 1e4], F)
    return np.concatenate([binades(-20, 20, 32, rng), (var + F(1e-5)).astype(F)]).astype(F)


def sqrt_in_range(seed=5):
    """sqrt_rn's domain: 0 and [2^-96, 2^40] (every binade: edge mantissas, 32 random), and k^2, k^2 -+ 1 ulp for integers k and
    scaled ones (k 2^-40)"""
    rng = np.random.default_rng(seed)
    k = np.concatenate([np.arange(1, 4097), rng.integers(4097, 1 << 20, 2048)]).astype(D)
    sq = np.concatenate([(k * k), (k * 2.0 ** -40) ** 2]).astype(F)      # exact where k < 2^12, rounded above
    sq = np.concatenate([sq, np.nextafter(sq, F(0)), np.nextafter(sq, F(np.inf))])
    x = np.concatenate([[F(0)], binades(-96, 40, 32, rng), sq]).astype(F)
    assert ((x == 0) | ((x >= F(2.0 ** -96)) & (x <= F(2.0 ** 40)))).all()
    return x


def sqrt_below_range(seed=6):
    """below 2^-96, where sqrt_rn is documented to be off by an ulp now and then: reported, not asserted.  Subnormals and every
    binade [2^-126, 2^-96)"""
    rng = np.random.default_rng(seed)
    sub = from_bits(np.concatenate([[1, 2, 3, 0x7FFFFF, 0x400000], rng.integers(1, 1 << 23, 2048)]).astype(U32))
    return np.concatenate([sub, binades(-126, -96, 256, rng, closed=False)]).astype(F)


# ------------------------------------------------------------------------------------ det_exp2w
EXP2_SPREADS = (0.0, 1.0, 90.0, 1000.0)
EXP2_MAXES = (-30.0, 0.37, 12.5, 88.0)


def exp2w(seed=7):
    """(l, c) with y = fmaf(l, log2e, c) covering [-200, 2] -> l, c, y (fp32; y exact through fma32) and `kind` per element:
      0  every integer y in [-200, 2] and its two float neighbours, y = -0 (l = -0, c = -0) and y = +0   [l = +-0, c = y]
      1  y just below 0: -2^-149 .. -2^-1 by powers of two and -1 + 2^-24 .. (v_fract must clamp to 0x1.fffffep-1)
      2  the transition through the subnormals, y in [-150, -125], 2^13 values
      3  dense [-200, 2], 2^15 values
      4  realistic pairs: logits l in [max - spread, max], c = -(max log2e) in fp32, for EXP2_SPREADS x EXP2_MAXES, 1024 each
         (the row maximum itself is the first of each block: y = 0 up to the fma's rounding)"""
    rng = np.random.default_rng(seed)
    ints = np.arange(-200, 3).astype(F)
    y0 = np.concatenate([ints, np.nextafter(ints, F(-np.inf)), np.nextafter(ints, F(np.inf)), [F(0)]])
    y1 = np.concatenate([-(F(2.0) ** np.arange(-149, 0).astype(F)), [prev(F(-1)), prev(prev(F(-1))), F(-0.99999)]]).astype(F)
    y2 = rng.uniform(-150, -125, 1 << 13).astype(F)
    y3 = rng.uniform(-200, 2, 1 << 15).astype(F)
    l = [np.zeros_like(y0), np.zeros_like(y1), np.zeros_like(y2), np.zeros_like(y3)]
    c = [y0, y1, y2, y3]
    kind = [np.full(y.size, k) for k, y in enumerate(c)]
    l[0] = np.concatenate([l[0], [F(-0.0)]]); c[0] = np.concatenate([c[0], [F(-0.0)]]); kind[0] = np.full(c[0].size, 0)
    for spread in EXP2_SPREADS:
        for mx in EXP2_MAXES:
            ll = (F(mx) - rng.uniform(0, 1, 1024) * spread).astype(F)
            ll[0] = F(mx)
            l.append(ll)
            c.append(np.full(1024, -(F(mx) * LOG2E), F))
            kind.append(np.full(1024, 4))
    l, c = np.concatenate(l).astype(F), np.concatenate(c).astype(F)
    return dict(l=l, c=c, y=fma32(l, LOG2E, c), kind=np.concatenate(kind))


def mp_exp2(y):
    """2^y of float32 y in mpmath at 120 bits -> (fp64 value, exact to fp64 rounding; only used where it is normal in fp64)"""
    import mpmath
    with mpmath.workprec(120):
        return np.array([float(mpmath.power(2, mpmath.mpf(float(v)))) for v in np.asarray(y, F)], D)


# ------------------------------------------------------------------------------------ det_sincos / rot_cs / det_tanf
def sincos_x(seed=8):
    """fp64 x: [-2 pi, 2 pi] dense (2^14 uniform), every multiple k pi / 4, k = -8 .. 8, as fp64 and its two neighbours (the quadrant
    switches of the reduction), 0 and -0"""
    rng = np.random.default_rng(seed)
    q = np.arange(-8, 9) * (np.pi / 4)
    return np.concatenate([rng.uniform(-2 * np.pi, 2 * np.pi, 1 << 14), q, np.nextafter(q, -np.inf), np.nextafter(q, np.inf), [0.0, -0.0]]).astype(D)


def mp_sincos(x):
    import mpmath
    with mpmath.workprec(120):
        xs = [mpmath.mpf(float(v)) for v in np.asarray(x, D)]
        return [mpmath.sin(v) for v in xs], [mpmath.cos(v) for v in xs]


def mp_abs_err(val, mp_vals):
    """|val - exact| in fp64 for fp64 val and mpmath exact values, the difference taken at 120 bits"""
    import mpmath
    with mpmath.workprec(120):
        return np.array([float(abs(mpmath.mpf(float(v)) - m)) for v, m in zip(val, mp_vals)], D)


def mp_round_f32(mp_vals):
    """the correctly rounded fp32 of mpmath values: through fp64, and where that lands exactly on the middle of two floats (a double
    rounding could go either way) decided at full precision"""
    import mpmath
    v64 = np.array([float(m) for m in mp_vals], D)
    out = v64.astype(F)
    hazard = np.nonzero((v64.view(np.int64) & ((1 << 29) - 1)) == (1 << 28))[0]
    with mpmath.workprec(120):
        for i in hazard:
            cands = [out[i], np.nextafter(out[i], F(-np.inf)), np.nextafter(out[i], F(np.inf))]
            out[i] = min(cands, key=lambda c: abs(mpmath.mpf(float(c)) - mp_vals[i]))
    return out


ROT_N_MAX = 360
# (i, n) whose fp64 cos / sin sits so close to the middle of two floats that a < 1 ulp(fp64) evaluation may round the other way:
# for these alone "equals the correctly rounded fp32" becomes "within one fp32 ulp".  Found with the oracle on the CPU
# (tests/test_device_math_cases_cpu.py asserts the list is complete for the oracle and at most 0.1 % of the pairs).
ROT_CS_BOUNDARY = ()


def rot_pairs():
    """every (i, n), n = 1 .. 360, i = 0 .. n (i = n: the full turn) -> i i32[], n i32[]"""
    n = np.repeat(np.arange(1, ROT_N_MAX + 1), np.arange(2, ROT_N_MAX + 2))
    i = np.concatenate([np.arange(k + 1) for k in range(1, ROT_N_MAX + 1)])
    return i.astype(np.int32), n.astype(np.int32)


def rot_angles(i, n):
    """(float)((double)(i * 2) * M_PI / (double)n), reference models/voting.py:33"""
    return ((i.astype(D) * 2) * VN.M_PI / n.astype(D)).astype(F)


def tan_x(seed=9):
    """the six `rot` of tests/ref_vote_cases.py (0, +-(pi/2 - 1 ulp), -0.7, +-float(pi/2)) first, then [-pi/2, pi/2] dense (2^12)"""
    h = np.nextafter(F(np.pi / 2), F(0))
    six = np.array([0.0, h, -h, -0.7, F(np.pi / 2), -F(np.pi / 2)], F)
    return np.concatenate([six, np.random.default_rng(seed).uniform(-np.pi / 2, np.pi / 2, 1 << 12).astype(F)]).astype(F)


# ------------------------------------------------------------------------------------ approximate inverse trigonometry
SUBNORMALS = from_bits(np.array([1, 2, 0x400000, 0x7FFFFF], U32))


def atan01_x():
    """[0, 1] dense (2^20 evenly spaced, 0 and 1 included), the subnormals, the smallest normal, 1 - 2^-24"""
    return np.concatenate([np.linspace(0.0, 1.0, 1 << 20).astype(F), SUBNORMALS, [F(2.0 ** -126), prev(F(1))]]).astype(F)


ATAN2_MAGS = (1e-30, 1e-20, 1e-3, 1.0, 8.5, 128.0, 1280.0, 1e6)
ATAN2_N_UNIT, ATAN2_N_OTHER = 1 << 20, 1 << 16


def atan2_yx():
    """-> y, x and `kind`:
      0  angles evenly spaced on the circle at magnitude 1 (2^20) and at every other magnitude of ATAN2_MAGS (2^16 each): 1e-30 is
         the smallest the callers let through (bv_arc: M > 1e-30), 128 = 2^7 the largest the callers produce (coordinates of a few metres, divided by
         nothing), 1280 one decade beyond, 1e6 far beyond
      1  the eight axis and diagonal directions at every magnitude
      2  every sign combination of (+-0, +-0) and (+-0, +-1), (+-1, +-0)
      3  |x| = |y| exactly, and |x|, |y| one ulp apart, every sign, at every magnitude"""
    ys, xs, ks = [], [], []
    for m in ATAN2_MAGS:
        n = ATAN2_N_UNIT if m == 1.0 else ATAN2_N_OTHER
        th = (np.arange(n) + 0.5) * (2 * np.pi / n) - np.pi
        ys.append((m * np.sin(th)).astype(F)); xs.append((m * np.cos(th)).astype(F)); ks.append(np.zeros(n, int))
        for sy, sx in ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)):
            ys.append(np.array([sy * m], F)); xs.append(np.array([sx * m], F)); ks.append(np.array([1]))
        v = F(m)
        for u in (v, np.nextafter(v, F(0)), np.nextafter(v, F(np.inf))):
            for sy in (1, -1):
                for sx in (1, -1):
                    ys.append(np.array([sy * u], F)); xs.append(np.array([sx * v], F)); ks.append(np.array([3]))
    z = (F(0.0), F(-0.0))
    for a in z:
        for b in z + (F(1), F(-1)):
            ys.append(np.array([a], F)); xs.append(np.array([b], F)); ks.append(np.array([2]))
            if b != 0:
                ys.append(np.array([b], F)); xs.append(np.array([a], F)); ks.append(np.array([2]))
    return dict(y=np.concatenate(ys).astype(F), x=np.concatenate(xs).astype(F), kind=np.concatenate(ks))


def acos_x():
    """[-1, 1] dense (2^20 evenly spaced, -1 and 1 included), +-(1 - 2^-24), +-0, +-subnormals"""
    return np.concatenate([np.linspace(-1.0, 1.0, 1 << 20).astype(F), [prev(F(1)), -prev(F(1)), F(0.0), F(-0.0)], SUBNORMALS, -SUBNORMALS]).astype(F)


def _fmaf(a, b, c):
    return (np.asarray(a, F).astype(D) * np.asarray(b, F).astype(D) + np.asarray(c, F).astype(D)).astype(F)


def atan01_np(t):
    """atan01_approx in fp32 numpy (fmaf through fp64: a double rounding here and there, irrelevant at 1e-5)"""
    t = np.asarray(t, F)
    t2 = (t * t).astype(F)
    p = _fmaf(t2, F(0.0208351), F(-0.0851330))
    for k in (0.1801410, -0.3302995, 0.9998660):
        p = _fmaf(t2, p, F(k))
    return (p * t).astype(F)


def atan2_np(y, x):
    """atan2_approx in fp32 numpy, an IEEE quotient where the device multiplies by v_rcp_f32 (1 ulp)"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    r = atan01_np((mn * (F(1) / np.maximum(mx, F(1e-37))).astype(F)).astype(F))
    r = np.where(ay > ax, (F(1.57079633) - r).astype(F), r)
    r = np.where(x < 0, (F(3.14159265) - r).astype(F), r)
    return np.copysign(r, y).astype(F)


def acos_np(u):
    """acos_approx in fp32 numpy, an IEEE square root where the device has v_sqrt_f32 (1 ulp)"""
    u = np.asarray(u, F)
    ax = np.abs(u)
    p = _fmaf(ax, F(-0.0187293), F(0.0742610))
    p = _fmaf(p, ax, F(-0.2121144))
    p = _fmaf(p, ax, F(1.5707288))
    r = (p * np.sqrt(np.maximum((F(1) - ax).astype(F), F(0))).astype(F)).astype(F)
    return np.where(u < 0, (F(3.14159265) - r).astype(F), r).astype(F)


# ------------------------------------------------------------------------------------ f2ord / ord2f
def ordered_floats():
    """strictly increasing in the total order of f2ord: -inf, -max, .., -1, .., -min normal, -subnormals, -0, +0, +subnormals, .. +inf"""
    pos = np.concatenate([SUBNORMALS[[0, 1, 2, 3]], [F(2.0 ** -126), np.nextafter(F(2.0 ** -126), F(1)), F(1e-20), prev(F(1)), F(1),
                                                   np.nextafter(F(1), F(2)), F(8.5), F(1e20), np.finfo(F).max, F(np.inf)]]).astype(F)
    return np.concatenate([-pos[::-1], [F(-0.0), F(0.0)], pos]).astype(F)


def f2ord_np(x):
    u = bits(x)
    return np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)


def random_bit_patterns(seed=10):
    """2^20 random float bit patterns, NaNs excluded"""
    b = np.random.default_rng(seed).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(U32)
    return b[~np.isnan(from_bits(b))]


# ------------------------------------------------------------------------------------ wave helpers
def wave_blocks(seed=11):
    """workgroups of 256 lanes (four waves), one element per lane -> ints i32[5 * 256], keys u64[5 * 256]; block 0, 1: random; 2: every
    lane equal; 3: the maximum in lane 0 of each wave; 4: the maximum in lane 63 of each wave"""
    rng = np.random.default_rng(seed)
    ints = rng.integers(-(1 << 20), 1 << 20, (5, 256)).astype(np.int32)
    keys = rng.integers(0, 1 << 63, (5, 256), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (5, 256), dtype=np.uint64)
    ints[2] = 7
    keys[2] = np.uint64(0x8000000012345678)
    top = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys[3] >>= np.uint64(1); keys[4] >>= np.uint64(1)
    keys[3].reshape(4, 64)[:, 0] = top
    keys[4].reshape(4, 64)[:, 63] = top - np.uint64(1)
    return ints.reshape(-1), keys.reshape(-1)


# ------------------------------------------------------------------------------------ bv_arc
ARC_NS = (1, 2, 7, 16, 72, 120, 360)
# c = K / M targets: both sides of the two cuts (c > 1.0005: empty; c <= -0.9995: full scan) and a spread in between
ARC_C = (1.004, 1.001, 1.0006, 1.0004, 1.0, 0.9999, 0.99, 0.9, 0.5, 0.0, -0.5, -0.9, -0.99, -0.9994, -0.9996, -1.0)
ARC_EPS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 2e-5, -2e-5, 4e-5, -4e-5, 6e-5, -6e-5, 1e-4, -1e-4)


def _pairs_frame(a, u, L, mu, nu):
    """two points per tuple the way the kernels meet them: b = a - L u snapped to a binary grid so that a - b is exact in fp32; the
    fp32 frame of pair_frame (oracle/voting_numpy._frame), x scaled by odist = nu, cc = a - ab mu -> dict"""
    n = len(a)
    quantum = np.where(L < 1e-4, 2.0 ** -30, 2.0 ** -20)[:, None]
    delta = np.round(L[:, None] * u / quantum) * quantum
    a = (np.round(a / quantum) * quantum).astype(F)
    pts = np.stack([a.astype(D), a.astype(D) - delta], 1).reshape(2 * n, 3).astype(F)
    idx = np.arange(2 * n).reshape(n, 2)
    a32, ab, x, y, live = VN._frame(pts, idx, np.asarray(nu, F))
    assert live.all()
    cc = (a32 - (ab * np.asarray(mu, F)[:, None]).astype(F)).astype(F)
    dd = (pts[idx[:, 0]] - pts[idx[:, 1]]).astype(F)
    return dict(cc=cc, x=x, y=y, ab=ab, L2=VN._dot(dd, dd).astype(F))


def arc_tuples(seed=12):
    """Tuples (cc, gt, x, y, tol, n, L2) for bv_arc, x _|_ y, |x| = |y| = rho up to fp32 rounding, from pair_frame's arithmetic
    (x^ odist, y = x cross ab) -> dict of arrays, `group` per tuple:
      0 SPREAD  gt in the circle's plane at r = 1.1 rho from its axis, tol such that c = K / M takes each value of ARC_C, for every n of
                ARC_NS, rho in {2e-3, 0.05, 0.3}, L in {5e-4, 2e-3, 0.2} (L2 on both sides of 1e-6), centres near 0.7 and near 8.5
      1 EDGE    the regime of the earlier bug: |gt| ~ 8.5, res in {2e-3, 4e-3}, tol = 3 res, gt radially outward of sample t at
                rho + tol (1 + eps), eps of ARC_EPS: tol within 1e-4 tol of that sample's distance; t in {0, 1, n // 2, n - 1};
                rho / res from 0.16 (eight orientations each below 1: M = rho r is smallest there, and the (tol + dc) dc term decides)
                to 75
      2 AXIS    gt next to the circle's axis: M = rho r for r from 1e-3 down to 1e-36 (cc at the origin, so that w = gt is exact),
                tol on both sides of the common distance sqrt(rho^2 + h^2)
      3 ZERO    B = -0 or +0 with A < 0 (atan2_approx returns -pi or +pi: the arc must hold its rotations either way), hand-made
                frames x = (rho, 0, 0), y = (0, rho, 0), cc = 0, gt = (-r, -+0, -+0)"""
    rng = np.random.default_rng(seed)
    rows = []                                                              # (group, n, rho, L, centre scale, c or eps, t)
    for n in ARC_NS:
        for rho in (2e-3, 0.05, 0.3):
            for L in (5e-4, 2e-3, 0.2):
                for scale in (0.7, 8.5):
                    for c in ARC_C:
                        for rep in range(2):
                            rows.append((0, n, rho, L, scale, c, rep))
        for res in (2e-3, 4e-3):
            for nu_res in (0.16, 0.25, 0.5, 1.0, 2.7, 12.0, 75.0):
                for t in sorted({0, min(1, n - 1), n // 2, n - 1}):
                    for eps in ARC_EPS:
                        for L in (2e-3, 0.2):
                            for rep in range(8 if nu_res < 1 else 1):          # (more orientations where M is smallest)
                                rows.append((1, n, nu_res * res, L, 8.5, eps, t + 1000 * (res == 4e-3)))
    P = len(rows)
    grp = np.array([r[0] for r in rows]); n = np.array([r[1] for r in rows]); rho = np.array([r[2] for r in rows], D)
    L = np.array([r[3] for r in rows], D); scale = np.array([r[4] for r in rows], D); par = np.array([r[5] for r in rows], D)
    tt = np.array([r[6] for r in rows])
    u = rng.normal(size=(P, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])[np.arange(P) % 6]
    u = np.where((np.arange(P) % 4 == 3)[:, None], axes, u)                # one in four along a coordinate axis
    d = rng.normal(size=(P, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    a = scale[:, None] * d * np.where(grp == 1, 1.0, rng.uniform(0.5, 1.0, P))[:, None]
    mu = rng.uniform(-0.1, 0.1, P)
    fr = _pairs_frame(a, u, L, mu, rho)
    cc, x, y = fr["cc"].astype(D), fr["x"].astype(D), fr["y"].astype(D)
    rr = np.linalg.norm(x, axis=-1)                                        # the circle's radius as the kernel has it
    xh, yh = x / rr[:, None], y / np.linalg.norm(y, axis=-1, keepdims=True)
    # SPREAD: phi random, r = 1.1 rho, tol^2 = r^2 + rho^2 - 2 c rho r
    phi = rng.uniform(-np.pi, np.pi, P)
    r = 1.1 * rr
    tol = np.sqrt(np.maximum(r * r + rr * rr - 2 * par * rr * r, 0.0))
    # EDGE: phi = the angle of sample t, r = rho + tol (1 + eps), tol = 3 res
    edge = grp == 1
    res = np.where(tt >= 1000, 4e-3, 2e-3)
    t = tt % 1000
    phi = np.where(edge, 2 * np.pi * t / n, phi)
    tol = np.where(edge, (3 * res.astype(F)).astype(F).astype(D), tol)
    r = np.where(edge, rr + tol * (1 + par), r)
    gt = cc + r[:, None] * (np.cos(phi)[:, None] * xh + np.sin(phi)[:, None] * yh)
    out = dict(cc=fr["cc"], gt=gt.astype(F), x=fr["x"], y=fr["y"], tol=tol.astype(F), n=n.astype(np.int32), L2=fr["L2"], group=grp)
    # AXIS and ZERO: hand-made frames at the origin
    ex = []
    for nn in ARC_NS:
        for rh in (2e-3, 0.3):
            for h in (0.0, 0.01):
                for k, rad in enumerate((1e-3, 1e-8, 1e-16, 1e-19, 1e-22, 1e-25, 1e-28, 1e-32, 1e-36, 0.0)):
                    for f in (1 - 1e-3, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-3):
                        ang = 0.7 + k
                        ex.append((2, nn, rh, (rad * np.cos(ang), rad * np.sin(ang), h), np.sqrt(rh * rh + h * h) * f))
            for rad in (rh * 0.5, rh, rh * 2):
                for f in (0.2, 1.0, 1.5, 2.5):
                    for z in (-0.0, 0.0):
                        ex.append((3, nn, rh, (-rad, z, z), rh * f))
    E = len(ex)
    erho = np.array([e[2] for e in ex], F)
    zero = np.zeros(E, F)
    out2 = dict(cc=np.zeros((E, 3), F), gt=np.array([e[3] for e in ex], F), x=np.stack([erho, zero, zero], 1), y=np.stack([zero, erho, zero], 1),
                tol=np.array([e[4] for e in ex], F), n=np.array([e[1] for e in ex], np.int32), L2=np.full(E, 0.04, F),
                group=np.array([e[0] for e in ex]))
    out = {k: np.concatenate([out[k], out2[k]]) for k in out}
    out["w"] = (out["gt"] - out["cc"]).astype(F)                           # sub3(gt, cc)
    out["cmax"] = np.abs(out["cc"]).max(-1).astype(F)                      # bv_cmax
    return out


def arc_passing(O, c):
    """The loop's own fp32 test (voting.py:101 as backvote_body runs it) for every rotation of every tuple, in the reference's
    operation order with oracle.rot_cs: offset = cos x + sin y, pc = cc + offset, pass = !(length(pc - gt) > tol)
    -> bool[P, max n] (False for i >= n)"""
    P, nmax = len(c["n"]), int(c["n"].max())
    S = np.zeros((P, nmax), bool)
    for n in np.unique(c["n"]):
        r = np.nonzero(c["n"] == n)[0]
        cs = np.array([O.rot_cs(i, int(n)) for i in range(int(n))], F)
        off = ((cs[None, :, :1] * c["x"][r, None, :]).astype(F) + (cs[None, :, 1:] * c["y"][r, None, :]).astype(F)).astype(F)
        pc = (c["cc"][r, None, :] + off).astype(F)
        dd = VN._length((pc - c["gt"][r, None, :]).astype(F))
        S[r[:, None], np.arange(int(n))[None, :]] = ~(dd > c["tol"][r, None])
    return S


def arc_exact_span(c):
    """the exact angular half-width alpha of the set {t: |cc + cos t x + sin t y - gt| <= tol} in fp64 (nan: empty, pi: everything) and M"""
    w, x, y = c["w"].astype(D), c["x"].astype(D), c["y"].astype(D)
    A, B = (w * x).sum(-1), (w * y).sum(-1)
    M = np.hypot(A, B)
    K = 0.5 * ((w * w).sum(-1) + (x * x).sum(-1) - c["tol"].astype(D) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = K / M
    return np.where(q > 1, np.nan, np.arccos(np.clip(q, -1, 1))), M


def bv_arc_np(c, slack=8e-4, margin=1.0, lower=1.0, dc_scale=2e-7):
    """bv_arc (csrc/backvote_common.h) restated in fp32 numpy, operation for operation, with IEEE sqrt / quotient where the device
    has v_sqrt_f32 / v_rcp_f32 and atan2_np / acos_np for the approximations -> lo i32[P], cnt i32[P].  The keyword arguments are the screen's slack terms
    (the 8e-4 rad, the index of margin, the lowering of K, the 2e-7 of dc), there to show which of them the tuples can tell from 0."""
    w, x, y, tol, n, cmax, L2 = c["w"], c["x"], c["y"], c["tol"], c["n"].astype(np.int64), c["cmax"], c["L2"]
    dot = lambda p, q: VN._dot(p, q).astype(F)
    A, B, w2, rho2 = dot(w, x), dot(w, y), dot(w, w), dot(x, x)
    M = np.sqrt((A * A + B * B).astype(F)).astype(F)
    dc = (F(dc_scale) * (cmax + np.sqrt(rho2).astype(F)).astype(F)).astype(F)
    t2 = (tol * tol).astype(F)
    low = ((F(3e-4) * rho2).astype(F) + (F(4e-6) * ((w2 + rho2).astype(F) + t2).astype(F)).astype(F)).astype(F)
    low = (low + ((tol + dc).astype(F) * dc).astype(F)).astype(F)
    K = ((F(0.5) * ((w2 + rho2).astype(F) - t2).astype(F)).astype(F) - (F(lower) * low).astype(F)).astype(F)
    narrow = (n > 0) & (L2 >= F(1e-6)) & (M > F(1e-30))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.where(narrow, (K * (F(1) / np.where(narrow, M, F(1))).astype(F)).astype(F), F(0))
    none = narrow & (q > F(1.0005))
    some = narrow & ~none & (q > F(-0.9995))
    qq = np.where(some, np.minimum(q, F(1)), F(0))                         # (elsewhere the branch is not taken: any finite value)
    alpha = (acos_np(qq) + F(slack)).astype(F)
    phi = atan2_np(B, A)
    k = (n.astype(F) * F(0.159154943)).astype(F)
    ic, hw = (phi * k).astype(F), _fmaf(alpha, k, F(margin))
    i_lo = np.floor((ic - hw).astype(F)).astype(np.int64)
    i_hi = np.ceil((ic + hw).astype(F)).astype(np.int64)
    width = i_hi - i_lo + 1
    some &= width < n
    lo = np.where(some, np.mod(i_lo, np.maximum(n, 1)), 0)
    cnt = np.where(none, 0, np.where(some, width, n))
    return lo.astype(np.int32), cnt.astype(np.int32)


def arc_member(lo, cnt, n, nmax):
    """rotation i is in [lo, lo + cnt) modulo n -> bool[P, nmax]"""
    ii = np.arange(nmax)[None, :]
    nn = np.maximum(n, 1).astype(np.int64)[:, None]
    return (ii < n[:, None]) & (np.mod(ii - lo[:, None].astype(np.int64), nn) < cnt[:, None])


def arc_regimes(c, cnt):
    """how many tuples fall in each regime of the screen -> dict(full=, empty=, arc=)"""
    return dict(full=int((cnt == c["n"]).sum()), empty=int((cnt == 0).sum()), arc=int(((cnt > 0) & (cnt < c["n"])).sum()))
