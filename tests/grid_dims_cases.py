"""The vote grid's dims, int32((max - min) / res) + 1 (nocs/inference.py:194-195), at the edges of the division: the reference and
the clouds that the CPU and the device tests share (numpy only).

Reference, per axis: e = f32(h - l), r = f32(res), q = f32(f64(e) / f64(r)), dims = int(q) + 1 -- plain float64 arithmetic, independent
of every path under test.  The float64 quotient rounded to float32 IS the correctly rounded float32 quotient: rounding a quotient
twice is innocuous when the wide format has at least 2 p + 2 digits for the narrow one's p, and 53 >= 2 * 24 + 2 (Figueroa, "When is
double rounding innocuous?", 1995).  It is what numpy's float32 division and IEEE hardware division give, and what the host and
every device entry point must reproduce, because the host's dims choose the pipeline (tile class, capacity) that the device's dims
then run on.

Two mistakes are what performance work on such a line produces, and the cases are built to bite on both:
  reciprocal-multiply   int(f32(e * f32(1 / r))) + 1      (a division by a scalar turned into a multiplication)
  unrounded double      int(f64(e) / f64(r)) + 1          (the quotient truncated before it was rounded to float32)
For every resolution -- those of cppf_amd.config.CATEGORIES plus 2e-3 and 1.6e-3 -- and k in 1..399 the extents are f32(k) * r and
its neighbours out to +-3 ulp; the generator asserts that at least MIN_BITING of them differ from the reference under each mistake
(a condition on the inputs, met by the reference alone; BITING holds the counts it found).

A cloud is two points, l and h = l + e on one axis, with l zero, negative or positive and chosen so that the subtraction is exact:
the generator asserts f32(h - l) == e, so the edge under test is the one intended."""
import numpy as np

from cppf_amd.config import CATEGORIES

f32, f64 = np.float32, np.float64
RESOLUTIONS = sorted({float(f32(c.res)) for c in CATEGORIES.values()} | {float(f32(2e-3)), float(f32(1.6e-3))})
K_RANGE = range(1, 400)
ULPS = range(-3, 4)
MIN_BITING = 20


def ref_dims_axis(e, r):
    """the reference: the correctly rounded float32 quotient (through float64), truncated, plus one"""
    return int(f32(f64(f32(e)) / f64(f32(r)))) + 1


def recip_dims_axis(e, r):
    """mistake 1: multiply by the rounded reciprocal"""
    return int(f32(f32(e) * (f32(1.0) / f32(r)))) + 1


def double_dims_axis(e, r):
    """mistake 2: truncate the double quotient without rounding it to float32 first"""
    return int(f64(f32(e)) / f64(f32(r))) + 1


def reference(pc, res):
    """(corners f32[2,3], dims tuple) of a cloud, by the reference formula"""
    pc = np.asarray(pc, f32).reshape(-1, 3)
    lo, hi = pc.min(0), pc.max(0)
    return np.stack([lo, hi]), tuple(ref_dims_axis(f32(hi[j] - lo[j]), res) for j in range(3))


def _ulp(e):
    return f64(np.spacing(f32(e)))


def _step(e, d):
    for _ in range(abs(d)):
        e = np.nextafter(f32(e), f32(np.inf) if d > 0 else f32(-np.inf))
    return f32(e)


def _ends(e, kind):
    """(l, h) with f32(h - l) == e exactly: kind 0: l = 0; 1: l = -2^floor(log2 e) (h = e - 2^.. is exact: the operands are within a
    factor of two); 2: l > 0 a small multiple of e's ulp, so that l + e is a float32"""
    e = f32(e)
    if kind == 0:
        cands = [f32(0.0)]
    elif kind == 1:
        cands = [f32(-(2.0 ** np.floor(np.log2(f64(e)))))]
    else:
        cands = [f32(_ulp(e) * m) for m in (64, 16, 4, 2, 1)]
    for l in cands:
        h = f32(f64(l) + f64(e))
        if f64(h) == f64(l) + f64(e) and f32(h - l) == e:
            return l, h
    raise AssertionError(f"no exact end points for extent {e!r}, kind {kind}")


def _cloud(ends, swap):
    """two points: the minima in one, the maxima in the other (swap: which comes first)"""
    lo = np.array([l for l, _ in ends], f32)
    hi = np.array([h for _, h in ends], f32)
    return np.stack([hi, lo] if swap else [lo, hi])


def _build():
    cases, biting = [], {}
    i = 0
    for r in RESOLUTIONS:
        r32 = f32(r)
        n_recip = n_double = 0
        bites = []
        for k in K_RANGE:
            base = f32(f32(k) * r32)
            for d in ULPS:
                e = _step(base, d)
                want = ref_dims_axis(e, r32)
                br, bd = recip_dims_axis(e, r32) != want, double_dims_axis(e, r32) != want
                n_recip += br
                n_double += bd
                kind, axis = i % 3, (i // 3) % 3
                l, h = _ends(e, kind)
                assert f32(h - l) == e
                ends = [(f32(0.0), f32(0.0))] * 3
                ends[axis] = (l, h)
                pc = _cloud(ends, swap=(i // 9) % 2 == 1)
                dims = [1, 1, 1]
                dims[axis] = want
                cases.append(dict(name=f"r{r:g}_k{k}_{d:+d}ulp_axis{axis}_l{'0-+'[kind]}", pc=pc, res=float(r32), dims=tuple(dims),
                                  biting=bool(br or bd), by_value=False))
                if br or bd:
                    bites.append(e)
                i += 1
        assert n_recip >= MIN_BITING and n_double >= MIN_BITING, (r, n_recip, n_double)
        biting[float(r32)] = dict(recip=int(n_recip), double=int(n_double), extents=bites)
        # the three axes of one cloud carrying three different edges, each with its own kind of minimum
        for t in range(0, len(bites) - 2, 3):
            ends = [_ends(bites[t + j], (t // 3 + j) % 3) for j in range(3)]
            assert all(f32(h - l) == bites[t + j] for j, (l, h) in enumerate(ends))
            cases.append(dict(name=f"r{r:g}_three_edges_{t // 3}", pc=_cloud(ends, swap=t % 2 == 1), res=float(r32),
                              dims=tuple(ref_dims_axis(bites[t + j], r32) for j in range(3)), biting=True, by_value=False))
    for r in RESOLUTIONS:
        one = np.array([[0.25, -0.5, 1.0]], f32)
        cases.append(dict(name=f"r{r:g}_single_point", pc=one, res=r, dims=(1, 1, 1), biting=False, by_value=False))
        cases.append(dict(name=f"r{r:g}_all_equal", pc=np.repeat(one, 7, 0), res=r, dims=(1, 1, 1), biting=False, by_value=False))
        den = f32(3e-42)                                      # a denormal extent: the quotient is denormal or tiny, dims 1
        assert 0 < den < np.finfo(f32).tiny
        cases.append(dict(name=f"r{r:g}_denormal_extent", pc=np.array([[0, 0, 0], [den, 0, den]], f32), res=r, dims=(1, 1, 1),
                          biting=False, by_value=False))
        e = biting[float(f32(r))]["extents"][0]
        # -0.0 and +0.0 both present as the minimum: either may be reported as the corner (min is free to return either zero)
        pc = np.array([[0.0, -0.0, e], [-0.0, 0.0, 0.0], [e, e, -0.0]], f32)
        d = ref_dims_axis(e, r)
        cases.append(dict(name=f"r{r:g}_signed_zero_minimum", pc=pc, res=r, dims=(d, d, d), biting=True, by_value=True))
    for c in cases:
        c["corners"] = np.stack([c["pc"].min(0), c["pc"].max(0)])
        assert reference(c["pc"], c["res"])[1] == c["dims"], c["name"]
    return cases, biting


CASES, BITING = _build()
DEVICE_CASES = [c for j, c in enumerate(CASES) if c["biting"] or j % 16 == 0]     # thinned for the device: every biting case stays


def corners_equal(got, want, by_value):
    """bit for bit, or by value where both zeros are present as an extreme"""
    got, want = np.asarray(got, f32).reshape(want.shape), np.asarray(want, f32)
    return bool(np.array_equal(got, want)) if by_value else bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))


# ---- reduction placement (device only): where in the cloud the minimum and the maximum sit
PLACEMENT_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def placement_cases(block):
    """clouds of N points whose minimum and maximum sit, independently, at index 0, 63, 64, N - 1 and the last index of the first
    trip of a block of `block` threads; everything else strictly inside the interval.  The extent on every axis is a biting
    one (res 0.004), so a lost lane, wave or second trip of the reduction changes the corner or the dims.  -> list of cases"""
    r = f32(0.004)
    ext = BITING[float(r)]["extents"]
    rng = np.random.default_rng(17)
    out = []
    for N in PLACEMENT_N:
        spots = sorted({p for p in (0, 63, 64, N - 1, block - 1) if 0 <= p < N})
        for i_lo in spots:
            for i_hi in spots:
                if i_lo == i_hi and N > 1:
                    continue
                t = len(out)
                ends = [_ends(ext[(t + 5 * j) % len(ext)], 1) for j in range(3)]          # l < 0 < h on every axis
                lo = np.array([l for l, _ in ends], f32)
                hi = np.array([h for _, h in ends], f32)
                if N == 1:
                    hi = lo
                pc = (lo + (hi - lo) * rng.uniform(0.25, 0.75, (N, 3))).astype(f32)
                assert N < 3 or ((pc > lo) & (pc < hi)).all()
                pc[i_hi] = hi
                pc[i_lo] = lo
                corners, dims = reference(pc, r)
                assert np.array_equal(corners, np.stack([lo, hi]))
                out.append(dict(name=f"N{N}_min{i_lo}_max{i_hi}", pc=pc, res=float(r), dims=dims, corners=corners, by_value=False))
    return out
