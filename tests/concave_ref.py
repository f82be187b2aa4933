"""Restatement of csrc/concave.hip (include/cppf.h "Concave edges") without a device.  This file is the definition.
- concave_ref: vectorised numpy.  The nine window sums and the four Cramer determinants are int64 and exact; everything after them is
  fp64 in ONE stated operation order (numpy rounds every ufunc once, division and square root correctly, and never contracts);
- brute_ref: the same outputs by a loop per pixel with Python integers, explicit column-replacement determinants and fractions for
  the three quotients (what concave_ref itself is held to);
- numerator_bound: the largest magnitude a Cramer determinant can take at the caps, from the window geometry alone;
- the images the tests share (tabletop_scene: an analytic ray-cast table with upright cylinders)."""
from fractions import Fraction

import numpy as np

MAX_RADIUS, MAX_STEP = 8, 16
DEFAULTS = dict(radius=3, step=4, tol_mm=10, slope_permille=10, min_count=16, cos_max=float(np.cos(np.deg2rad(30.0))), span_max=0.08)


def check_args(H, W, fx, fy, cx, cy, radius, step, tol_mm, slope_permille, min_count, cos_max, span_max):
    """True where cppf_concave_edges accepts the call (pointers aside)"""
    return bool(H >= 1 and W >= 1 and H * W <= 1 << 24 and 1 <= radius <= MAX_RADIUS and 1 <= step <= MAX_STEP and 0 <= tol_mm <= 65535
                and 0 <= slope_permille <= 1000 and min_count >= 3 and -1.0 < cos_max < 1.0 and np.isfinite(span_max) and span_max > 0
                and np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0)


def numerator_bound(radius=MAX_RADIUS, dz_max=65535):
    """An upper bound on |D| and on the three numerator determinants for any window of that radius: every entry of a determinant's
    matrix is bounded from the window geometry (N pixels, A1 = sum |du|, A2 = sum du^2, A11 = sum |du dv|) and |dz| <= dz_max -- the
    difference of two uint16 depths, whatever tol_mm and slope_permille are -- and a 3x3 determinant is at most the permanent of its
    bounds.  Returns (bound on D, bound on the numerators)."""
    k = np.arange(-radius, radius + 1)
    du, dv = np.meshgrid(k, k)
    N, A1, A2, A11 = du.size, int(np.abs(du).sum()), int((du * du).sum()), int(np.abs(du * dv).sum())

    def permanent(m):
        return (m[0][0] * (m[1][1] * m[2][2] + m[1][2] * m[2][1]) + m[0][1] * (m[1][0] * m[2][2] + m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] + m[1][1] * m[2][0]))

    M = [[N, A1, A1], [A1, A2, A11], [A1, A11, A2]]
    rhs = [N * dz_max, A1 * dz_max, A1 * dz_max]
    num = max(permanent([[rhs[i] if j == col else M[i][j] for j in range(3)] for i in range(3)]) for col in range(3))
    return permanent(M), num


def live_ref(depth, valid=None):
    z = np.asarray(depth).astype(np.uint16).astype(np.int64)
    live = z > 0
    if valid is not None:
        live &= np.asarray(valid) != 0
    return z, live


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx] where that lies inside the frame, `fill` elsewhere"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def sums_ref(depth, valid, radius, tol_mm, slope_permille):
    """the nine window sums, int64 [9,H,W], in the order n, Su, Sv, Suu, Suv, Svv, Sz, Szu, Szv (zeros at dead pixels)"""
    z, live = live_ref(depth, valid)
    zl = np.where(live, z, 0)
    lim = int(tol_mm) + (int(slope_permille) * zl) // 1000
    S = np.zeros((9,) + z.shape, np.int64)
    for dv in range(-radius, radius + 1):
        for du in range(-radius, radius + 1):
            zq = _shift(zl, dv, du, 0)
            dz = zq - zl
            adm = live & (zq > 0) & (np.abs(dz) <= lim * max(abs(du), abs(dv), 1))
            dz = np.where(adm, dz, 0)
            a = adm.astype(np.int64)
            for k, t in enumerate((a, a * du, a * dv, a * du * du, a * du * dv, a * dv * dv, dz, dz * du, dz * dv)):
                S[k] += t
    return S


def cramer_ref(S):
    """(D, Nc, Na, Nb) int64 [H,W] of the normal equations [[n,Su,Sv],[Su,Suu,Suv],[Sv,Suv,Svv]] (c0, a, b) = (Sz, Szu, Szv)"""
    n, Su, Sv, Suu, Suv, Svv, Sz, Szu, Szv = S
    C00, C01, C02 = Suu * Svv - Suv * Suv, Suv * Sv - Su * Svv, Su * Suv - Suu * Sv
    C11, C12, C22 = n * Svv - Sv * Sv, Su * Sv - n * Suv, n * Suu - Su * Su
    D = n * C00 + Su * C01 + Sv * C02
    return D, C00 * Sz + C01 * Szu + C02 * Szv, C01 * Sz + C11 * Szu + C12 * Szv, C02 * Sz + C12 * Szu + C22 * Szv


def surface_ref(c, am, bm, u, v, fx, fy, cx, cy):
    """(N [..,3] unit or zeros, P [..,3], fit bool) from c = the fitted depth in metres and am, bm = its slopes in metres per pixel,
    fp64, in the stated order.  c = am = bm = 0 gives N = 0: no fit."""
    with np.errstate(all="ignore"):
        xu, yv = u - cx, v - cy
        pux, puy, puz = c / fx + (xu * am) / fx, (yv * am) / fy, am
        pvx, pvy, pvz = (xu * bm) / fx, c / fy + (yv * bm) / fy, bm
        nx, ny, nz = puy * pvz - puz * pvy, puz * pvx - pux * pvz, pux * pvy - puy * pvx
        px, py, pz = (xu * c) / fx, (yv * c) / fy, c
        flip = (nx * px + ny * py) + nz * pz > 0.0
        nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        fit = np.isfinite(ln) & (ln > 0.0)
        safe = np.where(fit, ln, 1.0)
        N = np.stack([np.where(fit, nx / safe, 0.0), np.where(fit, ny / safe, 0.0), np.where(fit, nz / safe, 0.0)], -1)
    return N, np.stack([px, py, pz], -1), fit


def concave_ref(depth, valid, fx, fy, cx, cy, radius=3, step=4, tol_mm=10, slope_permille=10, min_count=16,
                cos_max=DEFAULTS["cos_max"], span_max=0.08):
    """cppf_concave_edges: dict(edge u8[H,W], normal f64[H,W,3], counts i32[4] = {edge pixels, pixels with a fit, live pixels, 0})"""
    depth = np.asarray(depth)
    H, W = depth.shape
    fx, fy, cx, cy, cos_max, span_max = (np.float64(x) for x in (fx, fy, cx, cy, cos_max, span_max))
    assert check_args(H, W, fx, fy, cx, cy, radius, step, tol_mm, slope_permille, min_count, cos_max, span_max)
    z, live = live_ref(depth, valid)
    S = sums_ref(depth, valid, int(radius), int(tol_mm), int(slope_permille))
    D, Nc, Na, Nb = cramer_ref(S)
    has = live & (S[0] >= int(min_count)) & (D > 0)
    Dd = np.where(has, D, 1).astype(np.float64)
    c0, a, b = Nc.astype(np.float64) / Dd, Na.astype(np.float64) / Dd, Nb.astype(np.float64) / Dd
    c = np.where(has, (z.astype(np.float64) + c0) / 1000.0, 0.0)
    am, bm = np.where(has, a / 1000.0, 0.0), np.where(has, b / 1000.0, 0.0)
    v, u = np.mgrid[:H, :W].astype(np.float64)
    N, P, fit = surface_ref(c, am, bm, u, v, fx, fy, cx, cy)
    sm2 = span_max * span_max
    edge = np.zeros((H, W), bool)
    s = int(step)
    with np.errstate(all="ignore"):
        for dy, dx in ((0, s), (s, 0)):
            Nm, Np, Pm, Pp = _shift(N, -dy, -dx, 0.0), _shift(N, dy, dx, 0.0), _shift(P, -dy, -dx, 0.0), _shift(P, dy, dx, 0.0)
            both = _shift(fit, -dy, -dx, False) & _shift(fit, dy, dx, False)
            d, dn = Pp - Pm, Np - Nm
            span2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            cosn = (Nm[..., 0] * Np[..., 0] + Nm[..., 1] * Np[..., 1]) + Nm[..., 2] * Np[..., 2]
            conv = (d[..., 0] * dn[..., 0] + d[..., 1] * dn[..., 1]) + d[..., 2] * dn[..., 2]
            edge |= live & both & (span2 <= sm2) & (cosn < cos_max) & (conv < 0.0)
    counts = np.array([int(edge.sum()), int(fit.sum()), int(live.sum()), 0], np.int32)
    return dict(edge=edge.astype(np.uint8), normal=N, counts=counts)


# ------------------------------------------------------------------------------------------------------------------- brute force
def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _surface_one(c, am, bm, u, v, fx, fy, cx, cy):
    """surface_ref for one pixel in Python floats (IEEE fp64, one rounding per operation)"""
    import math
    xu, yv = float(u) - cx, float(v) - cy
    pu = (c / fx + (xu * am) / fx, (yv * am) / fy, am)
    pv = ((xu * bm) / fx, c / fy + (yv * bm) / fy, bm)
    n = [pu[1] * pv[2] - pu[2] * pv[1], pu[2] * pv[0] - pu[0] * pv[2], pu[0] * pv[1] - pu[1] * pv[0]]
    p = ((xu * c) / fx, (yv * c) / fy, c)
    if (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2] > 0.0:
        n = [-x for x in n]
    l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    ln = math.sqrt(l2) if l2 >= 0.0 and math.isfinite(l2) else float("nan")
    if not (math.isfinite(ln) and ln > 0.0):
        return None, p
    return tuple(x / ln for x in n), p


def brute_ref(depth, valid, fx, fy, cx, cy, radius=3, step=4, tol_mm=10, slope_permille=10, min_count=16,
              cos_max=DEFAULTS["cos_max"], span_max=0.08, track=None):
    """concave_ref's dict by the definition's own words, one pixel at a time.  track: a dict that receives max_abs_num, the largest
    |determinant| met"""
    depth = np.asarray(depth)
    H, W = depth.shape
    fx, fy, cx, cy, cos_max, span_max = (float(x) for x in (fx, fy, cx, cy, cos_max, span_max))
    z = [[int(x) for x in row] for row in depth.astype(np.uint16)]
    live = [[z[y][x] > 0 and (valid is None or bool(valid[y][x])) for x in range(W)] for y in range(H)]
    surf = [[(None, None)] * W for _ in range(H)]
    biggest = 0
    for y in range(H):
        for x in range(W):
            if not live[y][x]:
                continue
            z0 = z[y][x]
            lim = tol_mm + (slope_permille * z0) // 1000
            rows = []
            for dv in range(-radius, radius + 1):
                for du in range(-radius, radius + 1):
                    yy, xx = y + dv, x + du
                    if 0 <= yy < H and 0 <= xx < W and live[yy][xx] and abs(z[yy][xx] - z0) <= lim * max(abs(du), abs(dv), 1):
                        rows.append((1, du, dv, z[yy][xx] - z0))
            if len(rows) < min_count:
                continue
            M = [[sum(r[i] * r[j] for r in rows) for j in range(3)] for i in range(3)]
            rhs = [sum(r[i] * r[3] for r in rows) for i in range(3)]
            D = _det3(M)
            nums = [_det3([[rhs[i] if j == col else M[i][j] for j in range(3)] for i in range(3)]) for col in range(3)]
            biggest = max(biggest, abs(D), *(abs(t) for t in nums))
            if D <= 0:
                continue
            c0, a, b = (float(Fraction(t, D)) for t in nums)
            surf[y][x] = _surface_one((float(z0) + c0) / 1000.0, a / 1000.0, b / 1000.0, x, y, fx, fy, cx, cy)
    if track is not None:
        track["max_abs_num"] = biggest
    edge, normal = np.zeros((H, W), np.uint8), np.zeros((H, W, 3), np.float64)
    sm2 = span_max * span_max
    for y in range(H):
        for x in range(W):
            if surf[y][x][0] is not None:
                normal[y, x] = surf[y][x][0]
            if not live[y][x]:
                continue
            for dy, dx in ((0, step), (step, 0)):
                if not (0 <= y - dy and y + dy < H and 0 <= x - dx and x + dx < W):
                    continue
                (nm, pm), (np_, pp) = surf[y - dy][x - dx], surf[y + dy][x + dx]
                if nm is None or np_ is None:
                    continue
                d = [pp[k] - pm[k] for k in range(3)]
                dn = [np_[k] - nm[k] for k in range(3)]
                if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= sm2 and (nm[0] * np_[0] + nm[1] * np_[1]) + nm[2] * np_[2] < cos_max
                        and (d[0] * dn[0] + d[1] * dn[1]) + d[2] * dn[2] < 0.0):
                    edge[y, x] = 1
    n_fit = sum(surf[y][x][0] is not None for y in range(H) for x in range(W))
    counts = np.array([int(edge.sum()), n_fit, sum(map(sum, live)), 0], np.int32)
    return dict(edge=edge, normal=normal, counts=counts)


# ------------------------------------------------------------------------------------------------------------------- images
def planar_image(seed, H=24, W=31, holes=0.08):
    """piecewise-planar depth rounded to millimetres: up to three planes z = z0 + gx x + gy y, the nearest at each pixel wins (so they
    meet in creases and steps), some pixels dead; returns (depth u16[H,W], valid u8[H,W] or None)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    z = np.full((H, W), np.inf)
    for _ in range(int(rng.integers(1, 4))):
        z0, gx, gy = rng.uniform(500, 1500), rng.uniform(-12, 12), rng.uniform(-12, 12)
        z = np.minimum(z, z0 + gx * (x - W / 2) + gy * (y - H / 2))
    d = np.clip(np.rint(z + rng.integers(-1, 2, (H, W))), 1, 65535).astype(np.uint16)
    d[rng.random((H, W)) < holes] = 0
    valid = (rng.random((H, W)) < 0.93).astype(np.uint8) if seed % 2 else None
    return d, valid


TABLE_POINT, TABLE_CYLINDERS = (0.0, 0.15, 1.0), ((-0.15, 0.0, 0.04, 0.12), (0.0, -0.1, 0.035, 0.2), (0.072, -0.1, 0.035, 0.15),
                                                  (0.2, 0.1, 0.05, 0.08))


def tabletop_scene(tilt_deg, intrinsics, H=480, W=640, point=TABLE_POINT, cylinders=TABLE_CYLINDERS):
    """An analytic tabletop in frame coordinates (x right, y down, z forward): a table plane through `point` with up = (0, -cos t,
    -sin t) and upright cylinders (x, z on the table, radius, height).  Rays through the integer pixel coordinates are cast in fp64;
    returns (depth u16[H,W] = rint(1000 z), owner i32[H,W]: cylinder index, len(cylinders) for the table, -1 for nothing)."""
    K = np.asarray(intrinsics, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    t = np.deg2rad(tilt_deg)
    up = np.array([0.0, -np.cos(t), -np.sin(t)])
    ex = np.array([1.0, 0.0, 0.0])
    ez = np.cross(up, ex)                                                     # the table's second in-plane axis: away from the camera
    o = np.asarray(point, np.float64)
    v, u = np.mgrid[:H, :W].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)       # z = the ray parameter
    with np.errstate(all="ignore"):
        best = (o @ up) / (ray @ up)
    best = np.where(np.isfinite(best) & (best > 0), best, np.inf)
    owner = np.where(np.isfinite(best), len(cylinders), -1).astype(np.int32)
    rx, rz, ry = ray @ ex, ray @ ez, ray @ up                                  # the ray in table coordinates (origin: the camera)
    cam = -o
    ox, oz, oy = cam @ ex, cam @ ez, cam @ up
    for k, (px, pz, rad, h) in enumerate(cylinders):
        A, B, Cc = rx * rx + rz * rz, 2 * ((ox - px) * rx + (oz - pz) * rz), (ox - px) ** 2 + (oz - pz) ** 2 - rad * rad
        with np.errstate(all="ignore"):
            disc = B * B - 4 * A * Cc
            ts = (-B - np.sqrt(disc)) / (2 * A)                               # the near wall
            side = (disc >= 0) & (ts > 0) & (oy + ts * ry >= 0) & (oy + ts * ry <= h)
            tc = (h - oy) / ry                                                # the top cap
            cap = (tc > 0) & ((ox + tc * rx - px) ** 2 + (oz + tc * rz - pz) ** 2 <= rad * rad)
        tk = np.minimum(np.where(side, ts, np.inf), np.where(cap, tc, np.inf))
        owner = np.where(tk < best, k, owner)
        best = np.minimum(best, tk)
    depth = np.where(np.isfinite(best), np.rint(1000.0 * best), 0.0)
    owner = np.where((depth > 0) & (depth <= 65535), owner, -1).astype(np.int32)
    return np.where(owner >= 0, depth, 0).astype(np.uint16), owner
