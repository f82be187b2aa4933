"""The back-vote boundary family: pairs whose vote circle has ONE chosen sample at a chosen distance from the centre, a relative
`eps` either side of tol, so that the acceptance of voting.py:101 is decided in the last bits -- where the two shortcuts of
csrc/backvote_common.h (the stage-1 screen of backvote_body / backvote_multi_kernel, the rotation arc of bv_arc) have to be supersets
of the exhaustive loop.  Shared by tests/test_backvote_cases_cpu.py (conditions on the inputs, and the proof that a margin-free
shortcut loses pairs on them) and tests/test_gpu_backvote_edges.py (the device against oracle.backvote).  Not a test module.

Construction, in fp64, rounded to fp32 at the end.  Every pair has its own two points (cloud [a_0, b_0, a_1, b_1, ..], idx (2k, 2k+1)).
With the reference's frame of a unit axis u (voting.py:27: x^ from co = (0, -u_z, u_y), fallback (-u_y, u_x, 0); y^ = x^ x u) and
e_t = cos(2 pi t / n) x^ + sin(2 pi t / n) y^, n the pair's adaptive rotation count:
    s = gt - R d,  cc = s - nu e_t,  a = cc + mu u,  b = a - L u,  outputs = (mu, nu),  mu ~ U(-0.1, 0.1)
so that sample t of the pair lies at R from gt.  Groups (column `group` of the case):
  MAIN      R = tol (1 + eps) over  nu x L x t x d x eps  (NU_RES, L_MAIN, {0, 1, n // 2, n - 1}, D_KINDS, EPS), two pairs each: a
            random u and u = +- a coordinate axis (+-x takes the `co` fallback)
  L_1E3     L = 1e-3 (1 -+ 1e-3): the L2 >= 1e-6 switch of bv_arc;   L_TINY  L around 3.2e-7: the L2 >= 1e-13 switch of stage 1
  INSIDE    R = tol {0.5, 0.9}: several rotations pass, also on both sides of the wrap n - 1 -> 0; the first in INDEX order wins
  AXIS      gt on the circle's axis, displaced sideways by {0, 1e-9, 1e-6, 1e-3} tol, sqrt(h^2 + nu^2) = tol (1 + eps): M at its
            1e-30 cut, c near +-1
  TOUCH     d radially outward, eps = 0, every nu, the touching point on and between sample angles: the arc's half-width -> 0
The grid is 10 cells larger than everything on every side: no face is near (the face rule has its own case, ref_vote_cases.shell_case).
"""
import numpy as np

from oracle import voting_numpy as VN

F, D = np.float32, np.float64
TWO_PI = 2 * np.pi
MAIN, L_1E3, L_TINY, INSIDE, AXIS, TOUCH = range(6)
GROUP_NAMES = ("main", "L~1e-3", "L~3.2e-7", "inside", "near-axis", "touching")
EPS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3, 1e-2, -1e-2)
NU_RES = (1.5 / TWO_PI, 3.7 / TWO_PI, 1.0, 2.7, 5.0, 12.0, 30.0, 75.0)      # nu / res: rotation counts 1 .. n_rots
L_MAIN = (2e-3, 0.03, 0.2)
L_SWITCH_1E3 = (1e-3 * (1 - 1e-3), 1e-3 * (1 + 1e-3))
L_SWITCH_TINY = tuple(3.2e-7 * m for m in (0.7, 0.95, 1.0, 1.05, 1.4))
D_KINDS = ("out", "in", "+u", "-u", "diag")
CENTRES = ((0.1, -0.05, 0.7), (1.5, -1.2, 3.0), (3.0, -2.0, 8.0))
RESOLUTIONS = (2e-3, 4e-3, 0.03)
ROTATIONS = (7, 72, 120)                      # 120: no LDS table, the rot_cs path
# res = 0.03 runs at n_rots = 7 only: at 72 and 120 rotations its -1e-5 class is accepted to 90 .. 92 % (eps tol = 9e-7 is above what
# the 1e-7 regularisers and fp32 rounding move nine samples in ten by), and the class no longer straddles as
# tests/test_backvote_cases_cpu.py demands of every configuration that the device test runs.
CONFIGS = [(g, r, n) for g in CENTRES for r in RESOLUTIONS for n in ROTATIONS if r != 0.03 or n == 7]


def rot_count(nu, res, n_rots):
    """voting.py:97 on the fp32 values: min(int(odist / res * (2 * M_PI)), n_rots)"""
    return VN._n_rots(np.asarray(nu, F), F(res), n_rots, True)


def frames(u):
    """fp64 x^, y^ of unit axes u[P,3] (voting.py:27 without the 1e-7 regularisers)"""
    co = np.stack([np.zeros(len(u)), -u[:, 2], u[:, 1]], -1)
    alt = np.stack([-u[:, 1], u[:, 0], np.zeros(len(u))], -1)
    co = np.where((np.linalg.norm(co, axis=-1) < 1e-7)[:, None], alt, co)
    x = co / np.linalg.norm(co, axis=-1, keepdims=True)
    return x, np.cross(x, u)


def family(gt, res, n_rots, seed=0, extras=True):
    """-> case dict: points f32[2P,3], outputs f32[P,2], idx i32[P,2], corner f32[3], dims i32[3], gt f32[3], tol, res, n_rots and,
    per pair, group, eps (nan outside MAIN / AXIS / the L switches), n (rotation count) and t (the target rotation)"""
    rng = np.random.default_rng(seed)
    tol = float(F(3 * res))
    gt = np.asarray(gt, F).astype(D)
    rows = []                                  # (group, nu / res, L, t (TOUCH: -10 - k), d kind, R / tol, eps, side)

    def grid(group, nus, Ls, ends_only, ds, factors):
        for nu in nus:
            n = int(rot_count((nu * res), res, n_rots))
            ts = sorted({0, n - 1} if ends_only else {0, min(1, n - 1), n // 2, n - 1})      # the distinct ones
            for L in Ls:
                for t in ts:
                    for d in ds:
                        for eps, f in factors:
                            rows.append((group, nu, L, t, d, f, eps, 0.0))

    by_eps = [(e, 1.0 + e) for e in EPS]
    all_d = range(len(D_KINDS))
    grid(MAIN, NU_RES, L_MAIN, False, all_d, by_eps)
    if extras:
        few = [(e, 1.0 + e) for e in (0.0, 1e-5, -1e-5, 1e-3, -1e-3)]
        grid(L_1E3, (2.7, 12.0), L_SWITCH_1E3, True, all_d, few)
        grid(L_TINY, (2.7, 12.0), L_SWITCH_TINY, True, all_d, few)
        grid(INSIDE, (1.0, 2.7, 12.0, 30.0), L_MAIN, True, all_d, [(np.nan, 0.5), (np.nan, 0.9)])
        for nu in NU_RES[:4]:                                              # nu < tol: the axis comes within tol of the circle
            for sign in (0, 1):                                            # d kind 2 / 3: gt on the +u / -u side
                for side in (0.0, 1e-9, 1e-6, 1e-3):
                    for e, f in by_eps:
                        rows.append((AXIS, nu, 0.03, 0, 2 + sign, f, e, side))
        for nu in NU_RES:
            for k in range(16):                                            # eighths of the circle, then the angles between samples
                rows.append((TOUCH, nu, 0.03, -10 - k, 0, 1.0, 0.0, 0.0))
    rows = [r + (kind,) for r in rows for kind in (0, 1)]                  # a random u, then an axis u
    P = len(rows)
    group = np.array([r[0] for r in rows])
    nu = (np.array([r[1] for r in rows]) * res).astype(F).astype(D)
    L = np.array([r[2] for r in rows])
    tcode = np.array([r[3] for r in rows])
    dk = np.array([r[4] for r in rows])
    R = tol * np.array([r[5] for r in rows])
    eps = np.array([r[6] for r in rows])
    side = np.array([r[7] for r in rows])
    kind = np.array([r[8] for r in rows])
    n = rot_count(nu, res, n_rots)
    nn = np.maximum(n, 1)
    t = np.maximum(tcode, 0).astype(D)
    k = -10 - tcode
    t = np.where(tcode <= -10, np.where(k < 8, np.floor(k * nn / 8.0), np.floor((k - 8) * nn / 8.0) + 0.5), t)
    u = rng.normal(size=(P, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])[np.arange(P) % 6]
    u = np.where((kind == 1)[:, None], axes, u)
    # a - b = L u is snapped to a binary grid that fp32 holds at these coordinates (below 16: 2^-20; the L ~ 3.2e-7 group: 2^-24)
    # and u, L are taken from the snapped vector: b = a - delta is then exact in fp32 and the kernels see the direction the
    # construction used.  (Unsnapped, rounding a and b turns a 2e-3 long pair by 5e-4 rad at coordinates of 8, and moves its
    # samples by 1e-2 tol: no eps class below that would be decided by eps.)
    quantum = np.where(group == L_TINY, 2.0 ** -24, 2.0 ** -20)[:, None]
    delta = np.round(L[:, None] * u / quantum) * quantum
    L = np.linalg.norm(delta, axis=-1)
    u = delta / L[:, None]
    x, y = frames(u)
    ang = TWO_PI * t / nn
    e = np.cos(ang)[:, None] * x + np.sin(ang)[:, None] * y
    d = np.select([(dk == 0)[:, None], (dk == 1)[:, None], (dk == 2)[:, None], (dk == 3)[:, None]], [e, -e, u, -u],
                  (e + u) / np.sqrt(2.0))
    cc = gt - R[:, None] * d - nu[:, None] * e
    ax = group == AXIS                                                     # gt = cc +- h u + side tol x^, |(h, nu)| = R
    h = np.sqrt(np.maximum(R * R - nu * nu, 0.0)) * np.where(dk == 2, 1.0, -1.0)
    cc = np.where(ax[:, None], gt - h[:, None] * u - (side * tol)[:, None] * x, cc)
    mu = rng.uniform(-0.1, 0.1, P).astype(F).astype(D)
    a = cc + mu[:, None] * u
    a = a.astype(F).astype(D)
    points = np.stack([a, a - delta], 1).reshape(2 * P, 3).astype(F)
    idx = np.arange(2 * P, dtype=np.int32).reshape(P, 2)
    lo = np.minimum(points.min(0).astype(D), gt - tol) - 10 * res
    hi = np.maximum(points.max(0).astype(D), gt + tol) + 10 * res
    corner = lo.astype(F)
    dims = (np.ceil((hi - corner.astype(D)) / res) + 2).astype(np.int32)
    keep = n > 0                                                           # (nu / res * 2 pi < 1: no rotation, nothing to probe)
    c = dict(points=points, outputs=np.stack([mu, nu], -1).astype(F), idx=idx, corner=corner, dims=dims, gt=gt.astype(F), tol=tol,
             res=float(res), n_rots=int(n_rots), group=group, eps=eps, n=n, t=t)
    assert keep.all()
    return c


def reorder(c, order):
    """the same case with its pair list in another order (the points stay)"""
    d = dict(c)
    for k in ("outputs", "idx", "group", "eps", "n", "t"):
        d[k] = np.ascontiguousarray(c[k][order])
    return d


def centres(c, n_centers=32, seed=0):
    """cppf_backvote_multi's centres: gt, gt displaced by +-{1e-7, 1e-6, 1e-5, 1e-4} tol along x and along a diagonal, the rest
    random inside the cloud's box -> f32[n_centers,3]"""
    gt, tol = c["gt"].astype(D), c["tol"]
    out = [gt]
    for dirn in (np.array([1.0, 0.0, 0.0]), np.ones(3) / np.sqrt(3.0)):
        for s in (1e-7, 1e-6, 1e-5, 1e-4):
            out += [gt + s * tol * dirn, gt - s * tol * dirn]
    rng = np.random.default_rng(seed + 1)
    lo, hi = c["points"].min(0).astype(D), c["points"].max(0).astype(D)
    while len(out) < 32:
        out.append(rng.uniform(lo, hi))
    return np.asarray(out[:n_centers], F)


# ------------------------------------------------------------------ the exhaustive loop, every rotation kept
def exhaustive(O, c, gt=None):
    """The reference's loop (voting.py:97-110) in its fp32 arithmetic, as oracle/voting_numpy.backvote, WITHOUT the break:
    -> passing bool[P, n_rots] (rotation i of pair p passes :101 and :103-107; False for i >= n) and dist f32[P, n_rots]
    (the left side of :101, inf for i >= n), plus the fp32 frame (a, ab, x, y, cc, nr) the shortcuts start from"""
    gx, gy, gz = (int(v) for v in c["dims"])
    P = c["idx"].shape[0]
    mu, nu = c["outputs"][:, 0].astype(F), c["outputs"][:, 1].astype(F)
    a, ab, x, y, live = VN._frame(c["points"], c["idx"], nu)
    cc = (a - (ab * mu[:, None]).astype(F)).astype(F)
    nr = np.where(live, VN._n_rots(nu, c["res"], c["n_rots"], True), 0)
    cr, g0 = np.asarray(c["corner"], F), np.asarray(c["gt"] if gt is None else gt, F)
    passing = np.zeros((P, c["n_rots"]), bool)
    dist = np.full((P, c["n_rots"]), np.inf, F)
    for n in np.unique(nr[nr > 0]):
        r = np.nonzero(nr == n)[0]
        cs = np.array([O.rot_cs(i, int(n)) for i in range(int(n))], F)
        off = ((cs[None, :, :1] * x[r, None, :]).astype(F) + (cs[None, :, 1:] * y[r, None, :]).astype(F)).astype(F)
        pc = (cc[r, None, :] + off).astype(F)
        dd = VN._length((pc - g0).astype(F))
        g = ((pc - cr).astype(F) / F(c["res"])).astype(F)
        outside = (g < 0).any(-1) | (g[..., 0] >= F(gx - 1)) | (g[..., 1] >= F(gy - 1)) | (g[..., 2] >= F(gz - 1))
        nz = (off != 0).any(-1)                                            # (a survivor has a non-zero offset, nocs/inference.py:230)
        passing[r[:, None], np.arange(int(n))[None, :]] = ~(dd > F(c["tol"])) & ~outside & nz
        dist[r[:, None], np.arange(int(n))[None, :]] = dd
    return passing, dist, dict(a=a, ab=ab, x=x, y=y, cc=cc, nr=nr)


# ------------------------------------------------------------------ the two shortcuts, restated
def screen(c, fr, margins=True, gt=None):
    """The stage-1 screen of backvote_body (csrc/pose_tail.hip) / backvote_multi_kernel (csrc/scene_multi.hip) in fp32 numpy, with
    IEEE sqrt and division where the device has v_sqrt / v_rcp -> bool[P]: the pair goes on to stage 2.  margins=False: every slack
    term (2e-4 mag, 1e-6, squash, the 0.9999 of the rotation-count test) is zero."""
    p = c["points"].astype(F)
    pa, pb = p[c["idx"][:, 0]], p[c["idx"][:, 1]]
    mu, nu = c["outputs"][:, 0].astype(F), c["outputs"][:, 1].astype(F)
    g0, tol, res = np.asarray(c["gt"] if gt is None else gt, F), F(c["tol"]), F(c["res"])
    m = F(1.0) if margins else F(0.0)
    dd = (pa - pb).astype(F)
    L2 = VN._dot(dd, dd).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / (np.sqrt(L2).astype(F) + F(1e-7))).astype(F)
        u = (dd * inv[:, None]).astype(F)
        cc = (pa - (u * mu[:, None]).astype(F)).astype(F)
        w = (g0 - cc).astype(F)
        h, w2, rho = VN._dot(w, u).astype(F), VN._dot(w, w).astype(F), np.abs(nu)
        r = np.sqrt(np.maximum(w2 - h * h, F(0))).astype(F)
        dist = np.sqrt((r - rho) * (r - rho) + h * h).astype(F)
        mag = (np.sqrt(w2) + rho + tol).astype(F)
        squash = ((rho + np.abs(mu)) * F(2e-7) * inv).astype(F)
        enough = (nu * (F(1.0) / res) * F(6.2831855)).astype(F) >= (F(0.9999) if margins else F(1.0))
        far = dist > (tol + m * (F(2e-4) * mag + F(1e-6) + squash)).astype(F)
    # (nearly) coincident points, L2 < 1e-13: no screen, every pair with a rotation goes on
    return np.where(L2 >= F(1e-13), enough & ~far, fr["nr"] > 0)


def arc(c, fr, margins=True, gt=None):
    """bv_arc (csrc/backvote_common.h) in fp64 with exact acos / atan2, from the fp32 frame -> member bool[P, n_rots]: rotation i
    of pair p is walked.  margins=False: no lowering of K, cuts at c > 1 and c > -1, no 8e-4 rad, no index of margin."""
    P, n_rots = c["idx"].shape[0], c["n_rots"]
    p = c["points"].astype(F)
    dd = (p[c["idx"][:, 0]] - p[c["idx"][:, 1]]).astype(F)
    L2 = VN._dot(dd, dd).astype(F)
    g0, tol = np.asarray(c["gt"] if gt is None else gt, F).astype(D), float(F(c["tol"]))
    x, y, w = fr["x"].astype(D), fr["y"].astype(D), g0 - fr["cc"].astype(D)
    n = fr["nr"].astype(np.int64)
    m = 1.0 if margins else 0.0
    A, B, w2, rho2 = (w * x).sum(-1), (w * y).sum(-1), (w * w).sum(-1), (x * x).sum(-1)
    M = np.sqrt(A * A + B * B)
    dc = 2e-7 * (np.abs(fr["cc"].astype(D)).max(-1) + np.sqrt(rho2))          # what rounding cc + offset can add to a distance
    K = 0.5 * (w2 + rho2 - tol * tol) - m * (3e-4 * rho2 + 4e-6 * (w2 + rho2 + tol * tol) + (tol + dc) * dc)
    ii = np.arange(n_rots)[None, :]
    member = ii < n[:, None]                                               # the whole circle
    narrow = (n > 0) & (L2 >= F(1e-6)) & (M > 1e-30)
    with np.errstate(divide="ignore", invalid="ignore"):
        cq = np.where(narrow, K / np.where(M > 0, M, 1.0), 0.0)
        none = narrow & (cq > 1.0 + m * 5e-4)
        some = narrow & ~none & (cq > -1.0 + m * 5e-4)
        alpha = np.arccos(np.clip(cq, -1.0, 1.0)) + m * 8e-4
        kk = n / TWO_PI
        ic, hw = np.arctan2(B, A) * kk, alpha * kk + m
        i_lo, i_hi = np.floor(ic - hw).astype(np.int64), np.ceil(ic + hw).astype(np.int64)
    cnt = i_hi - i_lo + 1
    some &= cnt < n
    rel = np.mod(ii - i_lo[:, None], np.maximum(n, 1)[:, None])            # position of rotation i on the walk from i_lo
    member = np.where(none[:, None], False, np.where(some[:, None], member & (rel < cnt[:, None]), member))
    return member, np.where(none, 0, np.where(some, cnt, n))
