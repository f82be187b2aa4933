"""Shared test code for the training views (cppf_amd/meshes.py, csrc/raster.hip):

- raster_ref: a numpy restatement of cppf_raster_depth with the fp32 operation order of include/cppf.h, bit for bit;
- ray_cast: an independent fp64 ray caster (Moller-Trumbore) through the same pinhole camera;
- procedural meshes written as OBJ text with outward CCW winding: box, capped cylinder with a neck, UV sphere, one large triangle;
- depth_points_ref / sample_ref: numpy restatements of cppf_depth_points and of MeshViewSampler.sample given its draws."""
import numpy as np

from cppf_amd import meshes as M

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------- rasteriser
def _transform(v, model):
    m = np.asarray(model, np.float64)
    c = [((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3)]
    return c[0].astype(f32), c[1].astype(f32), -(c[2].astype(f32))


def _clip(a, b, zn):
    t = (a[2] - zn) / (a[2] - b[2])
    return (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), zn)


def setup_ref(vertices, faces, model, fx, fy, W, H, znear, cull):
    """the primitives of include/cppf.h steps 1-5: list of (x[3], y[3], i[3], (c0, r0, c1, r1))"""
    X, Y, D = _transform(np.asarray(vertices, np.float64), model)
    zn = f32(znear)
    p00, p11 = f32(2.0 * fx / W), f32(2.0 * fy / H)
    hw, hh = f32(0.5) * f32(W), f32(0.5) * f32(H)
    one = f32(1.0)
    prims = []
    for tri in np.asarray(faces):
        v = [(X[k], Y[k], D[k]) for k in tri]
        poly = []
        for k in range(3):
            a, b = v[k], v[(k + 1) % 3]
            ia, ib = a[2] >= zn, b[2] >= zn
            if ia:
                poly.append(a)
            if ia and not ib:
                poly.append(_clip(a, b, zn))
            if not ia and ib:
                poly.append(_clip(b, a, zn))
        fans = [(0, 1, 2)] if len(poly) >= 3 else []
        if len(poly) == 4:
            fans.append((0, 2, 3))
        for fan in fans:
            q = [poly[k] for k in fan]
            x = [((p00 * p[0]) / p[2] + one) * hw for p in q]
            y = [((p11 * p[1]) / p[2] + one) * hh for p in q]
            iv = [one / p[2] for p in q]
            A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
            if not cull and A < 0:
                x[1], x[2], y[1], y[2], iv[1], iv[2] = x[2], x[1], y[2], y[1], iv[2], iv[1]
                A = -A
            if not A > 0:
                continue
            cl = lambda val, hi: min(max(val, f32(-1)), f32(hi))
            c0 = max(0, int(np.floor(cl(min(x) - one, W))))
            c1 = min(W - 1, int(np.floor(cl(max(x) + one, W))))
            j0 = max(0, int(np.floor(cl(min(y) - one, H))))
            j1 = min(H - 1, int(np.floor(cl(max(y) + one, H))))
            if c0 <= c1 and j0 <= j1:
                prims.append((x, y, iv, (c0, H - 1 - j1, c1, H - 1 - j0)))
    return prims


def _tl(ax, ay, bx, by):
    dy, dx = by - ay, bx - ax
    return dy < 0 or (dy == 0 and dx < 0)


def raster_ref(vertices, faces, model, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, znear=M.ZNEAR, cull=True):
    """include/cppf.h cppf_raster_depth in numpy fp32: depth f32[H,W], background 0"""
    depth = np.full((H, W), np.inf, f32)
    for x, y, iv, (c0, r0, c1, r1) in setup_ref(vertices, faces, model, fx, fy, W, H, znear, cull):
        cc, rr = np.meshgrid(np.arange(c0, c1 + 1), np.arange(r0, r1 + 1))
        px = cc.astype(f32) + f32(0.5)
        py = (H - 1 - rr).astype(f32) + f32(0.5)
        E = lambda a, b: (x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a])
        w0, w1, w2 = E(1, 2), E(2, 0), E(0, 1)
        inside = lambda w, a, b: (w > 0) | ((w == 0) & _tl(x[a], y[a], x[b], y[b]))
        cov = inside(w0, 1, 2) & inside(w1, 2, 0) & inside(w2, 0, 1)
        if not cov.any():
            continue
        d = ((w0 + w1) + w2) / ((w0 * iv[0] + w1 * iv[1]) + w2 * iv[2])
        sub = depth[r0:r1 + 1, c0:c1 + 1]
        np.minimum(sub, np.where(cov, d, np.inf).astype(f32), out=sub)
    depth[np.isinf(depth)] = 0
    return depth


def ray_cast(vertices, faces, model, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, cull=True, chunk=4096, pixels=None):
    """fp64 Moller-Trumbore through every pixel centre: depth f64[H,W] (0 = miss).  Front face: CCW seen from the camera.
    pixels: flat indices (row * W + column) -> the depths of those pixels only, as a vector"""
    m = np.asarray(model, np.float64)
    v = np.asarray(vertices, np.float64) @ m[:3, :3].T + m[:3, 3]
    tri = v[np.asarray(faces)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    if cull:
        keep = np.einsum("ij,ij->i", np.cross(e1, e2), v0) < 0
        v0, e1, e2 = v0[keep], e1[keep], e2[keep]
    cc, rr = np.meshgrid(np.arange(W), np.arange(H))
    ndx = 2 * (cc.ravel() + 0.5) / W - 1
    ndy = 2 * (H - rr.ravel() - 0.5) / H - 1
    dirs = np.stack([ndx / (2 * fx / W), ndy / (2 * fy / H), -np.ones_like(ndx)], -1)
    if pixels is not None:
        dirs = dirs[np.asarray(pixels)]
    out = np.zeros(dirs.shape[0])
    for s in range(0, dirs.shape[0], chunk):
        dv = dirs[s:s + chunk]
        p = np.cross(dv[:, None, :], e2[None])
        det = np.einsum("pfk,fk->pf", p, e1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = -v0[None]
            u = np.einsum("pfk,pfk->pf", np.broadcast_to(tv, p.shape), p) * inv
            q = np.cross(np.broadcast_to(tv, p.shape), e1[None])
            w = np.einsum("pk,pfk->pf", dv, q) * inv
            t = np.einsum("fk,pfk->pf", e2, q) * inv
        hit = (np.abs(det) > 1e-300) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
        t = np.where(hit, t, np.inf).min(1)
        out[s:s + chunk] = np.where(np.isinf(t), 0, t)
    return out.reshape(H, W) if pixels is None else out


def edge_distance(vertices, faces, model, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, pixels=None):
    """per pixel centre, the distance in pixels to the nearest projected triangle edge (fp64; no clipping).
    pixels: flat indices (row * W + column) -> the distances of those pixels only, as a vector"""
    m = np.asarray(model, np.float64)
    v = np.asarray(vertices, np.float64) @ m[:3, :3].T + m[:3, 3]
    d = -v[:, 2]
    sx = (2 * fx / W * v[:, 0] / d + 1) * W / 2
    sy = H - (2 * fy / H * v[:, 1] / d + 1) * H / 2
    s = np.stack([sx, sy], -1)
    f = np.asarray(faces)
    a = np.concatenate([s[f[:, 0]], s[f[:, 1]], s[f[:, 2]]])
    b = np.concatenate([s[f[:, 1]], s[f[:, 2]], s[f[:, 0]]])
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    P = np.stack([cc.ravel(), rr.ravel()], -1)
    if pixels is not None:
        P = P[np.asarray(pixels)]
    best = np.full(P.shape[0], np.inf)
    ab = b - a
    L2 = np.maximum((ab * ab).sum(-1), 1e-300)
    for k in range(0, a.shape[0], 256):
        ap = P[:, None, :] - a[None, k:k + 256]
        t = np.clip((ap * ab[None, k:k + 256]).sum(-1) / L2[None, k:k + 256], 0, 1)
        dd = np.linalg.norm(ap - t[..., None] * ab[None, k:k + 256], axis=-1)
        best = np.minimum(best, dd.min(1))
    return best.reshape(H, W) if pixels is None else best


# ------------------------------------------------------------------------------------------------------------- meshes
def to_obj(v, f, quads=None):
    """OBJ text of a mesh: `v` records, then `f` records (1-based)"""
    lines = [f"v {float(x)!r} {float(y)!r} {float(z)!r}" for x, y, z in np.asarray(v, np.float64)]
    lines += ["f " + " ".join(str(int(k) + 1) for k in face) for face in (quads if quads is not None else f)]
    return "\n".join(lines) + "\n"


def box(hx=0.5, hy=0.3, hz=0.2):
    """(vertices, triangles, quads) of an axis-aligned box, outward CCW"""
    v = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    idx = lambda sx, sy, sz: (sx > 0) * 4 + (sy > 0) * 2 + (sz > 0)
    quads = []
    for ax in range(3):
        for sgn in (-1, 1):
            o1, o2 = [a for a in range(3) if a != ax]
            corners = []
            for a1, a2 in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                s = [0, 0, 0]
                s[ax], s[o1], s[o2] = sgn, a1, a2
                corners.append(idx(*s))
            quads.append(corners)
    quads = _orient_quads(v, quads)
    tris = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v, np.array(tris, np.int32), quads


def _orient_quads(v, quads):
    out = []
    c = v.mean(0)
    for q in quads:
        n = np.cross(v[q[1]] - v[q[0]], v[q[2]] - v[q[0]])
        out.append(q if n @ (v[q[0]] - c) > 0 else q[::-1])
    return out


def lathe(profile, n_lon):
    """surface of revolution about +y of profile points (r, y) from bottom to top (r = 0: a pole), outward CCW"""
    verts, ring = [], []
    for r, y in profile:
        if r == 0:
            ring.append([len(verts)] * n_lon)
            verts.append((0.0, y, 0.0))
        else:
            ring.append(list(range(len(verts), len(verts) + n_lon)))
            ph = 2 * np.pi * np.arange(n_lon) / n_lon
            verts += [(r * np.cos(p), y, r * np.sin(p)) for p in ph]
    faces = []
    for k in range(len(profile) - 1):
        for j in range(n_lon):
            a, b = ring[k][j], ring[k][(j + 1) % n_lon]
            c, d = ring[k + 1][(j + 1) % n_lon], ring[k + 1][j]
            if a != b:
                faces.append((a, b, c))
            if c != d:
                faces.append((a, c, d))
    faces = np.array(faces, np.int32)
    v = np.array(verts, np.float64)
    tri = v[faces]
    vol = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum()
    if vol < 0:
        faces = faces[:, ::-1].copy()
    return v, faces


def necked_cylinder(radius=0.15, half_height=0.45, neck=0.45, shoulder=0.4, n_lon=48):
    """a bottle: body of `radius` up to y = shoulder * half_height, a neck of neck * radius above, both ends capped"""
    r2, ys, h = neck * radius, shoulder * half_height, half_height
    return lathe([(0, -h), (radius, -h), (radius, ys), (r2, ys), (r2, h), (0, h)], n_lon)


def uv_sphere(radius=0.5, n_lat=32, n_lon=64):
    th = np.linspace(0, np.pi, n_lat + 1)
    prof = [(0.0 if k in (0, n_lat) else radius * np.sin(t), -radius * np.cos(t)) for k, t in enumerate(th)]
    return lathe(prof, n_lon)


def big_triangle(z=-1.0, size=50.0):
    """one triangle, CCW seen from the camera at the origin looking down -z, that covers the whole frame at depth -z"""
    return np.array([[-size, -size, z], [size, -size, z], [0.0, size, z]], np.float64), np.array([[0, 1, 2]], np.int32)


def flipped(f):
    return np.ascontiguousarray(np.asarray(f)[:, ::-1])


# ------------------------------------------------------------------------------------------------------------- samples
def depth_points_ref(depth, K=M.DATASET_K):
    """cppf_depth_points in numpy: the dataset's points (X, -Y, -Z) of the pixels with depth > 0, row-major"""
    kinv = np.linalg.inv(np.asarray(K, np.float64))
    r, c = np.where(depth > 0)
    u, v, z = c.astype(np.float64), r.astype(np.float64), depth[r, c].astype(np.float64)
    xyz = [(kinv[k, 0] * u + kinv[k, 1] * v) + kinv[k, 2] for k in range(3)]       # kinv[k,1] * v is exact where fma would be
    return np.stack([xyz[0] * z / xyz[2], -(xyz[1] * z / xyz[2]), -(xyz[2] * z / xyz[2])], -1)


def rotate_ref(pc, A):
    return np.stack([(A[r, 0] * pc[:, 0] + A[r, 1] * pc[:, 1]) + A[r, 2] * pc[:, 2] for r in range(3)], -1)


def voxel_first_ref(pc32, res):
    """cppf_voxel_dedupe: the lowest index of every occupied voxel floor(p / res) (fp64 divide), ascending"""
    keys = np.floor(pc32.astype(np.float64) / res).astype(np.int64)
    _, first = np.unique(keys, axis=0, return_index=True)
    return np.sort(first)


def sample_ref(vertices, faces, draws, cfg, is_nocs, jitter):
    """MeshViewSampler.sample (canonical) in numpy given its draws (R, t, scale) and the standard-normal jitter f64[n,3] the
    device drew: (pc f32[N,3] after dedupe, half_extents)"""
    bmin, bmax = M.mesh_bounds(vertices, faces)
    model = M.model_matrix(draws["R"], draws["t"], draws["scale"], bmin, bmax)
    depth = raster_ref(vertices, faces, model)
    pc = depth_points_ref(depth)
    pc = pc - np.asarray(draws["t"])
    pc = rotate_ref(pc, np.linalg.inv(draws["R"]))
    if is_nocs:
        pc = rotate_ref(pc, M.FLIP2NOCS)
    pc = pc + np.clip(cfg.res / 4 * jitter[:pc.shape[0]], -cfg.res / 2, cfg.res / 2)
    keep = voxel_first_ref(pc.astype(np.float32), cfg.res)
    return pc[keep].astype(np.float32), M.view_half_extents(bmin, bmax, draws["scale"])
