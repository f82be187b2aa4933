"""Shared test code for the mesh frames (cppf_amd/mesh_frames.py, cppf_raster_instances in csrc/raster.hip):

- raster_instances_ref: the numpy restatement of cppf_raster_instances -- mesh_ref.raster_ref (the restatement of
  cppf_raster_depth, bit for bit) per instance, composed with the contract's rule: the minimum depth over the instances that cover
  a pixel, on equal depth the lowest instance index; the composition streams, one instance's image at a time;
- ray_cast_instances: the same composition over mesh_ref.ray_cast, an independent fp64 ray caster;
- frame_points_ref: the frame path's back-projection (utils.util.backproject's arithmetic, then frames.instance_cloud's x / y
  negation) of a depth image in metres, in fp64."""
import numpy as np

import mesh_ref as R
from cppf_amd import meshes as M


def _compose(renders, at=None):
    """(depth, labels) of per-instance depth images (0 = not covered), taken one at a time from an iterable -- the K images are
    never held together: minimum over covered pixels, first arg-min.  at: instance counts -> {K: (depth, labels) of the first K}"""
    depth = labels = None
    done = {}

    def result():
        return np.where(np.isinf(depth), 0, depth).astype(depth.dtype), labels.copy()

    k = 0
    for k, d in enumerate(renders):
        if depth is None:
            depth, labels = np.full(d.shape, np.inf, d.dtype), np.full(d.shape, -1, np.int32)
        better = (d > 0) & (d < depth)                       # strict: an equal depth leaves the pixel with the lower index
        depth[better] = d[better]
        labels[better] = k
        if at is not None and k + 1 in at:
            done[k + 1] = result()
    if at is not None:
        assert sorted(done) == sorted(at), (sorted(done), sorted(at))
        return done
    return result()


def _windowed(render, shape, dtype, win, fill):
    """an image that is `fill` outside the inclusive pixel window (c0, r0, c1, r1) and render(flat pixel indices) inside"""
    c0, r0, c1, r1 = (int(x) for x in win)
    rr, cc = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing="ij")
    out = np.full(shape, fill, dtype)
    out[r0:r1 + 1, c0:c1 + 1] = render((rr * shape[1] + cc).ravel()).reshape(rr.shape)
    return out


def raster_instances_ref(meshes, inst_mesh, model_views, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, znear=M.ZNEAR, cull=True, at=None):
    """include/cppf.h cppf_raster_instances in numpy fp32: (depth f32[H,W], labels i32[H,W]); background 0 / -1.
    at: a collection of instance counts -> {K: the images of the first K instances}, all from one pass"""
    return _compose((R.raster_ref(*meshes[m][:2], mv, fx, fy, W, H, znear, cull) for m, mv in zip(inst_mesh, model_views)), at)


def ray_cast_instances(meshes, inst_mesh, model_views, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, cull=True, windows=None):
    """windows: per instance an inclusive pixel window (c0, r0, c1, r1); the rays of an instance are cast inside its window only
    and it counts as a miss elsewhere (for instances known to stay inside their windows)"""
    if windows is None:
        return _compose(R.ray_cast(*meshes[m][:2], mv, fx, fy, W, H, cull) for m, mv in zip(inst_mesh, model_views))
    return _compose(_windowed(lambda px, m=m, mv=mv: R.ray_cast(*meshes[m][:2], mv, fx, fy, W, H, cull, pixels=px), (H, W), np.float64, w, 0.0)
                    for m, mv, w in zip(inst_mesh, model_views, windows))


def edge_distance_instances(meshes, inst_mesh, model_views, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, windows=None):
    """per pixel centre, the distance in pixels to the nearest projected triangle edge of any instance (windows: as
    ray_cast_instances; outside its window an instance's edges count as infinitely far)"""
    if windows is None:
        return np.minimum.reduce([R.edge_distance(*meshes[m][:2], mv, fx, fy, W, H) for m, mv in zip(inst_mesh, model_views)])
    best = np.full((H, W), np.inf)
    for m, mv, w in zip(inst_mesh, model_views, windows):
        np.minimum(best, _windowed(lambda px: R.edge_distance(*meshes[m][:2], mv, fx, fy, W, H, pixels=px), (H, W), np.float64, w, np.inf),
                   out=best)
    return best


def frame_points_ref(depth, intrinsics, mask=None):
    """points f64[n,3] of the pixels with depth > 0 (and mask), row-major: xyz = inv(K) (u, v, 1) with the INTEGER pixel
    coordinates, p = xyz z / xyz.z, x and y negated (backproject), then negated again (instance_cloud)"""
    kinv = np.linalg.inv(np.asarray(intrinsics, np.float64))
    ok = depth > 0 if mask is None else (depth > 0) & mask
    r, c = np.where(ok)
    u, v, z = c.astype(np.float64), r.astype(np.float64), depth[r, c].astype(np.float64)
    xyz = [(kinv[k, 0] * u + kinv[k, 1] * v) + kinv[k, 2] for k in range(3)]
    p = np.stack([-(xyz[0] * z / xyz[2]), -(xyz[1] * z / xyz[2]), xyz[2] * z / xyz[2]], -1)
    return np.stack([-p[:, 0], -p[:, 1], p[:, 2]], -1)


def model(t, rot=np.eye(3), scale=1.0):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = np.asarray(rot) * scale, t
    return m


def rot(a, b):
    return M.roty(a)[:3, :3] @ M.rotx(b)[:3, :3]
