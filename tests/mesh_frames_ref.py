"""Shared test code for the mesh frames (cppf_amd/mesh_frames.py, cppf_raster_instances in csrc/raster.hip):

- raster_instances_ref: the numpy restatement of cppf_raster_instances -- mesh_ref.raster_ref (the restatement of
  cppf_raster_depth, bit for bit) per instance, composed with the contract's rule: the minimum depth over the instances that cover
  a pixel, on equal depth the lowest instance index;
- ray_cast_instances: the same composition over mesh_ref.ray_cast, an independent fp64 ray caster;
- frame_points_ref: the frame path's back-projection (utils.util.backproject's arithmetic, then frames.instance_cloud's x / y
  negation) of a depth image in metres, in fp64."""
import numpy as np

import mesh_ref as R
from cppf_amd import meshes as M


def _compose(renders):
    """(depth, labels) of per-instance depth images (0 = not covered): minimum over covered pixels, first arg-min"""
    depth = np.full(renders[0].shape, np.inf, renders[0].dtype)
    labels = np.full(renders[0].shape, -1, np.int32)
    for k, d in enumerate(renders):
        better = (d > 0) & (d < depth)                       # strict: an equal depth leaves the pixel with the lower index
        depth[better] = d[better]
        labels[better] = k
    depth[np.isinf(depth)] = 0
    return depth, labels


def raster_instances_ref(meshes, inst_mesh, model_views, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, znear=M.ZNEAR, cull=True):
    """include/cppf.h cppf_raster_instances in numpy fp32: (depth f32[H,W], labels i32[H,W]); background 0 / -1"""
    return _compose([R.raster_ref(*meshes[m][:2], mv, fx, fy, W, H, znear, cull) for m, mv in zip(inst_mesh, model_views)])


def ray_cast_instances(meshes, inst_mesh, model_views, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT, cull=True):
    return _compose([R.ray_cast(*meshes[m][:2], mv, fx, fy, W, H, cull) for m, mv in zip(inst_mesh, model_views)])


def edge_distance_instances(meshes, inst_mesh, model_views, fx=M.FX, fy=M.FY, W=M.WIDTH, H=M.HEIGHT):
    """per pixel centre, the distance in pixels to the nearest projected triangle edge of any instance"""
    return np.minimum.reduce([R.edge_distance(*meshes[m][:2], mv, fx, fy, W, H) for m, mv in zip(inst_mesh, model_views)])


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
