"""Drop-in for the reference's models/voting.py: the three module-level kernel objects
`ppf_kernel`, `backvote_kernel`, `rot_voting_kernel`, called exactly like the CuPy RawKernels
they replace (models/voting.py:4,70,115):

    kernel((grid, 1, 1), (block, 1, 1), (arg0, arg1, ...))   ->   None

with the same positional argument order.  Differences a caller sees:
  * array arguments are torch tensors on a HIP device (replace `cp.asarray(x)` by a torch tensor) or any object exposing
    `__cuda_array_interface__` (wrapped zero-copy);
    dtype/shape/contiguity mistakes raise TypeError/ValueError instead of corrupting memory;
  * the (grid, block) tuples are accepted and ignored -- launch geometry is the library's business
    (the reference's own grid for ppf_voting is sized by N**2, nocs/inference.py:192);
  * work is enqueued on the current torch stream; outputs are updated in place, as before.
`findpeak_kernel` is not provided: it is dead code in the reference (never launched, and its source
includes a file that does not exist).
"""
import torch

from .. import _lib
from .._torch_util import call, dev_tensor, fill, require_cuda, scalar, scratch, workspace

__all__ = ["ppf_kernel", "backvote_kernel", "rot_voting_kernel", "vote_argmax", "vote_argmax_dyn", "grid_argmax",
           "vote_grid_raw", "grid_from_raw", "vote_fixed_point_bits"]

F32, I32 = torch.float32, torch.int32


def _as_device_tensor(a):
    """array arguments may be any object that exposes device memory -- a torch tensor, or anything with
    `__cuda_array_interface__` (CuPy-style arrays, numba device arrays, rocm-aware buffers): wrapped zero-copy, so in-place
    outputs (grid_obj, output_ocs, candidates) land in the caller's memory.  Scalars and host objects pass through unchanged."""
    if isinstance(a, torch.Tensor) or not hasattr(a, "__cuda_array_interface__"):
        return a
    # (no device argument: torch reads the device of the pointer from the interface, so an array that lives on another GPU than
    # the current one is wrapped where it is instead of being COPIED to the current device -- in-place outputs would land in a
    # temporary and the caller's array stay zero)
    t = torch.as_tensor(a)
    ptr = a.__cuda_array_interface__["data"][0]
    if not t.is_cuda or not t.is_contiguous() or (t.numel() > 0 and t.data_ptr() != ptr):
        raise ValueError("could not wrap the __cuda_array_interface__ array zero-copy (a strided or read-only view?): pass a "
                         "C-contiguous device array")
    return t


class _Kernel:
    def __init__(self, name, nargs, fn):
        self.name, self._nargs, self._fn = name, nargs, fn

    def __call__(self, grid, block, args, **kw):
        if kw:
            raise TypeError(f"{self.name}: unexpected keyword arguments {sorted(kw)}")
        if len(args) != self._nargs:
            raise TypeError(f"{self.name}: expected {self._nargs} kernel arguments, got {len(args)}")
        require_cuda()
        self._fn(*(_as_device_tensor(a) for a in args))
        return None

    def __repr__(self):
        return f"<cppf_amd kernel {self.name}>"


def _dims(gx, gy, gz, grid=None):
    gx, gy, gz = int(scalar(gx)), int(scalar(gy)), int(scalar(gz))
    if min(gx, gy, gz) < 1:
        raise ValueError(f"grid dims must be positive, got {(gx, gy, gz)}")
    if grid is not None and grid.numel() != gx * gy * gz:
        raise ValueError(f"grid_obj has {grid.numel()} cells, dims say {gx}x{gy}x{gz}")
    return gx, gy, gz


def _vote_inputs(points, outputs, probs, point_idxs, corner, dev=None, dropin=False):
    """The tensor contract the vote wrappers share: points f32[N,3] (on `dev` when given), outputs f32[P,2], probs f32[N] or None
    (all ones, nocs/inference.py:201: no tensor is read), point_idxs i32[P,2] (as the reference passes it) or the original i64[P,2],
    corner f32, all on the device of points.  dropin: the reference kernel's own arguments -- probs required, int32 indices only.
    Returns (device, whether the indices are int64, P)."""
    dev = dev_tensor(points, F32, "points", (3,), dev).device
    dev_tensor(outputs, F32, "outputs", (2,), dev)
    if probs is not None or dropin:
        dev_tensor(probs, F32, "probs", None, dev)
    i64 = not dropin and isinstance(point_idxs, torch.Tensor) and point_idxs.dtype == torch.int64
    dev_tensor(point_idxs, torch.int64 if i64 else I32, "point_idxs", (2,), dev)
    dev_tensor(corner, F32, "corner", None, dev)
    if probs is not None and probs.numel() != points.shape[0]:
        raise ValueError("probs must have one entry per point")
    return dev, i64, point_idxs.shape[0]


def _vote_scratch(dev, tag, n_ppfs, n_rots=None, dims=None, tiles=0):
    """the zeroed vote workspace `tag` of a by-value vote (n_rots, dims) or, dims None, of a *_dyn vote of tile class `tiles`"""
    if dims is None:
        need = _lib.lib().cppf_vote_workspace_bytes_dyn_pairs(tiles, n_ppfs)
    else:
        need = _lib.lib().cppf_vote_workspace_bytes(n_ppfs, int(n_rots), *dims)
        if need == 0:
            raise ValueError(f"n_rots must be in 1..360, got {n_rots}")
    return scratch(workspace(need, dev, tag, zero=True))


def _ppf_voting(points, outputs, probs, point_idxs, grid_obj, corner, res, n_ppfs, n_rots, gx, gy, gz, adaptive):
    """models/voting.py:8-66 (launch: nocs/inference.py:197-205)"""
    dev, _, _ = _vote_inputs(points, outputs, probs, point_idxs, corner, dropin=True)
    n_ppfs, n_rots = int(scalar(n_ppfs)), int(scalar(n_rots))
    dev_tensor(grid_obj, F32, "grid_obj", None, dev)
    gx, gy, gz = _dims(gx, gy, gz, grid_obj)
    if outputs.shape[0] < n_ppfs or point_idxs.shape[0] < n_ppfs or n_ppfs < 0:
        raise ValueError("n_ppfs exceeds the outputs/point_idxs arrays")
    call("cppf_ppf_voting", dev, points, outputs, probs, point_idxs, grid_obj, corner, float(scalar(res)), points.shape[0], n_ppfs, n_rots,
         gx, gy, gz, bool(scalar(adaptive)), _vote_scratch(dev, "vote", n_ppfs, n_rots, (gx, gy, gz)))


def _vote_flags(accumulate, workgroups):
    """the flags word of cppf_vote_argmax / _dyn / _batch (include/cppf.h): CPPF_VOTE_ACCUMULATE | CPPF_VOTE_WORKGROUPS(n)"""
    w = int(workgroups or 0)
    if w and not 64 <= w <= 256:
        raise ValueError(f"workgroups must be 0 (one per CU) or in 64..256, got {workgroups}")
    return (1 if accumulate else 0) | (w << 8)


def vote_argmax(points, outputs, probs, point_idxs, grid_obj, corner, res, n_rots, adaptive, out_idx=None,
                out_val=None, accumulate=True, workgroups=0):
    """ppf_voting + np.argmax (nocs/inference.py:197-208) without the host round trip.
    accumulate=True: grid_obj += votes (reference semantics, grid zero-initialised by the caller);
    accumulate=False: grid_obj = votes (no memset needed).
    workgroups: 0 = one vote workgroup per CU (fastest for one instance on an idle chip); 64..256 = at most that many, for
    callers that keep several instances in flight on different streams (cppf.h: CPPF_VOTE_WORKGROUPS).
    point_idxs may be int32 (as the reference passes it) or the original int64 pair list.
    Returns (out_idx i64[1], out_val f32[1]) device tensors."""
    dev, i64, n_ppfs = _vote_inputs(points, outputs, probs, point_idxs, corner)
    dev_tensor(grid_obj, F32, "grid_obj", None, dev)
    if grid_obj.dim() != 3:
        raise ValueError("grid_obj must be [gx,gy,gz]")
    gx, gy, gz = grid_obj.shape
    if out_idx is None:
        out_idx = torch.empty(1, dtype=torch.int64, device=dev)
    if out_val is None:
        out_val = torch.empty(1, dtype=F32, device=dev)
    call("cppf_vote_argmax", dev, points, outputs, probs, point_idxs, i64, grid_obj, corner, float(scalar(res)), points.shape[0], n_ppfs,
         int(n_rots), gx, gy, gz, bool(adaptive), _vote_flags(accumulate, workgroups), out_idx, out_val,
         _vote_scratch(dev, "vote", n_ppfs, n_rots, (gx, gy, gz)))
    return out_idx, out_val


def vote_argmax_dyn(points, outputs, probs, point_idxs, grid_flat, shape, corner, res, n_rots, adaptive, out_idx, out_val,
                    many_tiles=False, accumulate=False, workgroups=0):
    """vote_argmax for a captured, shape-polymorphic chain (cppf_vote_argmax_dyn): `shape` is a device i32[4]
    {n_points, gx, gy, gz}; `points`/`probs` are capacity-sized (rows beyond n_points are never read), `grid_flat` is a
    flat f32 buffer whose first gx*gy*gz cells receive the grid in the usual C order.  Same results as vote_argmax on
    the real shape.  A record exceeding a capacity yields out_idx = -1."""
    dev, i64, n_ppfs = _vote_inputs(points, outputs, probs, point_idxs, corner)
    dev_tensor(grid_flat, F32, "grid_flat", None, dev)
    dev_tensor(shape, I32, "shape", None, dev)
    if shape.numel() < 4:
        raise ValueError("shape must be i32[4]")
    many_tiles = _lib.tile_class(many_tiles)
    call("cppf_vote_argmax_dyn", dev, points, outputs, probs, point_idxs, i64, grid_flat, grid_flat.numel(), corner, float(scalar(res)),
         points.shape[0], n_ppfs, int(n_rots), shape, many_tiles, bool(adaptive), _vote_flags(accumulate, workgroups),
         out_idx, out_val, _vote_scratch(dev, "vote_dyn", n_ppfs, tiles=many_tiles))
    return out_idx, out_val


def vote_batch_workgroups(n_items, workgroups=0):
    """vote workgroups each object of a vote_argmax_batch call gets (256 / n_items, at least 64, unless `workgroups` says otherwise)"""
    return int(_lib.lib().cppf_vote_batch_workgroups(int(n_items), _vote_flags(False, workgroups)))


def vote_argmax_batch(items, n_rots, adaptive, accumulate=False, workgroups=0, ws_tag="vote_b", workspaces_out=None):
    """vote_argmax / vote_argmax_dyn for up to 8 objects enqueued together (cppf_vote_argmax_batch): the objects share ONE vote
    launch and ONE reduce launch, each on 256 / len(items) workgroups (at least 64; `workgroups` overrides); an object whose grid
    needs >= 4 LDS tiles (a posed object) gets its own binning launch first.  `items`: dicts
    {points, outputs, point_idxs, grid, corner, res, out_idx, out_val[, probs][, shape, many_tiles]} -- `grid` f32[gx,gy,gz], or with
    `shape` (device i32[4] {n_points, gx, gy, gz}) a flat capacity buffer as for vote_argmax_dyn.  Every object keeps its own vote
    workspace (scratch tag ws_tag + index in the current workspace scope).  Same grids, arg-max and peaks as the single calls, at
    any width (the fixed-point scale does not follow the width)."""
    if not 1 <= len(items) <= 8:
        raise ValueError("1 to 8 objects per call")
    flags = _vote_flags(accumulate, workgroups)
    arr = (_lib.VoteItem * len(items))()
    keep = []
    dev = items[0]["points"].device
    for i, it in enumerate(items):
        points, outputs, probs, idx, corner = it["points"], it["outputs"], it.get("probs"), it["point_idxs"], it["corner"]
        _, i64, n_ppfs = _vote_inputs(points, outputs, probs, idx, corner, dev)
        grid = dev_tensor(it["grid"], F32, "grid", None, dev)
        out_idx = dev_tensor(it["out_idx"], torch.int64, "out_idx", None, dev)
        out_val = dev_tensor(it["out_val"], F32, "out_val", None, dev)
        shape = it.get("shape")
        a = arr[i]
        if shape is not None:
            dev_tensor(shape, I32, "shape", None, dev)
            many = _lib.tile_class(it.get("many_tiles") or 0)
            ws = _vote_scratch(dev, f"{ws_tag}dyn{i}", n_ppfs, tiles=many)
            fill(a, dev, shape_dev=shape, grid_capacity=grid.numel(), many_tiles=many, gx=1, gy=1, gz=1)
        else:
            if grid.dim() != 3:
                raise ValueError("grid must be [gx,gy,gz] (or pass `shape` for a capacity buffer)")
            gx, gy, gz = (int(v) for v in grid.shape)
            ws = _vote_scratch(dev, f"{ws_tag}{i}", n_ppfs, n_rots, (gx, gy, gz))
            fill(a, shape_dev=None, grid_capacity=0, many_tiles=0, gx=gx, gy=gy, gz=gz)
        fill(a, dev, points=points, outputs=outputs, probs=probs, point_idxs=idx, idx_is_i64=i64, grid=grid, corner=corner, out_idx=out_idx,
             out_val=out_val, workspace=ws, n_points=points.shape[0], n_ppfs=n_ppfs, res=float(scalar(it["res"])))
        keep.append(ws.buf)
    call("cppf_vote_argmax_batch", dev, len(items), arr, int(n_rots), bool(adaptive), flags)
    if workspaces_out is not None:  # (the back-vote loads the rotation table a vote left in its workspace)
        workspaces_out[:] = keep
    return [(it["out_idx"], it["out_val"]) for it in items]


def vote_fixed_point_bits(n_ppfs, n_rots, dims):
    """fixed-point bits the tiled vote would choose (a lower bound on the binned path) for a pair list of n_ppfs pairs"""
    return int(_lib.lib().cppf_vote_fixed_point_bits(int(n_ppfs), int(n_rots), int(dims[0]), int(dims[1]), int(dims[2])))


def vote_grid_raw(points, outputs, probs, point_idxs, grid_raw, quantum, corner, res, n_rots, adaptive, fixed_bits=0,
                  accumulate=False):
    """The centre vote as exact integers (cppf_vote_grid_raw): grid_raw i64[gx,gy,gz] = every cell's sum of deposited
    quanta, quantum f32[1] = value of one quantum (0: not valid).  Ranks voting slices of one pair list pass the same
    fixed_bits, all-reduce grid_raw as integers and convert once (grid_from_raw): the multi-GPU grid is then the
    single-GPU grid bit for bit (cppf_amd/sharding.py)."""
    dev, i64, n_ppfs = _vote_inputs(points, outputs, probs, point_idxs, corner)
    dev_tensor(grid_raw, torch.int64, "grid_raw", None, dev)
    dev_tensor(quantum, F32, "quantum", None, dev)
    if grid_raw.dim() != 3:
        raise ValueError("grid_raw must be [gx,gy,gz]")
    gx, gy, gz = grid_raw.shape
    call("cppf_vote_grid_raw", dev, points, outputs, probs, point_idxs, i64, grid_raw, quantum, corner, float(scalar(res)), points.shape[0],
         n_ppfs, int(n_rots), gx, gy, gz, bool(adaptive), bool(accumulate), int(fixed_bits),
         _vote_scratch(dev, "vote", n_ppfs, n_rots, (gx, gy, gz)))


def grid_from_raw(grid_raw, quantum, grid=None, out_idx=None, out_val=None):
    """grid = (float)(grid_raw * quantum) -- the one rounding vote_argmax applies -- and its arg-max: (grid, idx, val)"""
    dev = dev_tensor(grid_raw, torch.int64, "grid_raw").device
    dev_tensor(quantum, F32, "quantum", None, dev)
    if grid is None:
        grid = torch.empty(grid_raw.shape, dtype=F32, device=dev)
    dev_tensor(grid, F32, "grid", None, dev)
    if grid.numel() != grid_raw.numel():
        raise ValueError("grid and grid_raw must have the same number of cells")
    if out_idx is None:
        out_idx = torch.empty(1, dtype=torch.int64, device=dev)
    if out_val is None:
        out_val = torch.empty(1, dtype=F32, device=dev)
    ws = workspace(256, dev, "argmax")
    call("cppf_grid_from_raw", dev, grid_raw, grid_raw.numel(), quantum, grid, out_idx, out_val, scratch(ws))
    return grid, out_idx, out_val


def grid_argmax(grid, out_idx=None, out_val=None):
    """np.argmax(grid) on device (nocs/inference.py:208): (idx i64[1], val f32[1]) device tensors."""
    dev = dev_tensor(grid, F32, "grid").device
    if out_idx is None:
        out_idx = torch.empty(1, dtype=torch.int64, device=dev)
    if out_val is None:
        out_val = torch.empty(1, dtype=F32, device=dev)
    ws = workspace(256, dev, "argmax")
    call("cppf_grid_argmax", dev, grid, grid.numel(), out_idx, out_val, scratch(ws))
    return out_idx, out_val


def _backvote(points, outputs, out_offsets, point_idxs, corner, res, n_ppfs, n_rots, gx, gy, gz, gt_center, tol):
    """models/voting.py:74-112 (launch: nocs/inference.py:219-228)"""
    dev = dev_tensor(points, F32, "points", (3,)).device
    n_ppfs, n_rots = int(scalar(n_ppfs)), int(scalar(n_rots))
    dev_tensor(outputs, F32, "outputs", (2,), dev)
    dev_tensor(out_offsets, F32, "out_offsets", (3,), dev)
    dev_tensor(point_idxs, I32, "point_idxs", (2,), dev)
    dev_tensor(corner, F32, "corner", None, dev)
    dev_tensor(gt_center, F32, "gt_center", None, dev)
    gx, gy, gz = _dims(gx, gy, gz)
    if min(outputs.shape[0], point_idxs.shape[0], out_offsets.shape[0]) < n_ppfs or n_ppfs < 0:
        raise ValueError("n_ppfs exceeds the outputs/point_idxs/out_offsets arrays")
    call("cppf_backvote", dev, points, outputs, out_offsets, point_idxs, corner, float(scalar(res)), n_ppfs, n_rots, gx, gy, gz, gt_center,
         float(scalar(tol)), None)


def _rot_voting(points, not_used, preds_rot, outputs_up, point_idxs, corner, res, n_ppfs, n_rots, gx, gy, gz):
    """models/voting.py:119-147 (launch: nocs/inference.py:268-275); `not_used`, corner, res and the
    grid dims are ignored by the reference kernel too."""
    dev = dev_tensor(points, F32, "points", (3,)).device
    n_ppfs, n_rots = int(scalar(n_ppfs)), int(scalar(n_rots))
    dev_tensor(preds_rot, F32, "preds_rot", None, dev)
    dev_tensor(outputs_up, F32, "outputs_up", None, dev)
    dev_tensor(point_idxs, I32, "point_idxs", (2,), dev)
    if preds_rot.numel() < n_ppfs or point_idxs.shape[0] < n_ppfs or n_ppfs < 0:
        raise ValueError("n_ppfs exceeds the preds_rot/point_idxs arrays")
    if outputs_up.numel() < n_ppfs * n_rots * 3:
        raise ValueError("outputs_up must hold n_ppfs*n_rots*3 floats")
    call("cppf_rot_voting", dev, points, preds_rot, outputs_up, point_idxs, n_ppfs, n_rots)


ppf_kernel = _Kernel("ppf_voting", 13, _ppf_voting)
backvote_kernel = _Kernel("backvote", 13, _backvote)
rot_voting_kernel = _Kernel("rot_voting", 12, _rot_voting)
