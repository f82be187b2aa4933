"""What the centre vote refuses before any HIP call: every row is one call through the C ABI with its return code, run without a
device.  The host never dereferences a device pointer, so a non-null integer stands in for one.  No row passes validation (it would
reach a launch): the base call of every entry point is valid except for its null workspace, so a row with a bad argument shows that
the argument is checked BEFORE the workspace, and the base rows themselves show that nothing else in the call is refused.
The codes follow the contract in include/cppf.h and were recorded from the library before the host side was restated around one
request record; size queries come from the library."""
import ctypes as C

import pytest

from cppf_amd import _lib

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, _lib.EUNSUPPORTED
P = 0x10000   # "a device pointer"
BASE = dict(points=P, outputs=P, probs=P, point_idxs=P, i64=0, grid=P, grid_raw=P, quantum=P, corner=P, res=0.004, n_points=64,
            n_ppfs=10, n_rots=72, dims=(4, 4, 4), adaptive=1, flags=0, fixed_bits=0, out_idx=P, out_val=P, ws=None, ws_bytes=0,
            shape_dev=P, grid_capacity=64, many_tiles=0)
BY_VALUE = ("ppf_voting", "argmax", "grid_raw")
SINGLE = BY_VALUE + ("dyn",)
WITH_FLAGS = ("argmax", "grid_raw", "dyn")       # cppf_ppf_voting has no flags word
FUSED = dict(n_ppfs=524288, dims=(26, 76, 26))
BINNED = dict(n_ppfs=2097152, dims=(52, 152, 52))
BEYOND = dict(n_ppfs=1000, dims=(400, 400, 400))   # more than 64 tiles: global atomics, which need 256 bytes


def call(entry, **kw):
    a = dict(BASE, **kw)
    L = _lib.lib()
    gx, gy, gz = a["dims"]
    if entry == "ppf_voting":
        return L.cppf_ppf_voting(a["points"], a["outputs"], a["probs"], a["point_idxs"], a["grid"], a["corner"], a["res"], a["n_points"],
                                 a["n_ppfs"], a["n_rots"], gx, gy, gz, a["adaptive"], a["ws"], a["ws_bytes"], None)
    if entry == "argmax":
        return L.cppf_vote_argmax(a["points"], a["outputs"], a["probs"], a["point_idxs"], a["i64"], a["grid"], a["corner"], a["res"],
                                  a["n_points"], a["n_ppfs"], a["n_rots"], gx, gy, gz, a["adaptive"], a["flags"], a["out_idx"],
                                  a["out_val"], a["ws"], a["ws_bytes"], None)
    if entry == "grid_raw":
        return L.cppf_vote_grid_raw(a["points"], a["outputs"], a["probs"], a["point_idxs"], a["i64"], a["grid_raw"], a["quantum"],
                                    a["corner"], a["res"], a["n_points"], a["n_ppfs"], a["n_rots"], gx, gy, gz, a["adaptive"], a["flags"],
                                    a["fixed_bits"], a["ws"], a["ws_bytes"], None)
    assert entry == "dyn"
    return L.cppf_vote_argmax_dyn(a["points"], a["outputs"], a["probs"], a["point_idxs"], a["i64"], a["grid"], a["grid_capacity"],
                                  a["corner"], a["res"], a["n_points"], a["n_ppfs"], a["n_rots"], a["shape_dev"], a["many_tiles"],
                                  a["adaptive"], a["flags"], a["out_idx"], a["out_val"], a["ws"], a["ws_bytes"], None)


def need_of(**kw):
    """the library's own size query for the call"""
    a = dict(BASE, **kw)
    return _lib.lib().cppf_vote_workspace_bytes(a["n_ppfs"], a["n_rots"], *a["dims"])


def need_dyn(many_tiles, n_ppfs=BASE["n_ppfs"]):
    return _lib.lib().cppf_vote_workspace_bytes_dyn_pairs(many_tiles, n_ppfs)


def class_cells(many_tiles):
    return _lib.tiles_cap(many_tiles) * _lib.lib().cppf_vote_tile_cells()


# ---- single-object entry points: (row, the entry points it exists for, arguments changed from BASE, code)
ARGUMENT_ROWS = [
    ("base call, null workspace", SINGLE, {}, EWORKSPACE),
    ("null points", SINGLE, dict(points=None), EINVAL),
    ("null grid", SINGLE, dict(grid=None, grid_raw=None), EINVAL),
    ("null corner", SINGLE, dict(corner=None), EINVAL),
    ("pairs, null outputs", SINGLE, dict(outputs=None), EINVAL),
    ("pairs, null point_idxs", SINGLE, dict(point_idxs=None), EINVAL),
    ("n_rots 0", SINGLE, dict(n_rots=0), EINVAL),
    ("n_rots 361", SINGLE, dict(n_rots=361), EINVAL),
    ("a zero dim", BY_VALUE, dict(dims=(4, 0, 4)), EINVAL),
    ("2^31 cells", BY_VALUE, dict(dims=(2048, 1024, 1024)), EINVAL),
    ("n_points 0", SINGLE, dict(n_points=0), EINVAL),
    ("n_ppfs -1", SINGLE, dict(n_ppfs=-1), EINVAL),
    ("flags bit 1", WITH_FLAGS, dict(flags=2), EINVAL),
    ("flags bit 17", WITH_FLAGS, dict(flags=1 << 17), EINVAL),
    ("flags bit 1 on a bad call", WITH_FLAGS, dict(flags=2, points=None, n_rots=0), EINVAL),
    ("workgroup hint with an integer image", ("grid_raw",), dict(flags=128 << 8), EINVAL),
    ("fixed_bits 7", ("grid_raw",), dict(fixed_bits=7), EINVAL),
    ("fixed_bits 25", ("grid_raw",), dict(fixed_bits=25), EINVAL),
    ("fixed_bits -1", ("grid_raw",), dict(fixed_bits=-1), EINVAL),
    ("null grid_raw", ("grid_raw",), dict(grid_raw=None), EINVAL),
    ("null quantum_out", ("grid_raw",), dict(quantum=None), EINVAL),
    # an empty pair list needs no outputs / point_idxs, and still its workspace
    ("no pairs, null outputs and point_idxs", ("ppf_voting", "argmax"), dict(n_ppfs=0, outputs=None, point_idxs=None), EWORKSPACE),
    # ---- the shape-polymorphic call
    ("null shape_dev", ("dyn",), dict(shape_dev=None), EINVAL),
    ("null shape_dev, good workspace", ("dyn",), lambda: dict(shape_dev=None, ws=P, ws_bytes=need_dyn(0)), EINVAL),
    ("n_ppfs 0", ("dyn",), dict(n_ppfs=0, ws=P, ws_bytes=1 << 40), EINVAL),
    ("grid_capacity 0", ("dyn",), dict(grid_capacity=0, ws=P, ws_bytes=1 << 40), EINVAL),
    ("grid_capacity 2^31", ("dyn",), dict(grid_capacity=1 << 31, ws=P, ws_bytes=1 << 40), EINVAL),
    # ---- an integer image needs the tiled path, whatever the workspace
    ("image beyond 64 tiles, null workspace", ("grid_raw",), BEYOND, EUNSUPPORTED),
    ("image beyond 64 tiles, 255 bytes", ("grid_raw",), dict(BEYOND, ws=P, ws_bytes=255), EUNSUPPORTED),
    ("image beyond 64 tiles, large workspace", ("grid_raw",), dict(BEYOND, ws=P, ws_bytes=1 << 40), EUNSUPPORTED),
    ("grid beyond 64 tiles, null workspace", ("ppf_voting", "argmax"), BEYOND, EWORKSPACE),
    ("grid beyond 64 tiles, 255 bytes", ("ppf_voting", "argmax"), dict(BEYOND, ws=P, ws_bytes=255), EWORKSPACE),
    ("grid beyond 64 tiles, sized pointer null", ("ppf_voting", "argmax"), dict(BEYOND, ws=None, ws_bytes=1 << 40), EWORKSPACE),
]
for shape_name, shape in (("fused", FUSED), ("binned", BINNED)):
    ARGUMENT_ROWS += [
        (f"{shape_name} shape, null workspace", BY_VALUE, shape, EWORKSPACE),
        (f"{shape_name} shape, sized pointer null", BY_VALUE, (lambda s=shape: dict(s, ws=None, ws_bytes=need_of(**s))), EWORKSPACE),
        (f"{shape_name} shape, one byte short", BY_VALUE, (lambda s=shape: dict(s, ws=P, ws_bytes=need_of(**s) - 1)), EWORKSPACE),
        # (a bad argument is reported before the short workspace)
        (f"{shape_name} shape, one byte short, n_rots 0", BY_VALUE,
         (lambda s=shape: dict(s, ws=P, ws_bytes=need_of(**s) - 1, n_rots=0)), EINVAL),
    ]
for many in (0, 16):
    ARGUMENT_ROWS += [
        (f"class {many}, one byte short", ("dyn",), (lambda m=many: dict(many_tiles=m, ws=P, ws_bytes=need_dyn(m) - 1)), EWORKSPACE),
        (f"class {many}, capacity + 1, good workspace", ("dyn",),
         (lambda m=many: dict(many_tiles=m, grid_capacity=class_cells(m) + 1, ws=P, ws_bytes=need_dyn(m))), EINVAL),
        # (the capacity of the class is looked at after the workspace)
        (f"class {many}, capacity + 1, one byte short", ("dyn",),
         (lambda m=many: dict(many_tiles=m, grid_capacity=class_cells(m) + 1, ws=P, ws_bytes=need_dyn(m) - 1)), EWORKSPACE),
        (f"class {many}, capacity + 1, null workspace", ("dyn",),
         (lambda m=many: dict(many_tiles=m, grid_capacity=class_cells(m) + 1)), EWORKSPACE),
    ]
SINGLE_CASES = [pytest.param(entry, kw, code, id=f"{entry}: {row}") for row, entries, kw, code in ARGUMENT_ROWS for entry in entries]


@pytest.mark.parametrize("entry, kw, code", SINGLE_CASES)
def test_single_object_refusals(entry, kw, code):
    assert call(entry, **(kw() if callable(kw) else kw)) == code


# ---- cppf_vote_argmax_batch: items are a host array
def item(**kw):
    """a valid by-value item on the fused shape (its workspace a stand-in of the queried size), or with `shape_dev` a valid dynamic one"""
    a = dict(BASE, **FUSED)
    a.update(kw)
    dyn = a.get("shape_dev_item") is not None
    if "ws_bytes" not in kw:
        a["ws"], a["ws_bytes"] = P, (need_dyn(a["many_tiles"], a["n_ppfs"]) if dyn else need_of(**a))
    gx, gy, gz = a["dims"]
    return dict(points=a["points"], outputs=a["outputs"], probs=a["probs"], point_idxs=a["point_idxs"], grid=a["grid"], corner=a["corner"],
                out_idx=a["out_idx"], out_val=a["out_val"], workspace=a["ws"], workspace_bytes=a["ws_bytes"],
                shape_dev=a.get("shape_dev_item"), grid_capacity=a["grid_capacity"] if dyn else 0, n_points=a["n_points"],
                n_ppfs=a["n_ppfs"], res=a["res"], gx=gx, gy=gy, gz=gz, idx_is_i64=a["i64"], many_tiles=a["many_tiles"] if dyn else 0)


def batch(items, n_items=None, n_rots=72, flags=0, null_items=False):
    arr = (_lib.VoteItem * max(len(items), 1))()
    for slot, fields in zip(arr, items):
        for k, v in fields.items():
            setattr(slot, k, v)
    n = len(items) if n_items is None else n_items
    return _lib.lib().cppf_vote_argmax_batch(n, None if null_items else C.addressof(arr), n_rots, 1, flags, None)


def short(**kw):
    """the item with a workspace one byte short of its query"""
    it = item(**kw)
    it["workspace_bytes"] -= 1
    return it


BATCH_ROWS = [
    ("n_items 0", lambda: batch([short()], n_items=0), EINVAL),
    ("n_items 9", lambda: batch([short()] * 9), EINVAL),
    ("null items", lambda: batch([short()], null_items=True), EINVAL),
    ("flags bit 1", lambda: batch([short()], flags=2), EINVAL),
    ("flags bit 17", lambda: batch([short()], flags=1 << 17), EINVAL),
    ("n_rots 0", lambda: batch([short()], n_rots=0), EINVAL),
    ("n_rots 361", lambda: batch([short()], n_rots=361), EINVAL),
    ("one item, null workspace", lambda: batch([item(ws=None, ws_bytes=0)]), EWORKSPACE),
    ("one item, sized pointer null", lambda: batch([dict(short(), workspace=None)]), EWORKSPACE),
    # the pre-pass over the workspaces comes before the loop that meets item 0's null points
    ("item 0 invalid, item 1 short", lambda: batch([item(points=None), short()]), EWORKSPACE),
    ("valid items, the last one short", lambda: batch([item(), item(**BINNED), item(shape_dev_item=P, grid_capacity=64), short()]), EWORKSPACE),
    ("valid items, a binned last one short", lambda: batch([item(), short(**BINNED)]), EWORKSPACE),
    ("valid items, a dynamic last one short", lambda: batch([item(), short(shape_dev_item=P, grid_capacity=64, many_tiles=16)]), EWORKSPACE),
    ("valid items, the last beyond 64 tiles with 255 bytes", lambda: batch([item(), item(ws=P, ws_bytes=255, **BEYOND)]), EWORKSPACE),
    ("eight valid items, the last one short", lambda: batch([item()] * 7 + [short()]), EWORKSPACE),
    # an invalid argument alone is refused when the loop reaches it: nothing was launched for a batch of one
    ("one item, null points", lambda: batch([item(points=None)]), EINVAL),
    ("one item, null grid", lambda: batch([item(grid=None)]), EINVAL),
    ("one item, a zero dim", lambda: batch([item(dims=(26, 0, 26), ws=P, ws_bytes=1 << 40)]), EINVAL),
    ("one item, n_points 0", lambda: batch([item(n_points=0)]), EINVAL),
    ("one dynamic item, grid_capacity 0", lambda: batch([item(shape_dev_item=P, grid_capacity=0)]), EINVAL),
    ("one dynamic item, capacity + 1",
     lambda: batch([item(shape_dev_item=P, grid_capacity=class_cells(16) + 1, many_tiles=16)]), EINVAL),
    ("one dynamic item, capacity + 1, short", lambda: batch([short(shape_dev_item=P, grid_capacity=class_cells(0) + 1)]), EWORKSPACE),
]


@pytest.mark.parametrize("run, code", [pytest.param(run, code, id=row) for row, run, code in BATCH_ROWS])
def test_batch_refusals(run, code):
    assert run() == code
