"""The table of tests/scratch_cases.py and its harness, without a device: every size query of include/cppf.h has a row (or one of at
most three reasoned exclusions), the queries are non-decreasing in their size arguments around the rows' shapes, the two shapes
of a row reach the layouts they name, and the harness primitives do what the device test relies on."""
import os
import re

import numpy as np
import pytest
import torch

import scratch_cases as S
from cppf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cppf.h")
QUERIED = [r for r in S.ROWS if r.query is not None]


def header_queries():
    """every exported `size_t cppf_*_workspace_bytes*(` of the header, plus cppf_vote_workspace_init_bytes"""
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^size_t\s+(cppf_\w*workspace(?:_init)?_bytes\w*)\s*\(", text, re.M)))


def test_every_size_query_of_the_header_has_a_row():
    names = header_queries()
    assert "cppf_vote_workspace_init_bytes" in names and len(names) >= len(S.MUST_COVER) + 1
    covered = {r.query for r in QUERIED} | {q for r in S.ROWS for q in r.also}
    assert len(S.EXCLUDED) <= 3 and all(isinstance(v, str) and len(v) > 20 for v in S.EXCLUDED.values())
    assert not set(S.EXCLUDED) & set(S.MUST_COVER) and not set(S.EXCLUDED) & covered
    assert set(S.MUST_COVER) <= covered
    missing = [n for n in names if n not in covered and n not in S.EXCLUDED]
    assert missing == [], missing
    assert covered | set(S.EXCLUDED) <= set(names)               # no row names a query the header does not export
    # the pose tail takes its scratch through CppfPoseTailItem: a row of its own, without a query
    assert S.BY_NAME["pose_tail"].query is None and "cppf_pose_tail_batch" in S.BY_NAME["pose_tail"].entries


def test_rows_name_entry_points_of_the_binding():
    assert len({r.name for r in S.ROWS}) == len(S.ROWS)
    for r in S.ROWS:
        assert set(r.shapes) == {"small", "large"} and r.entries, r.name
        for e in r.entries + ((r.query,) if r.query else ()) + tuple(r.also):
            assert e in _lib._SIGS, (r.name, e)
        assert r.refusal in (S.EWORKSPACE, S.EINVAL)


def test_the_must_cover_entry_points_are_run():
    run = {e for r in S.ROWS for e in r.entries}
    for e in ("cppf_vote_argmax", "cppf_ppf_voting", "cppf_vote_grid_raw", "cppf_backvote_ws", "cppf_backvote_count", "cppf_vote_argmax_dyn",
              "cppf_vote_argmax_batch", "cppf_pair_mlp_forward", "cppf_pair_mlp_decode", "cppf_pair_mlp_decode_sel", "cppf_pair_mlp_bf16_forward",
              "cppf_axis_sign", "cppf_scale_sum", "cppf_scale_exp_sum", "cppf_pose_tail_batch"):
        assert e in run, e
    pe = S.BY_NAME["point_encoder"].shapes
    assert {pe["small"]["layers"], pe["large"]["layers"]} == {1, 2}


@pytest.mark.parametrize("row", S.ROWS, ids=[r.name for r in S.ROWS])
def test_declared_sizes(row):
    """positive, the same number of regions at both shapes, and the large shape's regions hold the small shape's (the reuse leg
    runs both in the buffers of the large one)"""
    small, large = row.sizes(row.shapes["small"]), row.sizes(row.shapes["large"])
    assert len(small) == len(large) >= 1
    assert all(0 < a <= b for a, b in zip(small, large)), (small, large)
    assert [list(c) for c in row.refusals(row.shapes["small"])] and all(i < len(small) for c in row.refusals(row.shapes["small"]) for i in c)


def _grid(v):
    return sorted({max(v - 2, 0), max(v - 1, 0), v, v + 1, v + 2, v + 17, 2 * v, 2 * v + 1})


@pytest.mark.parametrize("row", QUERIED, ids=[r.name for r in QUERIED])
def test_queries_do_not_decrease_in_their_size_arguments(row):
    """one allocation sized for the largest call serves every call only if a larger problem never declares less: every size
    argument, alone, over a grid around both shapes (arguments the entry point refuses -- a count of zero, more meshes than faces --
    are left out: the query returns 0 for them)"""
    for shape, p in row.shapes.items():
        at = row.qargs(p)
        assert row.valid(**at) and row.q(**at) > 0
        for axis in row.axes:
            pts = [(v, row.q(**{**at, axis: v})) for v in _grid(at[axis]) if row.valid(**{**at, axis: v})]
            assert len(pts) >= 3                             # (one mesh of 8 faces leaves 1, 2, 3 meshes; a layer count of 1: 1, 2, 3, 18)
            assert all(b[1] >= a[1] > 0 for a, b in zip(pts, pts[1:])), (row.name, shape, axis, pts)


def test_vote_query_in_the_grid_dims():
    """NOT monotone in gx, gy, gz, by design: the bytes are those of the launch plan -- the tile footprint follows the grid's own
    extents, so a slightly larger grid can take a differently cut, smaller set of partial tiles -- and a grid beyond 64 tiles takes
    the global-atomics path, which needs no tiles at all.  What the header's remark rests on instead is a floor: no valid call
    declares less than the state block (cppf_vote_workspace_init_bytes), so that a workspace sized for one call always holds the
    state a later tiled call finds; and `enough for the largest call` means the largest of the QUERIED values."""
    L = _lib.lib()
    init = L.cppf_vote_workspace_init_bytes()
    assert init % 256 == 0 and init > 0
    row = S.BY_NAME["vote"]
    drops = 0
    for shape, p in row.shapes.items():
        at = row.qargs(p)
        for axis in ("gx", "gy", "gz"):
            vals = [row.q(**{**at, axis: v}) for v in range(1, 400)]
            assert min(vals) >= init, (shape, axis)
            drops += sum(b < a for a, b in zip(vals, vals[1:]))
    assert drops > 0                                         # (the reason this is not in the monotonicity table)
    assert L.cppf_vote_tiles(400, 400, 400) == 0 and L.cppf_vote_workspace_bytes(3000, 72, 400, 400, 400) == init      # global atomics
    assert L.cppf_vote_workspace_bytes(0, 72, 40, 36, 30) == init                                                     # an empty list
    assert L.cppf_vote_workspace_bytes(3000, 0, 40, 36, 30) == 0 and L.cppf_vote_workspace_bytes(3000, 361, 40, 36, 30) == 0


def test_vote_dyn_query_in_the_tile_class():
    """many_tiles is a capacity CLASS, not a size: 0 (3 tiles, no queues) < 4 <= ... <= 64, and 1 means 64"""
    q = S.BY_NAME["vote_dyn"].q
    order = [q(n_ppfs=3000, many_tiles=m) for m in [0] + list(range(4, 65))]
    assert all(a <= b for a, b in zip(order, order[1:])) and order[0] < order[1]
    assert q(n_ppfs=3000, many_tiles=1) == order[-1]
    assert all(v >= _lib.lib().cppf_vote_workspace_init_bytes() for v in order)


def test_mesh_vote_stats_query_in_the_mesh_count():
    """NOT monotone in n_meshes once the launch is at its cap, by design: a mesh gets min(ceil(pairs / 256), ceil(4096 / M)) blocks of
    partial maxima, so below the cap the bytes grow with M, and at the cap M ceil(4096 / M) blocks is a sawtooth between 4096 and
    4096 + M - 1.  What holds instead: the bytes are exactly those blocks (16 B each) plus the centres, each rounded up to 256 -- so
    a workspace for 4096 + M blocks serves every batch of up to M meshes, and `the largest call` means the largest QUERIED value."""
    q = S.BY_NAME["mesh_vote_stats"].q
    r256 = lambda v: S.round_up(v, 256)
    for pairs in (500, 128 * 256 + 5):
        vals = []
        for M in range(1, 200):
            blocks = min((pairs + 255) // 256, (4096 + M - 1) // M)
            assert q(M=M, n=300, pairs=pairs) == r256(M * 24) + r256(M * blocks * 16), (M, pairs)
            assert M * blocks < 4096 + M
            vals.append(q(M=M, n=300, pairs=pairs))
        drops = sum(b < a for a, b in zip(vals, vals[1:]))
        assert (drops > 0) == (pairs > 500)                  # (the small shape stays below the cap up to M = 199: 2 blocks a mesh)
        assert all(b >= a for a, b in zip(vals[:32], vals[1:32]))


def test_the_vote_shapes_reach_both_paths():
    """small: the fused kernel on a 2-tile grid; large: binning + queue-consuming kernels on >= 4 tiles; the large grid fits the
    dyn row's class 16"""
    L = _lib.lib()
    for name in ("vote", "vote_dyn"):
        for shape, p in S.BY_NAME[name].shapes.items():
            plan = np.zeros(10, np.int32)
            assert L.cppf_vote_plan_query(p["n_ppfs"], S.VOTE_ROTS, p["gx"], p["gy"], p["gz"], plan.ctypes.data) == 0
            want_path, lo, hi = (2, 2, 2) if shape == "small" else (3, 4, 16)
            assert plan[0] == want_path and lo <= plan[1] <= hi, (name, shape, plan)
            assert plan[9] > 0                               # fixed point: the same bits on every run
    assert S.BY_NAME["vote_dyn"].shapes["small"]["many_tiles"] == 0 and S.BY_NAME["vote_dyn"].shapes["large"]["many_tiles"] == 16


def test_the_shapes_reach_the_layouts_they_name():
    sh = lambda n: (S.BY_NAME[n].shapes["small"], S.BY_NAME[n].shapes["large"])
    s, l = sh("compact")
    assert s["n"] <= 1024 and (l["n"] + 1023) // 1024 == 3
    s, l = sh("pose_sums")
    assert s["n_sel"] < 256 and l["n_sel"] > 65536
    s, l = sh("pair_mlp")
    assert (s["N"], s["P"]) == (64, 65) and (l["N"], l["P"]) == (300, 1000)
    s, l = sh("backproject")
    assert s["H"] * s["W"] <= 1024 < 2 * 1024 < l["H"] * l["W"]
    s, l = sh("scene_proposals")
    assert all(s[k] <= 8 for k in ("gx", "gy", "gz")) and all(l[k] > 16 and l[k] % 8 for k in ("gx", "gy", "gz"))
    s, l = sh("point_encoder_backward")
    assert s["N"] < 1024 < l["N"]
    s, l = sh("box_nms")
    assert max(s["sizes"]) <= 64 and max(l["sizes"]) > 128 and 0 in l["sizes"] and sum(l["sizes"]) == l["n"]
    s, l = sh("surface_sample")
    assert s["F"] <= 1024 < l["F"]
    for name in ("segment_instance", "segment_instances", "proposal_support"):       # chunks of 1024 pairs, blocks of 256 points
        s, l = sh(name)
        assert s["P"] <= 1024 and (l["P"] + 1023) // 1024 == 3 and l["P"] % 1024 and s["N"] <= 256 < l["N"] <= 512, name
    s, l = sh("mesh_vote_stats")                                 # blocks of 256 pairs per mesh, at most ceil(4096 / M) of them
    blocks, cap = (lambda p: (p["pairs"] + 255) // 256), (lambda p: (4096 + p["M"] - 1) // p["M"])
    assert 1 < blocks(s) < cap(s) and blocks(l) == cap(l) + 1 and s["n"] <= 256 < l["n"]
    assert (S.RW, S.RH) == (40, 24)


# ------------------------------------------------------------------------------------------------ the harness
@pytest.mark.parametrize("declared", [1, 255, 256, 257, 1000, 4096, 70001])
def test_fenced_layout(declared):
    f = S.Fenced(declared, "cpu")
    assert f.ptr % 256 == 0 and f.ptr == f.body.data_ptr()
    assert f.body.numel() == declared and f.body_bytes == S.round_up(declared, 256) and f.body_bytes % 256 == 0
    lo, hi = f.fences()
    assert lo.numel() == S.FENCE == 256 * 1024 and hi.numel() == S.FENCE + f.body_bytes - declared
    assert lo.data_ptr() + S.FENCE == f.ptr and hi.data_ptr() == f.ptr + declared        # bytes from ptr + declared on count as fence
    assert hi.data_ptr() + hi.numel() <= f.t.data_ptr() + f.t.numel()
    assert f.intact() and bool((f.t == S.FENCE_BYTE).all())
    S.poison(f.body, "ff")
    assert f.intact()
    for victim in (lo[-1:], hi[:1], hi[-1:], lo[:1]):        # one byte on either side of the body, and the far ends
        victim.fill_(0)
        assert not f.intact()
        victim.fill_(S.FENCE_BYTE)
    assert f.intact()


def test_poison_patterns_read_as_claimed():
    b = torch.zeros(64, dtype=torch.uint8)
    S.poison(b, "ff")
    a = b.numpy()
    assert np.isnan(a.view(np.float32)).all() and np.isnan(a.view(np.float64)).all()
    assert (a.view(np.int32) == -1).all() and (a.view(np.uint32) == 2 ** 32 - 1).all() and (a.view(np.uint64) == 2 ** 64 - 1).all()
    b = torch.zeros(67, dtype=torch.uint8)                   # a ragged tail is filled too
    S.poison(b, "big")
    a = b.numpy()[:64]
    assert a[:4].tolist() == [0x00, 0x80, 0x7F, 0x7F]        # 0x7F7F8000, little-endian
    f = a.view(np.float32)
    assert np.isfinite(f).all() and (f > 3e38).all()
    assert (a.view(np.int32) == 0x7F7F8000).all() and (a.view(np.int32) > 2 ** 30).all()
    assert np.isfinite(a.view(np.float64)).all() and (a.view(np.float64) > 1e300).all()
    assert (b.numpy()[64:] == 0x7F).all()


def test_vote_rule_never_poisons_the_state_region():
    init = int(_lib.lib().cppf_vote_workspace_init_bytes())
    for declared in (init - 1024, init, init + 4096):
        (z0, z1), (p0, p1) = S.poison_range(declared, True, init)
        assert (z0, z1) == (0, min(init, declared)) and (p0, p1) == (z1, declared)
    assert S.poison_range(5000, False, init) == ((0, 0), (0, 5000))
    # on a buffer: a small `init` through the same code path prepare() takes
    body = torch.full((4096,), 0x33, dtype=torch.uint8)
    S.prepare(body, 4096, True, "ff", init_bytes=1024)
    assert bool((body[:1024] == 0).all()) and bool((body[1024:] == 0xFF).all())
    S.prepare(body, 4096, True, "big", init_bytes=8192)      # a workspace shorter than the state block: all of it stays zero
    assert bool((body == 0).all())
    # a workspace in use (the end-to-end test, between two runs): the state region keeps what the last call left, byte for byte
    body = torch.full((4096,), 0x33, dtype=torch.uint8)
    S.dirty(body, 4096, True, "ff", init_bytes=1024)
    assert bool((body[:1024] == 0x33).all()) and bool((body[1024:] == 0xFF).all())
    S.dirty(body, 4096, True, "big", init_bytes=8192)
    assert bool((body[:1024] == 0x33).all()) and bool((body[1024:] == 0xFF).all())
    S.dirty(body, 4096, False, "ff")
    assert bool((body == 0xFF).all())
    for row in S.ROWS:
        assert row.state == row.name.startswith("vote")
