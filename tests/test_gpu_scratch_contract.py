"""Every scratch-taking entry point of include/cppf.h held to the header's two promises about workspaces: a workspace of exactly
the queried size is enough, and what it holds on entry does not matter (the vote's state block aside).  The table and the harness
are tests/scratch_cases.py; four legs per row:

  baseline   a fresh zero-filled allocation of twice the declared size: the reference of the other legs (its correctness against
             the oracle, the restatements and the fixtures is what the rest of the suite pins)
  exact      the declared bytes between two 256 KiB fences, poisoned: return code 0, every output bit for bit the baseline's,
             every fence byte intact
  reuse      one fenced buffer sized for the large shape, poisoned once: large, small, large with nothing written in between
  refusal    the same full-size buffer passed as one byte short: the documented code, outputs and fences untouched

No kernel is ever handed fewer real bytes than it declares, so a violation is a failed assertion, never a fault."""
import numpy as np
import pytest
import torch

import scratch_cases as S

pytestmark = pytest.mark.gpu

ROW_IDS = [r.name for r in S.ROWS]
_baselines = {}


def baseline(row, shape, dev):
    key = (row.name, shape)
    if key not in _baselines:
        p = row.shapes[shape]
        keep, regions = [], []
        for n in row.sizes(p):
            t = torch.zeros(max(2 * n, 256), dtype=torch.uint8, device=dev)      # zero-filled: the vote's contract as well
            keep.append(t)
            regions.append(S.Region(t.data_ptr(), t.numel(), t[:n]))
        rcs, outs = row.run(S.inputs_of(row, shape, dev), p, regions)
        host = outs.host()
        assert all(rc == 0 for rc in rcs), (row.name, shape, rcs)
        _baselines[key] = host
    return _baselines[key]


def fenced_regions(row, sizes, dev, pattern):
    """one poisoned Fenced per region (the vote's state block zeroed, never poisoned)"""
    fs = [S.Fenced(n, dev) for n in sizes]
    for f in fs:
        S.prepare(f.body, f.declared, row.state, pattern)
    return fs


def check_call(row, shape, dev, fs, tag):
    """run `shape` in the fenced buffers `fs`, each region passed at the shape's own declared size"""
    p = row.shapes[shape]
    sizes = row.sizes(p)
    assert all(n <= f.declared for n, f in zip(sizes, fs))
    regions = [S.Region(f.ptr, n, f.body[:n]) for n, f in zip(sizes, fs)]
    rcs, outs = row.run(S.inputs_of(row, shape, dev), p, regions)
    got = outs.host()
    assert all(rc == 0 for rc in rcs), (tag, rcs)
    assert S.same(got, baseline(row, shape, dev)) == [], tag
    assert all(f.intact() for f in fs), f"{tag}: a fence byte was written"


@pytest.mark.parametrize("pattern", S.POISONS)
@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("row", S.ROWS, ids=ROW_IDS)
def test_exact_size_fenced_and_poisoned(dev, row, shape, pattern):
    fs = fenced_regions(row, row.sizes(row.shapes[shape]), dev, pattern)
    check_call(row, shape, dev, fs, f"{row.name}/{shape}/{pattern}")


@pytest.mark.parametrize("pattern", S.POISONS)
@pytest.mark.parametrize("row", S.ROWS, ids=ROW_IDS)
def test_reuse_across_shapes_without_cleaning(dev, row, pattern):
    """what the grow-only scratch cache and the captured pipelines do: the buffer of the largest call serves every call, and
    nobody cleans it in between"""
    fs = fenced_regions(row, row.sizes(row.shapes["large"]), dev, pattern)
    for i, shape in enumerate(("large", "small", "large")):
        check_call(row, shape, dev, fs, f"{row.name}/{pattern}/call {i} ({shape})")


@pytest.mark.parametrize("pattern", S.POISONS)
@pytest.mark.parametrize("row", [r for r in S.ROWS if r.state], ids=[r.name for r in S.ROWS if r.state])
def test_vote_keeps_only_its_state_block_between_calls(dev, row, pattern):
    """the vote's workspace in use: the state block holds what the last call left (the rotation-table cache, the queue counters, the
    carry plane) and is left alone, everything behind it is dirtied again before every call -- a vote may trust its state block and
    nothing else, whatever the counters an earlier call of another shape left there"""
    fs = fenced_regions(row, row.sizes(row.shapes["large"]), dev, pattern)
    for i, shape in enumerate(("large", "small", "large", "large")):
        check_call(row, shape, dev, fs, f"{row.name}/{pattern}/call {i} ({shape})")
        for f in fs:
            S.dirty(f.body, f.declared, True, S.POISONS[(S.POISONS.index(pattern) + i + 1) % 2])


@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("row", S.ROWS, ids=ROW_IDS)
def test_one_byte_short_is_refused_before_anything_is_written(dev, row, shape):
    p = row.shapes[shape]
    sizes = row.sizes(p)
    for case in row.refusals(p):
        if all(sizes[i] == 0 for i in case):
            continue
        fs = fenced_regions(row, sizes, dev, "ff")
        regions = [S.Region(f.ptr, n - 1 if i in case and n > 0 else n, f.body) for i, (n, f) in enumerate(zip(sizes, fs))]
        rcs, outs = row.run(S.inputs_of(row, shape, dev), p, regions, short=True)
        touched = outs.touched()
        assert rcs and all(rc == row.refusal for rc in rcs), (row.name, shape, case, rcs)
        assert touched == [], (row.name, shape, case)
        assert all(f.intact() for f in fs)


def test_sel_pass_reads_the_table_that_is_present(dev):
    """include/cppf.h, cppf_pair_mlp_decode_sel: the workspace's per-point table "is reused, not rebuilt".  So after a first pass of
    the OTHER shape in the same buffer the small shape's selected pass gives the result of the table actually present: row i holds
    the projection of the large shape's feat[i], i.e. the result of a proper first pass on (pc, nrm, large feat[:N]) -- not a
    rebuilt table, and nothing read beyond the N rows."""
    row = S.BY_NAME["pair_mlp"]
    small, large = row.shapes["small"], row.shapes["large"]
    ins, inl = S.inputs_of(row, "small", dev), S.inputs_of(row, "large", dev)
    # expected: the first pass on the foreign features, then the selected pass, in clean scratch
    t = torch.zeros(2 * row.sizes(large)[0], dtype=torch.uint8, device=dev)
    clean = S.Region(t.data_ptr(), t.numel(), t)
    want = S.Outs(dev)
    assert row.decode(ins, small, clean, want, feat=inl["feat"][:small["N"]].contiguous()) == 0
    assert row.decode_sel(ins, small, clean, want) == 0
    want = want.host()
    (f,) = fenced_regions(row, row.sizes(large), dev, "ff")
    got = S.Outs(dev)
    assert row.decode(ins, small, S.Region(f.ptr, row.sizes(small)[0], f.body), got) == 0          # the small shape's own first pass,
    assert row.decode(inl, large, S.Region(f.ptr, f.declared, f.body), S.Outs(dev)) == 0            # the large one's in between,
    assert row.decode_sel(ins, small, S.Region(f.ptr, row.sizes(small)[0], f.body), got) == 0      # then the small selected pass
    got = got.host()
    assert np.array_equal(got["heads"], want["heads"]) and f.intact()
    own = baseline(row, "small", dev)["heads"]
    assert not np.array_equal(got["heads"], own)         # (the case bites: the foreign table changes the answer)


# ------------------------------------------------------------------------------------------------ end to end
def _d(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poison_scratch_cache(pattern):
    """every buffer of the grow-only scratch cache, in place -- the scoped scratch of captured pipelines included.  Nothing is written
    to the state region of the vote buffers (tags "vote..."): it keeps, byte for byte, what the last vote left there, and the next
    vote runs on that live state with everything behind it dirtied"""
    from cppf_amd import _torch_util as tu
    assert tu._ws_cache
    torch.cuda.synchronize()
    for (_, _, tag), buf in tu._ws_cache.items():
        S.dirty(buf, buf.numel(), tag.startswith("vote"), pattern)
    return len(tu._ws_cache)


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


@pytest.mark.parametrize("pattern", S.POISONS)
def test_pipelines_do_not_depend_on_what_the_scratch_cache_holds(golden, dev, pattern):
    """estimate_pose on a 512-point object, scene_poses on a two-object scene and one frame through the eager frame path; then every
    cached scratch buffer is poisoned in place and the three run again: the records are the same bits.  A captured PosePipeline
    likewise: run (capture), replay, poison its scratch, replay."""
    import os

    import cppf_amd.synthetic as syn
    import scene_poses_ref as SP
    from conftest import GOLDEN
    from cppf_amd import scene_poses, training
    from cppf_amd.config import CATEGORIES
    from cppf_amd.frames import frame_poses
    from cppf_amd.inference import PosePipeline, estimate_pose, grid_shape
    from cppf_amd.utils.util import read_depth_png
    from test_gpu_configs import make_encoder, seeded_sd
    from test_real_frame import DEPTH, instances
    d = _d(dev)
    sph = golden("sphere.npz")["pts"]
    enc = make_encoder(seeded_sd(0, 4.0), dev)
    ob = syn.make_object("mug", 512, 7)
    idx = syn.make_pairs(512, 24, 7)
    u_tr, u_rot = syn.make_uniforms(idx.shape[0], 7)
    sc = SP.perfect_scene("mug", 2, 1, pairs_per_object=60000, n_points=1024)
    depth = read_depth_png(DEPTH)
    inst = instances(depth)[:2]
    encs, pencs = {}, {}
    for cat, src in (("mug", "mug"), ("bowl", "bottle"), ("can", "bottle")):
        pencs[cat], encs[cat] = training.load_weights(os.path.join(GOLDEN, f"trained_{src}.npz"), CATEGORIES[src], dev)

    def three():
        r = estimate_pose(enc, d(ob["pc"]), d(ob["normals"]), d(ob["feat"]), d(idx), d(u_tr), d(u_rot), ob["cfg"], sph)
        one = _bytes(r["ws"].rec.cpu().numpy(), r["ws"].mask.cpu().numpy(), r["heads"].cpu().numpy(), r["outputs"].cpu().numpy())
        assert r["n_surv"] > 0
        out = scene_poses.scene_poses(None, d(sc["pc"]), d(sc["nrm"]), None, d(sc["idx"]), None, None, sc["cfg"], outputs=d(sc["outputs"]),
                                      heads=d(sc["heads"]), max_proposals=4)
        assert len(out["poses"]) >= 2
        two = _bytes(*out["proposals"], out["pairs"].cpu().numpy(), out["offsets"], out["surv_bits"].cpu().numpy(),
                     *[a for p in out["poses"] for a in (p["T"], p["R"], p["scale"], p["point_mask"])])
        poses = frame_poses(depth, inst, encs, pencs, n_pairs=20000, device=dev, seed=3)
        assert all(p is not None for p in poses)
        frame = _bytes(*[a for p in poses for a in (p["T"], p["up"], p["scale"], p["R"], np.array([p["argmax"], p["n_surv"]]))])
        return one, two, frame

    first = three()
    assert _poison_scratch_cache(pattern) >= 3
    again = three()
    for name, a, b in zip(("estimate_pose", "scene_poses", "frame_poses"), first, again):
        assert a == b, name

    corners, dims = grid_shape(ob["pc"], ob["cfg"].res)
    pp = PosePipeline(enc, ob["cfg"], 512, idx.shape[0], dims, dev, sph)
    pp.load(ob["pc"], ob["normals"], ob["feat"], idx, u_tr, u_rot, corners[0].copy())
    recs = []
    for step in range(3):                                    # capture, replay, poison, replay
        if step == 2:
            _poison_scratch_cache(pattern)
        pp.run()
        recs.append(_bytes(pp.ws.rec.cpu().numpy(), pp.ws.mask.cpu().numpy()))
    assert recs[0] == recs[1] == recs[2]
