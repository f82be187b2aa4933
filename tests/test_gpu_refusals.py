"""An instance the shape-polymorphic vote REFUSES on BatchPoseRunner's staged path (records assembled on the device, nothing read
back): the contract of the class docstring -- the refused row is poisoned (NaN in columns 0..11, -1 in column 12), the other rows
are untouched, every batch's late check is kept in a FIFO, check() / a later run() report the refusal exactly once with the batch's
sequence number and the objects' indices, and the runner serves the next batch as a fresh one would.

How a refusal is provoked (no fault involved; FrameRunner lives on the same mechanism, test_real_frame.py): put() honours a
caller's `dims`, so a cloud stretched x2 about its centre is handed over with the dims of the unstretched cloud.  The host picks a
few-tile pipeline from the claim; the chain's first launch computes the real dims from the cloud, the vote finds they need more
tiles than its class holds, writes arg-max -1 / peak NaN and votes nothing (test_dyn_vote_reports_a_record_beyond_its_capacities,
test_tile_capacity_classes), and the pose tail runs on.  Read for index -1 before this was run: center_from_argmax_body only
divides and multiplies the index (T = corner + c * res: finite garbage, no address is formed from it), backvote_body takes that T
as `gt_center` -- arithmetic and comparisons against the dims record, no grid access at all -- and everything behind it indexes by
pair, never by cell.  Every comparison here is exact: integers, NaN-ness, bit equality against a fresh runner."""
import numpy as np
import pytest
import torch

from cppf_amd import _lib, sharding
from cppf_amd.batch import BatchPoseRunner
from cppf_amd.config import NOCS_CATEGORIES
from cppf_amd.inference import grid_class, grid_shape
from test_gpu_configs import make_encoder, seeded_sd
from test_gpu_resident import mixed_batch

pytestmark = pytest.mark.gpu

P = 20000


@pytest.fixture(scope="module")
def encoders(dev):
    sd = seeded_sd(4, 4.0)
    return {c: make_encoder(sd, dev) for c in NOCS_CATEGORIES}


@pytest.fixture(autouse=True)
def collect_dead_runners():
    """An exception a test caught keeps its traceback, the traceback the test's frame, the frame the runner: a reference cycle, so the
    dead runner -- pipelines, chains, captured graphs -- would wait for a cycle collection at some later moment of some later test.
    It goes here, while nothing is being captured."""
    yield
    import gc
    gc.collect()


def good_batch(seed0):
    return mixed_batch(4, (600, 1000, 800), P, seed0)


def on_device(objs, dev, dims=None):
    out = []
    for j, o in enumerate(objs):
        d = dict(o, pc=torch.from_numpy(o["pc"]).to(dev), normals=torch.from_numpy(o["normals"]).to(dev),
                 feat=torch.from_numpy(o["feat"]).to(dev))
        if dims is not None:
            d["dims"] = dims[j]
        out.append(d)
    return out


def refused_batch(seed0, bad):
    """good_batch(seed0) with object `bad` stretched x2 about its centre and every object's dims CLAIMED to be those of the
    unstretched cloud -> (host objects, claimed dims).  Asserted from grid_class alone: the claim passes set_shape on a few-tile
    pipeline, the real grid needs more tiles than that class holds -- so the device must refuse it, and only it."""
    objs = good_batch(seed0)
    claimed = [grid_shape(o["pc"], o["cfg"].res)[1] for o in objs]
    pc = objs[bad]["pc"]
    c = (pc.min(0) + pc.max(0)) / 2
    objs[bad] = dict(objs[bad], pc=np.ascontiguousarray(((pc - c) * 2 + c).astype(np.float32)))
    for j, o in enumerate(objs):
        T_claim, many_claim, cells_claim = grid_class(claimed[j])
        T_real = grid_class(grid_shape(o["pc"], o["cfg"].res)[1])[0]
        assert 1 <= T_claim <= _lib.tiles_cap(many_claim) and int(np.prod(claimed[j])) <= cells_claim       # the claim passes set_shape
        if j == bad:
            assert many_claim == 0 and (T_real == 0 or T_real > _lib.tiles_cap(many_claim)), (j, T_real, many_claim)
        else:
            assert grid_shape(o["pc"], o["cfg"].res)[1] == claimed[j]
    return objs, claimed


def fresh_records(encoders, dev, seed0, seed):
    fresh = BatchPoseRunner(encoders, dev)
    out = fresh.run(fresh.put(good_batch(seed0)), seed=seed).cpu().numpy()
    fresh.check()
    assert (out[:, 12] >= 0).all()
    return out


def assert_refused_row(rec, j):
    assert np.isnan(rec[j, 0:12]).all(), rec[j]
    assert rec[j, 12] == -1 and np.isnan(rec[j, 13]) and rec[j, 15] == j and (rec[j, 16:] == 0).all(), rec[j]
    assert np.isfinite(rec[j, 14])


def assert_report(err, batch, ids):
    assert isinstance(err, _lib.CppfError)
    assert err.batch == batch and list(err.object_ids) == list(ids)
    assert f"batch {batch}" in str(err) and str(list(ids)) in str(err), str(err)


def run_reporting(runner, batch, seed, reports):
    """run(); a late report of an EARLIER batch is noted and the run repeated, as the contract says a caller does"""
    try:
        return runner.run(batch, seed=seed)
    except _lib.CppfError as e:
        reports.append(e)
        return runner.run(batch, seed=seed)


def drain(runner, reports):
    for _ in range(8):
        try:
            runner.check()
            return
        except _lib.CppfError as e:
            reports.append(e)
    raise AssertionError("check() keeps raising")


def test_refused_row_is_poisoned_and_check_reports_it_once(encoders, dev):
    """(a) a refused batch, then check(): the row, the other rows against a fresh runner, the error, and the runner afterwards"""
    runner = BatchPoseRunner(encoders, dev)
    objs, claimed = refused_batch(500, bad=0)
    rec = runner.run(runner.put(on_device(objs, dev, claimed)), seed=3)
    assert rec.is_cuda and rec.shape == (4, sharding.RECORD)
    rec = rec.cpu().numpy()
    assert_refused_row(rec, 0)
    want = fresh_records(encoders, dev, 500, 3)                  # (row j is a function of the seed, j and object j alone)
    np.testing.assert_array_equal(rec[1:], want[1:])
    with pytest.raises(_lib.CppfError) as ei:
        runner.check()
    assert_report(ei.value, 0, [0])
    runner.check()                                               # reported once; nothing outstanding: returns
    assert not runner._checks and not runner._reports
    # the runner stays usable: the same pipelines serve the good batch as a fresh runner would
    again = runner.run(runner.put(good_batch(500)), seed=3).cpu().numpy()
    np.testing.assert_array_equal(again, want)
    runner.check()


def test_a_refusal_is_not_lost_when_later_batches_arrive_before_its_snapshot_lands(encoders, dev):
    """(b) overlap_batches: a refused batch and two good ones without a synchronisation; the snapshot's event is MADE to answer
    'not yet' when the second batch looks (a stub, no race with the device).  The refusal surfaces from a later run() or from
    check(), exactly once, naming batch 0; every good batch's records are its own"""
    runner = BatchPoseRunner(encoders, dev, overlap_batches=True)
    objs, claimed = refused_batch(520, bad=0)
    goods = [good_batch(540), good_batch(560)]
    inputs = [runner.put(on_device(objs, dev, claimed))] + [runner.put(g) for g in goods]
    reports, asked = [], []
    r0 = runner.run(inputs[0], seed=0)
    ev = runner._checks[-1]["ev"]
    assert runner._checks[-1]["batch"] == 0

    def not_yet():
        asked.append(1)
        del ev.query                                             # (the event's own query from here on)
        return False
    ev.query = not_yet
    r1 = runner.run(inputs[1], seed=1)                           # looks, is told 'not yet', must keep batch 0's check
    assert asked == [1] and [c["batch"] for c in runner._checks] == [0, 1] and not reports
    r2 = run_reporting(runner, inputs[2], 2, reports)
    drain(runner, reports)
    assert len(reports) == 1
    assert_report(reports[0], 0, [0])
    r0, r1, r2 = (r.cpu().numpy() for r in (r0, r1, r2))
    assert_refused_row(r0, 0)
    np.testing.assert_array_equal(r0[1:], fresh_records(encoders, dev, 520, 0)[1:])
    np.testing.assert_array_equal(r1, fresh_records(encoders, dev, 540, 1))
    np.testing.assert_array_equal(r2, fresh_records(encoders, dev, 560, 2))


def test_a_later_run_reports_the_old_batch_before_it_enqueues_the_new_one(encoders, dev):
    """the snapshot HAS landed (a device synchronisation) when the next batch comes: that run() raises, naming batch 0, and has
    enqueued nothing -- no check queued, no sequence number used; the same call again is batch 1 and equals a fresh runner's"""
    runner = BatchPoseRunner(encoders, dev)
    objs, claimed = refused_batch(580, bad=0)
    runner.run(runner.put(on_device(objs, dev, claimed)), seed=5)
    good = runner.put(good_batch(580))
    torch.cuda.synchronize()
    with pytest.raises(_lib.CppfError) as ei:
        runner.run(good, seed=6)
    assert_report(ei.value, 0, [0])
    assert not runner._checks and not runner._reports and runner._batch_no == 1
    rec = runner.run(good, seed=6)
    assert [c["batch"] for c in runner._checks] == [1]
    np.testing.assert_array_equal(rec.cpu().numpy(), fresh_records(encoders, dev, 580, 6))
    runner.check()
    assert not runner._checks


def test_a_refusal_in_the_runners_last_batch_is_reported_by_check(encoders, dev):
    """(c) a good batch, then a refused one as the last thing the runner does: run() never comes again, check() reports batch 1"""
    runner = BatchPoseRunner(encoders, dev)
    reports = []
    good = run_reporting(runner, runner.put(good_batch(600)), 7, reports)
    objs, claimed = refused_batch(620, bad=2)
    rec = run_reporting(runner, runner.put(on_device(objs, dev, claimed)), 8, reports)
    assert not reports
    with pytest.raises(_lib.CppfError) as ei:
        runner.check()
    assert_report(ei.value, 1, [2])
    runner.check()
    rec = rec.cpu().numpy()
    assert_refused_row(rec, 2)
    want = fresh_records(encoders, dev, 620, 8)
    np.testing.assert_array_equal(rec[[0, 1, 3]], want[[0, 1, 3]])
    np.testing.assert_array_equal(good.cpu().numpy(), fresh_records(encoders, dev, 600, 7))


def test_refusals_in_two_batches_are_reported_in_order(encoders, dev):
    """(d) batches 0 and 2 refused (different objects), batch 1 good: two reports, oldest first, each exactly once"""
    runner = BatchPoseRunner(encoders, dev, overlap_batches=True)
    reports = []
    a, claimed_a = refused_batch(640, bad=0)
    b, claimed_b = refused_batch(660, bad=2)
    run_reporting(runner, runner.put(on_device(a, dev, claimed_a)), 0, reports)
    mid = run_reporting(runner, runner.put(good_batch(680)), 1, reports)
    last = run_reporting(runner, runner.put(on_device(b, dev, claimed_b)), 2, reports)
    drain(runner, reports)
    assert len(reports) == 2
    assert_report(reports[0], 0, [0])
    assert_report(reports[1], 2, [2])
    assert_refused_row(last.cpu().numpy(), 2)
    np.testing.assert_array_equal(mid.cpu().numpy(), fresh_records(encoders, dev, 680, 1))
    # ... and the runner serves a good batch afterwards
    np.testing.assert_array_equal(runner.run(runner.put(good_batch(680)), seed=1).cpu().numpy(), fresh_records(encoders, dev, 680, 1))
    runner.check()


def test_check_of_a_good_batch_returns_and_adapts_the_chains(encoders, dev):
    """(e) a good batch alone: check() returns at once the second time, and every chain's form follows its members' survivor
    shares exactly as PoseChain.adapt decides (what the late look did before check() existed)"""
    runner = BatchPoseRunner(encoders, dev)
    runner.check()                                               # nothing outstanding
    rec = runner.run(runner.put(good_batch(700)), seed=4).cpu().numpy()
    ran = runner._checks[-1]["ran"]
    assert len(runner._checks) == 1 and sorted(s for _, slots in ran for s in slots) == [0, 1, 2, 3]
    runner.check()
    assert not runner._checks
    runner.check()
    for chain, slots in ran:
        share = float(np.mean([rec[s, 14] / P for s in slots]))
        assert 0 < share <= 1
        want = True if share > chain.FULL_FIRST_ON else (False if share < chain.FULL_FIRST_OFF else False)      # (a new chain starts split)
        assert chain.full_first == want, (slots, share)


def test_no_cycle_collection_can_run_inside_a_capture(encoders, dev, monkeypatch):
    """A dead runner in a reference cycle (the tests above leave such: a caught exception's traceback holds the frame that holds the
    runner) is freed by whichever cycle collection comes next, and its chains' __del__ drops their captured graphs.  Inside another
    chain's capture that aborts the process, so _GraphCache.run captures with the collector off and puts it back: observed here from
    the chain's own launches -- the two warm-up runs with the collector on, the captured one with it off, on again afterwards."""
    import gc
    from cppf_amd import inference
    assert gc.isenabled()
    runner = BatchPoseRunner(encoders, dev)
    objs = runner.put(good_batch(720))
    first = runner.run(objs, seed=1).cpu().numpy()                    # a combination's first sighting runs eagerly
    seen, orig = [], inference.PoseChain._chain

    def spy(self):
        seen.append((bool(torch.cuda.is_current_stream_capturing()), gc.isenabled()))
        return orig(self)
    monkeypatch.setattr(inference.PoseChain, "_chain", spy)
    second = runner.run(objs, seed=1).cpu().numpy()                   # the second is captured
    assert gc.isenabled()
    capturing = [on for cap, on in seen if cap]
    assert capturing and not any(capturing), seen                      # every captured run: collector off
    assert [on for cap, on in seen if not cap] and all(on for cap, on in seen if not cap), seen      # the warm-up runs: on
    np.testing.assert_array_equal(first, second)
    runner.check()
