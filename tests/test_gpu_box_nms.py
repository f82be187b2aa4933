"""cppf_box_nms_batch (csrc/box_nms.hip) on the device: the reference's pick lists (tests/golden/nms_cases.npz), evaluation.nms_3d's
host path, the IoUs of cppf_pose_eval_pairs bit for bit, one batched call against per-group calls, the bit-matrix word boundaries
with ties, the grid-stride loop, and run-to-run identical bytes."""
import numpy as np
import pytest
import torch

from cppf_amd import _lib
from cppf_amd import evaluation as E
from cppf_amd._torch_util import call, scratch

pytestmark = pytest.mark.gpu

OVER_LANES = 2048 * 64        # csrc/box_nms.hip: NMS_MAX_BLOCKS workgroups of 64 lanes -- more pairs than this enter the stride loop


@pytest.fixture(scope="module")
def z(golden):
    return golden("nms_cases.npz")


def _case(z, k):
    return z[f"RT_{k}"], z[f"scales_{k}"], z[f"scores_{k}"], float(z[f"thresh_{k}"]), z[f"pick_{k}"], z[f"iou_{k}"]


def _align(b):
    return (b + 255) & ~255


def _run(dev, RT, scales, scores, sizes, thresh):
    """one call on boxes in group order: (pick i32[n], n_pick i32[G], iou f64[pairs], the bit matrices' words u64)"""
    n, G = len(RT), len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    m = np.asarray(sizes, np.int64)
    n_pairs, n_words = int((m * (m - 1) // 2).sum()), int((m * ((m + 63) // 64)).sum())
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    pick = torch.full((n,), -7, dtype=torch.int32, device=dev)
    n_pick = torch.full((G,), -7, dtype=torch.int32, device=dev)
    iou = torch.full((max(n_pairs, 1),), -7.0, dtype=torch.float64, device=dev)
    ws = torch.full((_lib.lib().cppf_box_nms_workspace_bytes(n, G),), 0xA5, dtype=torch.uint8, device=dev)
    call("cppf_box_nms_batch", dev, d(RT), d(scales), d(scores), n, off, G, float(thresh), pick, n_pick, iou, scratch(ws))
    at = _align(4 * (G + 1)) + 2 * _align(8 * (G + 1))
    bits = ws[at:at + 8 * n_words].cpu().numpy().view(np.uint64)
    return pick.cpu().numpy(), n_pick.cpu().numpy(), iou.cpu().numpy()[:n_pairs], bits


def _lists(pick, n_pick, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    for a, b, k in zip(off[:-1], off[1:], n_pick):
        assert (pick[a + k:b] == -1).all() and (pick[a:a + k] >= 0).all()
    return [pick[a:a + k].tolist() for a, k in zip(off[:-1], n_pick)]


def _pairs_iou(dev, RT, scales):
    """cppf_pose_eval_pairs for every (i, j), i < j, the boxes on both sides, no sweep"""
    m = len(RT)
    i, j = np.triu_indices(m, 1)
    pairs = np.stack([i, j], -1).astype(np.int32)
    iou, _, _ = E.pose_metrics_device(RT, scales, RT, scales, np.zeros(m, np.int32), pairs, np.zeros(len(pairs), np.int32), device=dev)
    return iou.cpu().numpy()


def _random_boxes(rng, m, side, levels=None):
    from scipy.spatial.transform import Rotation
    RT = np.tile(np.eye(4), (m, 1, 1))
    RT[:, :3, :3] = Rotation.random(m, random_state=int(rng.integers(1 << 30))).as_matrix()
    RT[:, :3, 3] = rng.uniform(-0.5 * side, 0.5 * side, (m, 3))
    scales = rng.uniform(0.5, 1.5, (m, 3))
    scores = rng.permutation(m) + rng.uniform(0, 0.5, m) if levels is None else rng.integers(0, levels, m).astype(np.float64)
    return RT, scales, scores


def test_golden_pick_lists_and_the_host_path(z, dev):
    for k in range(int(z["n_cases"])):
        RT, scales, scores, thresh, want, want_iou = _case(z, k)
        pick, n_pick, iou, _ = _run(dev, RT, scales, scores, [len(RT)], thresh)
        (got,) = _lists(pick, n_pick, [len(RT)])
        assert got == want.tolist() and n_pick.tolist() == [len(want)], k
        assert len(iou) == 0 or np.abs(iou - want_iou).max() <= 1e-6
        (pub,) = E.nms_3d(RT, scales, scores, thresh, device=dev)             # the public entry: the same list, int64
        assert pub.dtype == np.int64 and pub.tolist() == want.tolist()
        if len(RT) <= 65:                                                      # (the host path on the larger case: test_box_nms_cpu)
            assert E.nms_3d(RT, scales, scores, thresh)[0].tolist() == got


def test_iou_out_is_pose_eval_pairs_bit_for_bit(z, dev):
    for k in (1, 2, 4, 5):
        RT, scales, scores, thresh, _, _ = _case(z, k)
        _, _, iou, _ = _run(dev, RT, scales, scores, [len(RT)], thresh)
        assert np.array_equal(iou.view(np.uint64), _pairs_iou(dev, RT, scales).view(np.uint64)), k
    # a rotation block that carries a scale: the same normalisation on both sides
    RT, scales, scores, thresh, _, _ = _case(z, 2)
    RT = RT.copy()
    RT[:, :3, :3] *= np.linspace(0.5, 2.0, len(RT))[:, None, None]
    _, _, iou, _ = _run(dev, RT, scales, scores, [len(RT)], thresh)
    assert np.array_equal(iou.view(np.uint64), _pairs_iou(dev, RT, scales).view(np.uint64))


def test_one_batched_call_equals_the_per_group_calls(z, dev):
    by_size = {len(z[f"scores_{k}"]): k for k in range(int(z["n_cases"]))}
    sizes = [0, 1, 65, 2, 0, 64, 130]
    cases = [_case(z, by_size[m]) for m in sizes if m]
    RT, scales, scores = (np.concatenate([c[i] for c in cases]) for i in range(3))
    pick, n_pick, iou, bits = _run(dev, RT, scales, scores, sizes, 0.3)
    want_pick, want_n, want_iou, want_bits = [], [], [], []
    for m in sizes:
        if m == 0:
            want_n.append(0)
            continue
        c = _case(z, by_size[m])
        p, k, u, b = _run(dev, c[0], c[1], c[2], [m], 0.3)
        assert p[:k[0]].tolist() == c[4].tolist()
        want_pick.append(p); want_n.append(int(k[0])); want_iou.append(u); want_bits.append(b)
    assert np.array_equal(pick, np.concatenate(want_pick)) and n_pick.tolist() == want_n          # slot for slot, the -1 fill included
    assert np.array_equal(iou.view(np.uint64), np.concatenate(want_iou).view(np.uint64))
    assert np.array_equal(bits, np.concatenate(want_bits))
    # two runs: identical bytes in pick, n_pick and the bit matrices
    pick2, n_pick2, _, bits2 = _run(dev, RT, scales, scores, sizes, 0.3)
    assert pick.tobytes() == pick2.tobytes() and n_pick.tobytes() == n_pick2.tobytes() and bits.tobytes() == bits2.tobytes()
    # the public entry over the same groups: indices into the caller's arrays
    gid = np.repeat(np.arange(len(sizes)), sizes)
    got = E.nms_3d(RT, scales, scores, 0.3, groups=gid, device=dev)
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert [g.tolist() for g in got] == [(off[i] + np.asarray(w)).tolist() for i, w in enumerate(_lists(pick, n_pick, sizes))]


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 128, 129])
def test_word_boundaries_with_ties_equal_the_host_path(dev, m):
    """crowded boxes (most are suppressed, across the 64-bit words of a row) with scores on 5 levels: ties everywhere"""
    rng = np.random.default_rng(100 + m)
    RT, scales, scores = _random_boxes(rng, m, 0.8, levels=5)
    pick, n_pick, _, _ = _run(dev, RT, scales, scores, [m], 0.3)
    (got,) = _lists(pick, n_pick, [m])
    (want,) = E.nms_3d(RT, scales, scores, 0.3)
    assert got == want.tolist()
    assert m < 6 or len(np.unique(scores)) < m                              # (ties are present)


def test_the_stride_loop_on_one_large_group(dev):
    """nms_over_kernel's grid is capped at 2 048 workgroups of 64 lanes; a single group of 520 boxes has 134 940 pairs, more than
    its 131 072 lanes, so the last pairs are served by the second trip of the loop.  Checked against cppf_pose_eval_pairs and a numpy
    greedy on the device's own IoU matrix (the host IoU would take minutes here)."""
    m = 520
    assert m * (m - 1) // 2 > OVER_LANES
    rng = np.random.default_rng(7)
    RT, scales, scores = _random_boxes(rng, m, 3.0, levels=40)
    pick, n_pick, iou, bits = _run(dev, RT, scales, scores, [m], 0.3)
    assert np.array_equal(iou.view(np.uint64), _pairs_iou(dev, RT, scales).view(np.uint64))
    full = np.zeros((m, m))
    full[np.triu_indices(m, 1)] = iou
    full = full + full.T
    over = full > 0.3
    wpr = (m + 63) // 64
    rows = np.zeros((m, wpr * 64), bool)
    rows[:, :m] = over
    assert np.array_equal(bits, np.packbits(rows.reshape(m, wpr, 64), axis=-1, bitorder="little").view(np.uint64).reshape(-1))
    order = np.argsort(scores, kind="stable")[::-1]
    alive, want = np.ones(m, bool), []
    for i in order:
        if alive[i]:
            want.append(int(i))
            alive &= ~over[i]
    (got,) = _lists(pick, n_pick, [m])
    assert got == want and 10 < len(want) < m
