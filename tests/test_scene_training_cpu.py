"""cppf_amd.scene_training without a device: the loss from compact targets against training.loss_fn on their dense expansion, the
numpy restatement of the stratified draw, and the fp64 restatement of the targets (tests/scene_training_ref.py) against
training.targets in torch fp32 -- the yardstick the device test measures the kernel with."""
import numpy as np
import pytest
import torch

import scene_training_ref as R
from cppf_amd import scene_training as ST
from cppf_amd import synthetic as syn
from cppf_amd import training

EPS = 2.0 ** -24                          # fp32 unit roundoff


def _compact(scene, idx):
    """targets_ref's dict as the torch tensors the kernel writes (CPU)"""
    cfg = scene["cfg"]
    t = R.targets_ref(scene["pc"], scene["nrm"], scene["inst"], idx, scene["table"], scene["flags"], cfg.vote_range, cfg.tr_num_bins,
                      cfg.rot_num_bins)
    return dict(kind=torch.from_numpy(t["kind"]), pair_inst=torch.from_numpy(t["pair_inst"]), low=torch.from_numpy(t["low"].astype(np.uint8)),
                w_low=torch.from_numpy(t["w_low"].astype(np.float32)), aux=torch.from_numpy(t["aux"]))


def _preds(P, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.randn((1, P, cfg.out_dim), generator=g)).requires_grad_(True)


def _pairs(n_points, P, seed):
    return np.random.default_rng(seed).integers(0, n_points, (P, 2)).astype(np.int32)


@pytest.mark.parametrize("cat", ["bottle", "mug"])                       # without and with the right head
def test_loss_equals_loss_fn_on_dense_targets(cat):
    scene = R.posed_scene([cat], cat, 300, seed=1)
    cfg, P = scene["cfg"], 1000
    t = _compact(scene, _pairs(300, P, 2))
    assert bool((t["kind"] == 1).all())
    table = torch.from_numpy(scene["table"])
    tr, rot, aux, scale = ST.dense_targets(t, cfg, table)
    assert tr.shape == (P, 2, cfg.tr_num_bins) and rot.shape == (P, 2, cfg.rot_num_bins) and scale.shape == (P, 3)
    assert torch.allclose(tr.sum(-1), torch.ones(P, 2), atol=1e-6) and torch.allclose(rot.sum(-1), torch.ones(P, 2), atol=1e-6)
    pa, pb = _preds(P, cfg, 3), _preds(P, cfg, 3)
    la = ST.scene_loss_fn(pa, t, table, cfg)
    lb = training.loss_fn(pb, tr, rot, aux, scale[0], cfg)
    # both are fp32 tree sums of the same P terms per head: 10 log2(n) eps covers any order
    assert abs(float(la.detach()) - float(lb.detach())) <= 1e-5 * abs(float(lb.detach())), (float(la.detach()), float(lb.detach()))
    la.backward(), lb.backward()
    gmax = float(pb.grad.abs().max())
    assert gmax > 0 and float((pa.grad - pb.grad).abs().max()) <= 1e-5 * gmax


def test_scale_term_uses_each_pairs_own_row():
    scene = R.posed_scene(["mug", "mug"], "mug", 300, seed=4)
    cfg = scene["cfg"]
    assert np.abs(scene["table"][0, 9:12] - scene["table"][1, 9:12]).max() > 1e-3          # two sizes
    m, off = R.members_ref(scene["inst"], scene["flags"])
    idx = R.draw_ref(m, off, scene["inst"], 300, 800, 800, seed=5)
    t = _compact(scene, idx)
    k = t["pair_inst"].long()
    assert bool((t["kind"] == 1).all()) and 0 < int((k == 0).sum()) < 800
    table = torch.from_numpy(scene["table"])
    pr = _preds(800, cfg, 6).detach()
    tr, rot, aux, _ = ST.dense_targets(t, cfg)
    want = sum(float((k == j).sum()) / 800 * training.loss_fn(pr[:, k == j], tr[k == j], rot[k == j], aux[k == j], table[j, 9:12], cfg)
               for j in (0, 1))
    got = ST.scene_loss_fn(pr, t, table, cfg)
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    # the rows matter: predictions that hit every pair's own row have no scale term; with the rows swapped the term is |s0 - s1|^2 / 3
    p64, t64 = pr.double().clone(), table.double()
    p64[0, :, -3:] = t64[k][:, 9:12]
    gap = float(ST.scene_loss_fn(p64, t, t64[[1, 0]], cfg)) - float(ST.scene_loss_fn(p64, t, t64, cfg))
    assert abs(gap - float(((t64[0, 9:12] - t64[1, 9:12]) ** 2).sum() / 3)) <= 1e-9


def test_negatives_are_ignored_exactly_or_pulled_to_the_far_bin():
    scene = R.posed_scene(["bottle", "can", "bottle"], "bottle", 300, seed=7, n_background=60)
    cfg, P = scene["cfg"], 1000
    t = _compact(scene, _pairs(360, P, 8))
    neg, pos = t["kind"] == 0, t["kind"] == 1
    assert int(neg.sum()) > 100 and int(pos.sum()) > 50
    table = torch.from_numpy(scene["table"])
    pa = _preds(P, cfg, 9)
    la = ST.scene_loss_fn(pa, t, table, cfg, neg_weight=0.0)
    la.backward()
    assert float(pa.grad[0, neg].abs().max()) == 0.0 and float(pa.grad[0, pos].abs().max()) > 0
    pb = pa.detach().clone()
    pb[0, neg] = 7.0 * torch.randn((int(neg.sum()), cfg.out_dim), generator=torch.Generator().manual_seed(10))
    assert float(ST.scene_loss_fn(pb, t, table, cfg)) == float(la.detach())                          # bit for bit
    # positives only: the same value as the loss of the positives' rows alone
    sub = {k: v[pos] for k, v in t.items()}
    alone = ST.scene_loss_fn(pa.detach()[:, pos], sub, table, cfg)
    assert abs(float(alone) - float(la)) <= 1e-5 * abs(float(la))
    # neg_weight > 0: plus the KL of the one-hot farthest nu bin against the nu head, averaged over the negatives
    tb = cfg.tr_num_bins
    nu = pa.detach()[0, :, tb:2 * tb]
    hand = -(torch.log_softmax(nu[neg].double(), -1)[:, tb - 1]).mean()
    lw = ST.scene_loss_fn(pa.detach(), t, table, cfg, neg_weight=0.25)
    assert abs(float(lw) - (float(la) + 0.25 * float(hand))) <= 1e-5 * abs(float(lw))


def test_kind_255_takes_no_part():
    scene = R.posed_scene(["bottle"], "bottle", 300, seed=11)
    cfg = scene["cfg"]
    idx = _pairs(300, 257, 12)
    idx[5, 1], idx[200, 0] = 300, -1
    t = _compact(scene, idx)
    assert t["kind"][5] == 255 and t["kind"][200] == 255 and int((t["kind"] == 255).sum()) == 2
    table = torch.from_numpy(scene["table"])
    p = _preds(257, cfg, 13)
    ST.scene_loss_fn(p, t, table, cfg, neg_weight=0.5).backward()
    assert float(p.grad[0, [5, 200]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------- the draw
def _labels(seed, n=300):
    rng = np.random.default_rng(seed)
    inst = rng.integers(-1, 3, n).astype(np.int32)                        # background, instances 0..2
    return inst, np.array([1, 0, 1], np.int32)                            # instance 1 is of another category: an empty segment


def test_draw_restatement():
    inst, flags = _labels(1)
    N, P, P_pos, seed = inst.shape[0], 1000, 600, 0xC0FFEE1234
    members, seg_off = R.members_ref(inst, flags)
    assert seg_off[1] == seg_off[2] and seg_off[3] == members.shape[0] > 0
    assert all(np.all(np.diff(members[seg_off[k]:seg_off[k + 1]]) > 0) for k in range(3))
    idx = R.draw_ref(members, seg_off, inst, N, P, P_pos, seed)
    a, b = idx[:P_pos, 0], idx[:P_pos, 1]
    assert np.all(inst[a] == inst[b]) and np.all((flags[inst[a]] & 1) == 1) and np.all(inst[a] >= 0)
    assert set(np.unique(inst[a])) == {0, 2}
    p = np.arange(P, dtype=np.uint64)
    w = syn.philox4x32_10([p, 0 * p, 0 * p + np.uint64(4), 0 * p], seed)
    uni = np.stack([(w[0] * np.uint64(N)) >> np.uint64(32), (w[1] * np.uint64(N)) >> np.uint64(32)], -1).astype(np.int32)
    assert np.array_equal(idx[P_pos:], uni[P_pos:])
    assert not np.array_equal(uni[:, 0], syn.philox_pairs(seed, P, N)[0][:, 0])          # stream 4 is not the uniform draw's stream 0
    # a pair's draw depends on (seed, p) alone
    assert np.array_equal(R.draw_ref(members, seg_off, inst, N, 257, 257, seed), R.draw_ref(members, seg_off, inst, N, P, P, seed)[:257])
    # no member: every pair is uniform
    m0, off0 = R.members_ref(inst, np.zeros(3, np.int32))
    assert m0.shape[0] == 0 and np.array_equal(R.draw_ref(m0, off0, inst, N, P, P, seed), uni)


# ---------------------------------------------------------------------------------------- fp64 restatement against torch fp32
def deviation(scene, idx, ob, t64):
    """how far training.targets (torch fp32, CPU) is from the fp64 restatement on the positives of t64: dict(tr, rot: the largest
    deviation of a dense soft target on the mu / nu heads and, with the hard pairs set aside, on the angle heads; hard: the fraction
    set aside; aux_mismatch: sign targets that differ where |n . axis| >= 1e-6)"""
    cfg = scene["cfg"]
    tr64, rot64 = R.dense_all(t64, cfg.tr_num_bins, cfg.rot_num_bins)
    tr32, rot32, aux32 = R.torch_targets(scene["pc"], scene["nrm"], idx, ob, cfg)
    hard = R.hard_pairs(t64, cfg.res)
    ok = t64["aux_margin"] >= 1e-6
    return dict(tr=float(np.abs(tr32 - tr64).max()), rot=float(np.abs(rot32 - rot64)[~hard].max()), hard=float(hard.mean()),
                aux_mismatch=int(((aux32 != t64["aux"]) & ok).sum()), aux_unclear=float((~ok).any(-1).mean()))


@pytest.mark.parametrize("cat", ["bottle", "mug", "laptop"])
def test_restatement_against_training_targets(cat):
    """The yardstick of the device test.  Bounds from the number format, not from a run: with r = the largest distance of a point from
    its centre, a mu / nu value is a chain of fewer than 32 fp32 roundings of quantities <= r, so its bin coordinate x = value /
    interval is off by at most 32 eps r / interval (+ 32 eps of x itself); a cosine of u with an axis is off by at most 4 eps r / |d| +
    8 eps, |d| >= res, and acos' slope is at most 1 / sqrt(1 - 0.999^2) once the hard pairs are set aside."""
    worst = dict(tr=0.0, rot=0.0, hard=0.0)
    for seed in (1, 2, 3):
        scene = R.posed_scene([cat], cat, 2048, seed=seed)
        cfg, ob = scene["cfg"], scene["obs"][0]
        assert 0.8 < np.linalg.norm(ob["center"]) < 1.6                                   # about 1 m away, as a frame's cloud is
        idx = _pairs(2048, 20000, 100 + seed)
        t64 = R.targets_ref(scene["pc"], scene["nrm"], scene["inst"], idx, scene["table"], scene["flags"], cfg.vote_range, cfg.tr_num_bins,
                            cfg.rot_num_bins)
        assert np.all(t64["kind"] == 1) and np.all(t64["low"] <= np.array([cfg.tr_num_bins - 2] * 2 + [cfg.rot_num_bins - 2] * 2))
        assert np.all((t64["w_low"] >= 0) & (t64["w_low"] <= 1))
        dv = deviation(scene, idx, ob, t64)
        print(f"{cat} seed {seed}: torch fp32 against fp64: mu/nu {dv['tr']:.3g}, angles {dv['rot']:.3g} with {100 * dv['hard']:.2f} % set "
              f"aside, aux mismatches {dv['aux_mismatch']}, pairs with an unclear sign {100 * dv['aux_unclear']:.3f} %")
        r = float(np.linalg.norm(scene["pc"].astype(np.float64) - ob["center"], axis=-1).max())
        int_tr = min(2 * cfg.vote_range[0], cfg.vote_range[1]) / (cfg.tr_num_bins - 1)
        assert dv["tr"] <= 32 * EPS * r / int_tr + 32 * EPS * cfg.tr_num_bins
        assert dv["rot"] <= (4 * EPS * r / cfg.res + 8 * EPS) / np.sqrt(1 - 0.999 ** 2) / (np.pi / (cfg.rot_num_bins - 1)) + 32 * EPS * cfg.rot_num_bins
        assert dv["hard"] <= 0.03 and dv["aux_mismatch"] == 0 and dv["aux_unclear"] <= 0.01
        for k in worst:
            worst[k] = max(worst[k], dv[k])
    print(f"{cat}: worst of seeds 1-3: mu/nu {worst['tr']:.3g}, angles {worst['rot']:.3g}, set aside {100 * worst['hard']:.2f} %")
