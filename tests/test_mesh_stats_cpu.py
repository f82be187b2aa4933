"""CPU checks of the mesh statistics (cppf_amd/mesh_stats.py, tests/mesh_stats_ref.py) and of the category files
(cppf_amd/config.py): the restatement against the reference's own generate_target and gen_stats.py body (executed by
tests/golden/make_golden_stats.py), Open3D's count rule, the Philox twin, the YAML reader and writer, right_sym targets."""
import dataclasses
import glob
import os

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_stats_cases as MC
import mesh_stats_ref as SR
from cppf_amd import config, mesh_stats as MS, training
from cppf_amd.config import CATEGORIES
from cppf_amd.synthetic import philox4x32_10

GOLDEN_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config")
TAGS = ("plain", "rightsym", "rightsym_zright_upsym")


def test_pair_arithmetic_reproduces_generate_target_bit_for_bit(golden):
    g = golden("stats.npz")
    pc = g["pc"]
    for tag in TAGS:
        idx = g[f"{tag}.point_idxs"]
        proj, dist = SR.pair_targets(pc[idx[:, 0]], pc[idx[:, 1]])
        ref = g[f"{tag}.targets_tr"]
        assert ref.dtype == np.float32
        assert np.array_equal(proj.astype(np.float32), ref[:, 0]) and np.array_equal(dist.astype(np.float32), ref[:, 1]), tag
    # the flags change targets_rot only, never targets_tr (include/cppf.h: why the statistics take no flags)
    assert all(np.array_equal(g[f"{t}.targets_tr"], g["plain.targets_tr"]) for t in TAGS)
    assert not np.array_equal(g["rightsym.targets_rot"], g["plain.targets_rot"])


def test_restatement_reproduces_gen_stats(golden):
    """gen_stats.py's body, executed on fixed point sets with its own generate_target drawing from np.random.seed(SEED): the same
    per-mesh rows from the restatement (given the same pairs) aggregate to the reference's printed figures"""
    g = golden("stats.npz")
    M, P = int(g["gen.n_meshes"]), int(g["gen.n_pairs"])
    np.random.seed(int(g["gen.seed"]))
    rows = []
    for k in range(M):
        pts = g[f"gen.points{k}"]
        idx = np.random.randint(0, pts.shape[0], size=[P, 2])          # the draw generate_target made (legacy RandomState stream)
        assert np.array_equal(idx[:64], g[f"gen.first_pairs{k}"])
        rows.append(SR.mesh_row(pts, idx))
    for agg in (SR.aggregate(rows), MS.aggregate(np.array(rows))):
        np.testing.assert_allclose(agg["scale_range"], g["gen.scale_range"], rtol=2e-16, atol=0)   # numpy's 1-D norm: its own dot
        assert np.array_equal(np.array(agg["vote_range"], np.float32), g["gen.vote_range"])
        assert np.array_equal(agg["scale_mean"], g["gen.scale_mean"])
    printed = str(g["gen.printed"]).splitlines()
    ours = MS.format_stats(MS.aggregate(np.array(rows))).splitlines()
    assert [ln.split(":")[0] for ln in ours] == [ln.split(":")[0] for ln in printed] == ["scale_range", "vote_range", "scale_mean"]
    assert ours[2] == printed[2]


def _meshes():
    v0, f0 = R.box(0.2, 0.2, 0.2)[:2]
    v_deg = np.vstack([v0, [[0.0, 0.0, 0.3], [0.1, 0.1, 0.3], [0.2, 0.2, 0.3]]])
    f_deg = np.vstack([f0, [[0, 0, 1], [8, 9, 10], [3, 3, 3]]]).astype(np.int32)
    return [R.box()[:2], R.uv_sphere(0.5, 16, 32), R.necked_cylinder(), (v_deg, f_deg), R.uv_sphere(0.3, 64, 128)]


def test_counts_follow_open3d_rule_and_sum_to_n():
    for v, f in _meshes():
        a = SR.areas(v, f)
        q = a / SR.blocked_total(a)
        C = SR.blocked_cumsum(q)
        for n in (1, 7, 2048, 5000):
            E = SR.counts_end(C, n)
            cnt = np.diff(np.concatenate([[0], E]))
            assert cnt.sum() == n and (cnt >= 0).all()
            assert np.array_equal(cnt, SR.open3d_counts(C, n)), (f.shape, n)
            assert (cnt[a == 0] == 0).all()
            pts, t, E2, ok = SR.sample_surface(v, f, n, seed=3)
            assert ok and np.array_equal(np.bincount(t, minlength=f.shape[0]), cnt)
    # end counts that decrease behind a block boundary (tests/mesh_stats_cases.py): the counts are the steps of E's running maximum
    for i, case in enumerate(MC.DIP_CASES):
        v, f, Cc, E = MC.dip_case(i)
        n = case["N"]
        assert (np.diff(E) < 0).any()
        cnt = np.diff(np.concatenate([[0], np.maximum.accumulate(E)]))
        assert cnt.sum() == n and np.array_equal(cnt, SR.open3d_counts(Cc, n)), (case["F"], n)
        assert (cnt[SR.areas(v, f) == 0] == 0).all()
        assert np.array_equal(np.bincount(MC.dip_sample(i)[1], minlength=f.shape[0]), cnt)
    # F <= 1024: the blocked order is Open3D's serial chain; F > 1024 (the 16 384-face sphere) is blocked
    v, f = R.box()[:2]
    a = SR.areas(v, f)
    S = 0.0
    for x in a:
        S = S + x
    c, serial = 0.0, []
    for x in a / S:
        c = c + x
        serial.append(c)
    assert SR.blocked_total(a) == S and np.array_equal(SR.blocked_cumsum(a / S), serial)


def test_round_is_std_round():
    x = np.array([0.5, 1.5, 2.5, 0.49999999999999994, 2047.5, 3.0, 0.0])
    assert SR.round_half_away(x).tolist() == [1.0, 2.0, 3.0, 0.0, 2048.0, 3.0, 0.0]
    assert np.round(x).tolist() != SR.round_half_away(x).tolist()


def test_sampled_points_lie_on_their_faces():
    for v, f in _meshes()[:3]:
        pts, t, _, ok = SR.sample_surface(v, f, 2048, seed=1, mesh=4)
        p0, p1, p2 = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
        nrm = np.cross(p1 - p0, p2 - p0)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        assert np.abs(np.einsum("ij,ij->i", pts - p0, nrm)).max() < 1e-12
    _, _, _, ok = SR.sample_surface(np.zeros((3, 3)), np.array([[0, 1, 2]]), 16, seed=0)
    assert not ok


def test_philox_twin():
    # Random123's known-answer vectors for Philox-4x32-10
    kat = [(([0, 0, 0, 0], 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           (([0xffffffff] * 4, 0xffffffffffffffff), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           (([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0x299f31d0 << 32) | 0xa4093822),
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for (c, k), want in kat:
        assert [int(w) for w in philox4x32_10(c, k)] == want
    r1, r2 = MS.surface_uniforms(7, 3, 100000)
    assert r1.min() >= 0 and r1.max() < 1 and abs(r1.mean() - 0.5) < 0.01 and abs(r2.mean() - 0.5) < 0.01
    assert not np.array_equal(r1, MS.surface_uniforms(7, 4, 100000)[0])         # the mesh index is part of the counter
    idx = MS.stats_pairs(7, 3, 100000, 2048)
    assert idx.min() == 0 and idx.max() == 2047 and idx.dtype == np.int64
    assert MS.u53(0xffffffff, 0xffffffff) == 1 - 2.0 ** -53 and MS.u53(0, 0) == 0


def test_category_files_equal_the_transcribed_configs():
    base = config.parse_flat_yaml(open(os.path.join(GOLDEN_CFG, "config.yaml")).read())
    for k, v in config.YAML_DEFAULTS.items():
        assert base[k] == v and type(base[k]) is type(v), k
    files = sorted(glob.glob(os.path.join(GOLDEN_CFG, "category", "*.yaml")))
    assert len(files) == 12
    for p in files:
        cfg = config.load_category_yaml(p)
        ref = CATEGORIES[cfg.category]
        for fld in dataclasses.fields(config.CategoryConfig):
            assert getattr(cfg, fld.name) == getattr(ref, fld.name), (p, fld.name)
        assert isinstance(cfg.res, float)
        assert config.load_category_yaml(p, defaults=os.path.join(GOLDEN_CFG, "config.yaml")) == cfg


def test_yaml_round_trip_and_reader_rules(tmp_path):
    cfg = config.CategoryConfig("roll", 4e-3, [0.1234567890123, 0.2], [1 / 3, 0.05, 2e-5], True, up_sym=False, z_right=True,
                                scale_range=[0.2, 0.4], right_sym=True, npoint_max=8000, knn=40)
    p = str(tmp_path / "roll.yaml")
    config.save_category_yaml(cfg, p)
    assert open(p).readline().strip() == "# @package _global_"
    assert config.load_category_yaml(p) == cfg
    cfg2 = dataclasses.replace(cfg, scale_range=None)
    config.save_category_yaml(cfg2, p)
    assert config.load_category_yaml(p) == cfg2
    d = config.parse_flat_yaml("# @package _global_\nres: 4e-3  # a comment\nopt:\n  lr: 1e-3\nhydra:\n  run:\n    dir: x\n"
                               "defaults:\n  - _self_\nvote_range: [1e-1, 2]\nflag: True\nname: mug\n")
    assert d == {"res": 0.004, "vote_range": [0.1, 2], "flag": True, "name": "mug"}
    bad = tmp_path / "bad.yaml"
    bad.write_text("category: x\nvote_range: [0.1, 0.1]\n")
    with pytest.raises(ValueError):
        config.load_category_yaml(str(bad))


def test_right_sym_targets_match_the_reference(golden):
    g = golden("stats.npz")
    pc, nrm = torch.from_numpy(g["pc"].astype(np.float32)), torch.from_numpy(g["nrm"].astype(np.float32))
    for tag in TAGS:
        up_sym, right_sym, z_right = (bool(v) for v in g[f"{tag}.flags"])
        cfg = dataclasses.replace(CATEGORIES["bottle"], up_sym=up_sym, right_sym=right_sym, z_right=z_right, regress_right=True)
        idx = torch.from_numpy(g[f"{tag}.point_idxs"])
        tr, rot, aux, _ = training.targets(pc, nrm, idx, np.zeros(3), np.eye(3), np.array([0.05, 0.15, 0.05]), cfg)
        np.testing.assert_array_equal(aux.numpy(), g[f"{tag}.aux"])
        np.testing.assert_allclose(tr.numpy(), g[f"{tag}.tr_soft"], atol=2e-4)          # test_oracle_golden's tolerances
        np.testing.assert_allclose(rot.numpy(), g[f"{tag}.rot_soft"], atol=2e-4)


def test_derive_config():
    stats = dict(vote_range=[np.float32(0.25), np.float32(0.2)], scale_mean=np.array([0.1, 0.3, 0.2]), scale_range=[0.5, 0.7])
    cfg = MS.derive_config("roll", stats, 5e-3, [0.2, 0.4], right_sym=True, regress_right=True)
    assert cfg.category == "roll" and cfg.right_sym and cfg.regress_right and not cfg.up_sym and cfg.scale_range == [0.2, 0.4]
    np.testing.assert_allclose(cfg.vote_range, [0.1, 0.08], rtol=1e-7)
    np.testing.assert_allclose(cfg.scale_mean, [0.06, 0.09, 0.03], rtol=1e-12)
    with pytest.raises(ValueError):
        MS.derive_config("roll", stats, 5e-3, [0.4, 0.2])
