"""Mesh statistics on the MI355X: csrc/mesh_stats.hip against its numpy restatement (tests/mesh_stats_ref.py) bit for bit, Open3D's
count rule, the area weighting, zero-area meshes in a batch, batch / seed invariance, analytic bounds on a sphere, right_sym
targets on the device, and a category that is not in CATEGORIES taken from meshes to a config to a trained network that recovers
held-out poses."""
import dataclasses

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_stats_ref as SR
from cppf_amd import config, training
from cppf_amd import mesh_stats as MS
from cppf_amd import meshes as M
from cppf_amd.config import CATEGORIES

pytestmark = pytest.mark.gpu


def _shapes():
    v0, f0 = R.box(0.2, 0.2, 0.2)[:2]
    v_deg = np.vstack([v0, [[0.0, 0.0, 0.3], [0.1, 0.1, 0.3], [0.2, 0.2, 0.3]]])
    f_deg = np.vstack([f0, [[0, 0, 1], [8, 9, 10], [3, 3, 3]]]).astype(np.int32)
    return [R.box()[:2], R.uv_sphere(0.5, 16, 32), R.necked_cylinder(), (v_deg, f_deg), R.uv_sphere(0.3, 40, 80)]


def _check_sample(pts, fid, v, f, n, seed, mesh):
    ref, t, _, ok = SR.sample_surface(v, f, n, seed, mesh)
    assert ok
    assert np.array_equal(pts, ref), (mesh, np.abs(pts - ref).max())
    assert np.array_equal(fid, t), mesh


def test_sampling_is_bit_exact_against_the_restatement(dev):
    shapes = _shapes()
    for n, seed in ((2048, 0), (5000, 77)):
        pts, fid, status = MS.sample_surface_batch(shapes, n, seed=seed, device=dev)
        assert status.cpu().tolist() == [0] * len(shapes)
        pts, fid = pts.cpu().numpy(), fid.cpu().numpy()
        for m, (v, f) in enumerate(shapes):
            _check_sample(pts[m], fid[m], v, f, n, seed, m)


def test_two_million_triangles(dev):
    v, f = R.uv_sphere(0.5, 1000, 1000)
    assert f.shape[0] > 1_990_000
    pts, fid = MS.sample_surface(v, f, 2048, seed=9, device=dev, return_faces=True)
    _check_sample(pts.cpu().numpy(), fid.cpu().numpy(), v, f, 2048, 9, 0)
    st, status = MS.vote_stats_batch(pts[None], 100000, seed=9)
    assert int(status.item()) == 0
    assert np.array_equal(st[0].cpu().numpy(), SR.vote_stats(pts.cpu().numpy(), 100000, 9, 0))


def test_counts_and_area_weighting(dev):
    v, f = R.necked_cylinder(0.15, 0.45, n_lon=24)
    n = 200000
    pts, fid = MS.sample_surface(v, f, n, seed=1, device=dev, return_faces=True)
    cnt = np.bincount(fid.cpu().numpy(), minlength=f.shape[0])
    a = SR.areas(v, f)
    C = SR.blocked_cumsum(a / SR.blocked_total(a))
    assert np.array_equal(cnt, SR.open3d_counts(C, n)) and cnt.sum() == n
    expected = n * a / a.sum()
    chi2 = float(((cnt - expected) ** 2 / expected).sum())
    assert chi2 < 0.5 * f.shape[0], chi2               # Open3D's rule: |count - expected| <= 1 per face, far inside a random draw's
    # within a face the points are uniform: the barycentric weight of v0, 1 - sqrt(r1), has mean 1/3
    p, t = pts.cpu().numpy(), fid.cpu().numpy()
    big = np.argmax(a)
    sel = p[t == big]
    tri = v[f[big]]
    w = np.linalg.lstsq(np.stack([tri[1] - tri[0], tri[2] - tri[0]], 1), (sel - tri[0]).T, rcond=None)[0]
    assert sel.shape[0] > 1000 and abs(float((1 - w.sum(0)).mean()) - 1 / 3) < 0.03


def test_zero_area_mesh_in_a_batch(dev, tmp_path):
    good0, good1 = R.box()[:2], R.uv_sphere(0.5, 16, 32)
    flat = (np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 0, 0]]), np.array([[0, 1, 2], [0, 3, 1]], np.int32))
    pts, fid, status = MS.sample_surface_batch([good0, flat, good1], 2048, seed=4, device=dev)
    assert status.cpu().tolist() == [0, 1, 0]
    assert torch.isnan(pts[1]).all() and (fid[1] == -1).all()
    p = pts.cpu().numpy()
    _check_sample(p[0], fid[0].cpu().numpy(), *good0, 2048, 4, 0)
    _check_sample(p[2], fid[2].cpu().numpy(), *good1, 2048, 4, 2)
    st, sst = MS.vote_stats_batch(pts, 1000, seed=4)
    assert sst.cpu().tolist() == [0, 1, 0] and torch.isnan(st[1]).all() and not torch.isnan(st[[0, 2]]).any()
    paths = []
    for k, (v, f) in enumerate([good0, flat, good1]):
        paths.append(str(tmp_path / f"m{k}.obj"))
        open(paths[-1], "w").write(R.to_obj(v, f))
    with pytest.raises(MS.MeshStatsError, match="m1.obj"):
        MS.category_stats(paths, device=dev)
    with pytest.raises(MS.MeshStatsError):
        MS.sample_surface(*flat, 16, device=dev)


def test_vote_stats_bit_exact_batch_and_seed_invariance(dev):
    shapes = _shapes()
    pts, _, _ = MS.sample_surface_batch(shapes, 2048, seed=3, device=dev)
    st, status = MS.vote_stats_batch(pts, 100000, seed=3)
    st = st.cpu().numpy()
    assert status.cpu().tolist() == [0] * len(shapes)
    p = pts.cpu().numpy()
    for m in range(len(shapes)):
        assert np.array_equal(st[m], SR.vote_stats(p[m], 100000, 3, m)), m
        # M single calls with first_mesh = m give the batch's bits
        pm, _, _ = MS.sample_surface_batch([shapes[m]], 2048, seed=3, first_mesh=m, device=dev)
        assert torch.equal(pm[0], pts[m])
        sm, _ = MS.vote_stats_batch(pm, 100000, seed=3, first_mesh=m)
        assert np.array_equal(sm[0].cpu().numpy(), st[m])
    again = MS.vote_stats_batch(MS.sample_surface_batch(shapes, 2048, seed=3, device=dev)[0], 100000, seed=3)[0].cpu().numpy()
    assert np.array_equal(again, st)
    other = MS.vote_stats_batch(pts, 100000, seed=4)[0].cpu().numpy()
    assert np.array_equal(other[:, [0, 3, 4, 5]], st[:, [0, 3, 4, 5]]) and not np.array_equal(other, st)
    # category_stats: chunked or not, the same rows, and gen_stats.py's aggregation of them
    a = MS.category_stats(shapes, seed=3, device=dev)
    b = MS.category_stats(shapes, seed=3, device=dev, max_faces_per_call=3000)
    assert np.array_equal(a["rows"], st) and np.array_equal(b["rows"], st)
    agg = SR.aggregate(st)
    assert a["scale_range"] == agg["scale_range"] and a["vote_range"] == agg["vote_range"]
    assert np.array_equal(a["scale_mean"], agg["scale_mean"])


def test_sphere_bounds(dev):
    r = 0.37
    v, f = R.uv_sphere(r, 64, 128)
    pts = MS.sample_surface(v, f, 2048, seed=0, device=dev)
    st, _ = MS.vote_stats_batch(pts[None], 100000, seed=0)
    diag, mp, md = (float(x) for x in st[0, :3].cpu().numpy())
    full = 2 * np.sqrt(3) * r
    assert 0.99 * full <= diag <= full, (diag, full)
    c = np.abs(SR.centre(pts.cpu().numpy())).max()                # the bbox centre of 2048 samples is not exactly 0
    for x in (mp, md):
        assert 0.99 * r <= x <= np.float32(r + np.sqrt(3) * c), (x, r, c)
    # self-pairs (kept, as np.random.randint keeps them): proj 0 and dist2o = |a| exactly
    p = pts.cpu().numpy() - SR.centre(pts.cpu().numpy())
    idx = MS.stats_pairs(0, 0, 100000, 2048)
    self_ = idx[:, 0] == idx[:, 1]
    assert self_.sum() > 10
    proj, dist = SR.pair_targets(p[idx[self_, 0]], p[idx[self_, 1]])
    a = p[idx[self_, 0]]
    assert (proj == 0).all() and np.array_equal(dist, np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]))


def test_right_sym_targets_on_the_device(dev, golden):
    g = golden("stats.npz")
    pc = torch.from_numpy(g["pc"].astype(np.float32)).to(dev)
    nrm = torch.from_numpy(g["nrm"].astype(np.float32)).to(dev)
    for tag in ("plain", "rightsym", "rightsym_zright_upsym"):
        up_sym, right_sym, z_right = (bool(x) for x in g[f"{tag}.flags"])
        cfg = dataclasses.replace(CATEGORIES["bottle"], up_sym=up_sym, right_sym=right_sym, z_right=z_right, regress_right=True)
        idx = torch.from_numpy(g[f"{tag}.point_idxs"]).to(dev)
        tr, rot, aux, _ = training.targets(pc, nrm, idx, np.zeros(3), np.eye(3), np.array([0.05, 0.15, 0.05]), cfg)
        np.testing.assert_array_equal(aux.cpu().numpy(), g[f"{tag}.aux"])
        np.testing.assert_allclose(tr.cpu().numpy(), g[f"{tag}.tr_soft"], atol=2e-4)
        np.testing.assert_allclose(rot.cpu().numpy(), g[f"{tag}.rot_soft"], atol=2e-4)


def _roll_files(tmp_path, n, seed):
    """a family of lathe shapes (bodies with a neck of varied proportions), unit bbox diagonal as ShapeNet's model_normalized"""
    rng = np.random.default_rng(seed)
    paths = []
    for k in range(n):
        v, f = R.necked_cylinder(rng.uniform(0.12, 0.2), rng.uniform(0.25, 0.4), neck=rng.uniform(0.5, 0.8),
                                 shoulder=rng.uniform(0.1, 0.5), n_lon=40)
        v = v / np.linalg.norm(v.max(0) - v.min(0))
        p = tmp_path / f"roll_{k}" / "models" / "model_normalized.obj"
        p.parent.mkdir(parents=True)
        p.write_text(R.to_obj(v, f))
        paths.append(str(p))
    return paths


def test_new_category_from_meshes_to_a_trained_network(dev, tmp_path):
    name = "roll"
    assert name not in CATEGORIES
    paths = _roll_files(tmp_path, 5, 2)
    stats = MS.category_stats(paths, device=dev)
    cfg = MS.derive_config(name, stats, 5e-3, [0.2, 0.4], up_sym=True)
    yml = str(tmp_path / "roll.yaml")
    config.save_category_yaml(cfg, yml)
    cfg = config.load_category_yaml(yml)
    assert cfg == MS.derive_config(name, stats, 5e-3, [0.2, 0.4], up_sym=True)
    sampler = M.MeshViewSampler(paths, name, dev, seed=8, n_pairs=20000, cfg=cfg)
    assert not sampler.is_nocs                                         # a name outside NOCS_CATEGORIES: the SUN RGB-D views
    clipped, total, scale_t = 0, 0, []
    for _ in range(50):
        s = sampler.sample()
        pc, idx = s["pc"], s["point_idxs"]
        a, b = pc[idx[:, 0]], pc[idx[:, 1]]
        d = a - b
        u = d / (d.norm(dim=-1, keepdim=True) + 1e-7)
        proj = (a * u).sum(-1)
        dist = (a - proj[:, None] * u).norm(dim=-1)
        clipped += int(((proj.abs() > cfg.vote_range[0]) | (dist > cfg.vote_range[1])).sum())
        total += idx.shape[0]
        scale_t.append(s["targets_scale"].cpu().numpy())
    frac, mean_scale = clipped / total, np.mean(scale_t, 0)
    print("clipped", frac, "mean scale target", mean_scale, "cfg", cfg)
    assert frac <= 0.005 and np.all(np.abs(mean_scale) <= 0.1), (frac, mean_scale)
    penc, enc, losses = training.train_on_meshes(name, paths, dev, steps=3000, n_pairs=200000, seed=0, cfg=cfg)
    assert losses[-1] < 0.7 * losses[0], losses
    held = M.MeshViewSampler(paths, name, dev, seed=4242, cfg=cfg)
    errs = []
    for j in range(12):
        ob = held.sample(canonical=False)
        pose = training.infer(penc, enc, ob, dev, seed=j)
        errs.append(training.pose_errors(pose, ob))
    med = {k: float(np.median([e[k] for e in errs])) for k in ("t_cells", "up_deg_mod_sign", "scale_rel")}
    print("held-out medians", med)
    assert med["t_cells"] <= 4.0 and med["up_deg_mod_sign"] <= 10.0 and med["scale_rel"] <= 0.2, errs
