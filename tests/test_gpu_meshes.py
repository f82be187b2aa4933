"""Training views on the MI355X: csrc/raster.hip against its numpy restatement (tests/mesh_ref.py) bit for bit, the culling
invariants, a 2-million-triangle mesh against an analytic ray cast, the capacity error, the compaction, MeshViewSampler's samples
against their restatement, and train_on_meshes -> training.infer recovering the pose of held-out rendered views."""
import numpy as np
import pytest
import torch

import mesh_ref as R
from cppf_amd import _lib, training
from cppf_amd import meshes as M
from cppf_amd.config import CATEGORIES

pytestmark = pytest.mark.gpu


def _model(t, rot=np.eye(3)):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, t
    return m


def _rot(a, b):
    return M.roty(a)[:3, :3] @ M.rotx(b)[:3, :3]


def _cases():
    sph = R.uv_sphere(0.3, 16, 32)
    bot = R.necked_cylinder(0.15, 0.45, n_lon=32)
    bx = R.box(0.3, 0.2, 0.15)[:2]
    strip = (np.array([[-1.0, -0.3, 1.0], [1.0, -0.3, 1.0], [1.0, -0.3, -5.0], [-1.0, -0.3, -5.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    # zero-area faces (a repeated vertex, three collinear vertices) next to real ones
    v0, f0 = R.box(0.2, 0.2, 0.2)[:2]
    v_deg = np.vstack([v0, [[0.0, 0.0, 0.3], [0.1, 0.1, 0.3], [0.2, 0.2, 0.3]]])
    f_deg = np.vstack([f0, [[0, 0, 1], [8, 9, 10], [3, 3, 3]]]).astype(np.int32)
    # a mesh half of whose triangles lie off screen (left, right, behind the camera)
    offs = [np.array([0.0, 0, 0]), np.array([-40.0, 0, 0]), np.array([40.0, 0, 0]), np.array([0.0, 0, 4.0])]
    vo = np.vstack([sph[0] + o for o in offs])
    fo = np.vstack([sph[1] + k * sph[0].shape[0] for k in range(4)]).astype(np.int32)
    return [
        ("sphere", *sph, _model([0.05, -0.02, -1.2], _rot(0.3, 0.4)), True),
        ("sphere_nocull", *sph, _model([0.05, -0.02, -1.2], _rot(0.3, 0.4)), False),
        ("bottle", *bot, _model([-0.1, 0.05, -1.6], _rot(1.1, 0.7)), True),
        ("bottle_inside", *bot, _model([0.0, 0.0, -0.1], _rot(0.2, 0.1)), False),      # the camera inside: near-plane crossings
        ("box_near", *bx, _model([0.0, 0.0, -0.3], _rot(0.5, 0.3)), True),              # faces cross z = -0.05, fills the frame
        ("strip", *strip, np.eye(4), True),
        ("degenerate", v_deg, f_deg, _model([0.0, 0.0, -1.0], _rot(0.4, 0.2)), False),
        ("offscreen", vo, fo, _model([0.0, 0.0, -1.5]), True),
        ("fullframe", *R.big_triangle(-1.3), np.eye(4), True),
    ]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_render_is_bit_exact_against_the_restatement(dev, case):
    name, v, f, model, cull = case
    d = M.render_depth(v, f, model, cull=cull, device=dev).cpu().numpy()
    ref = R.raster_ref(v, f, model, cull=cull)
    assert (ref > 0).sum() > 100, name
    assert np.array_equal(d.view(np.uint32), ref.view(np.uint32)), (name, int(((d > 0) != (ref > 0)).sum()),
                                                                    float(np.abs(d - ref).max()))
    if name == "fullframe":
        assert (d > 0).all()


def test_culling_invariants(dev):
    v, f = R.necked_cylinder(0.15, 0.45, n_lon=40)
    for k, model in enumerate([_model([0.0, 0.0, -1.3], _rot(0.6, 0.5)), _model([0.1, -0.1, -0.9], _rot(2.0, -0.4))]):
        on = M.render_depth(v, f, model, cull=True, device=dev).cpu().numpy()
        off = M.render_depth(v, f, model, cull=False, device=dev).cpu().numpy()
        assert np.array_equal(on, off), k                               # a closed mesh: the front faces hide every back face
        far = M.render_depth(v, R.flipped(f), model, cull=True, device=dev).cpu().numpy()
        assert np.array_equal(far > 0, on > 0), k                       # the far side covers the same silhouette...
        assert np.all(far[on > 0] >= on[on > 0]) and np.mean(far[on > 0] > on[on > 0]) > 0.9, k   # ...behind the near side


def _sphere_depth(model, r, W=M.WIDTH, H=M.HEIGHT, fx=M.FX, fy=M.FY):
    """analytic ray cast of the sphere |p - c| = r (c = the model's translation) through every pixel centre"""
    c = model[:3, 3]
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    dx = (2 * cc / W - 1) / (2 * fx / W)
    dy = (2 * (H - rr) / H - 1) / (2 * fy / H)
    dirs = np.stack([dx, dy, -np.ones_like(dx)], -1)
    a = (dirs * dirs).sum(-1)
    b = -2 * (dirs @ c)
    disc = b * b - 4 * a * (c @ c - r * r)
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0)
    nrm = (t[..., None] * dirs - c) / r
    cos_inc = np.abs((nrm * dirs).sum(-1)) / np.sqrt(a)                 # |cos| of the angle between the ray and the surface normal
    return t, cos_inc


def test_two_million_triangles_and_the_capacity_error(dev):
    v, f = R.uv_sphere(0.4, 1000, 1000)
    assert f.shape[0] >= 1_990_000
    model = _model([0.02, -0.01, -1.5])
    d = M.render_depth(v, f, model, device=dev).cpu().numpy()
    ref, cos_inc = _sphere_depth(model, 0.4)
    both = (d > 0) & (ref > 0)
    assert both.sum() > 40000
    rel = np.abs(d - ref) / np.maximum(ref, 1e-9)
    # the facets deviate from the sphere by their sag (~2e-6 m here), which a grazing ray sees magnified by 1 / cos
    assert np.max(rel[both & (cos_inc > 0.2)]) < 2e-5 and np.max(rel[both]) < 1e-3
    mis = (d > 0) != (ref > 0)
    assert mis.sum() < 0.01 * both.sum()                                # only along the silhouette (tessellation)
    with pytest.raises(_lib.CppfError, match=r"\(-5\)"):                 # CPPF_ECAPACITY, not a partial image
        M.render_depth(v, f, model, device=dev, max_bin_entries=1000)


def test_compaction_order_and_values(dev):
    v, f = R.necked_cylinder(0.15, 0.45, n_lon=32)
    d = M.render_depth(v, f, _model([0.03, 0.02, -1.1], _rot(0.8, 0.6)), device=dev)
    pts, count = M.depth_points(d)
    n = int(count.item())
    ref = R.depth_points_ref(d.cpu().numpy())
    assert n == ref.shape[0] > 1000
    assert np.array_equal(pts[:n].cpu().numpy(), ref)


def _bottle_files(tmp_path, n=4, seed=0):
    rng = np.random.default_rng(seed)
    paths = []
    for k in range(n):
        r, h = rng.uniform(0.11, 0.17), rng.uniform(0.38, 0.48)
        v, f = R.necked_cylinder(r, h, neck=rng.uniform(0.35, 0.55), shoulder=rng.uniform(0.2, 0.5), n_lon=40)
        v = v / np.linalg.norm(v.max(0) - v.min(0))                    # ShapeNet's model_normalized: unit bbox diagonal
        p = tmp_path / f"bottle_{k}" / "models" / "model_normalized.obj"
        p.parent.mkdir(parents=True)
        p.write_text(R.to_obj(v, f))
        paths.append(str(p))
    return paths


def test_samples(dev, tmp_path):
    paths = _bottle_files(tmp_path)
    tiny = tmp_path / "tiny.obj"
    v, f = R.necked_cylinder(0.002, 0.006, n_lon=12)
    tiny.write_text(R.to_obj(v, f))
    paths = [str(tiny)] + paths
    cfg = CATEGORIES["bottle"]
    s1 = M.MeshViewSampler(paths, "bottle", dev, seed=5, n_pairs=5000)
    s2 = M.MeshViewSampler(paths, "bottle", dev, seed=5, n_pairs=5000)
    for k in range(3):
        a = s1.sample(mesh_index=0 if k == 0 else None)
        b = s2.sample(mesh_index=0 if k == 0 else None)
        if k == 0:                                                     # the tiny mesh renders a few pixels: redrawn
            assert a["skipped"] and a["skipped"][0]["mesh"] == 0 and a["skipped"][0]["n_points"] < 100 and a["mesh"] != 0
        for key in ("pc", "normals", "point_idxs", "targets_tr", "targets_rot", "targets_rot_aux", "targets_scale"):
            assert torch.equal(a[key], b[key]), key                    # the same seed: the same sample bit for bit
        n = a["pc"].shape[0]
        assert 100 <= n <= cfg.npoint_max
        # the restatement given the draws (and the device's jitter draws, replayed from the generator state)
        vv, ff = M.load_obj(a["path"])
        g = torch.Generator(device=dev)
        g.set_state(a["jitter_state"])
        n_px = int((R.raster_ref(vv, ff, a["model"]) > 0).sum())
        jit = torch.randn((n_px, 3), generator=g, device=dev, dtype=torch.float64).cpu().numpy()
        pc_ref, half = R.sample_ref(vv, ff, a, cfg, True, jit)
        assert np.array_equal(a["pc"].cpu().numpy(), pc_ref)
        assert np.array_equal(a["half_extents"], half)
        # every point on the surface of the posed mesh, within the jitter and the half-pixel footprint of the dataset's backproject
        bmin, bmax = M.mesh_bounds(vv, ff)
        obj = (a["pc"].cpu().numpy().astype(np.float64) @ M.FLIP2NOCS) / a["scale"] + (bmin + bmax) / 2   # mesh frame
        rad = np.hypot(obj[:, 0], obj[:, 2])
        prof = _profile_distance(vv, rad, obj[:, 1])
        tol = (np.sqrt(3) * cfg.res / 2 + 0.75 * (-a["t"][2] + 0.3) / M.FX) / a["scale"] + 2e-3
        assert np.max(prof) < tol, (np.max(prof), tol)
        # the targets: training.targets on the same cloud, and the scale target in closed form
        tr, rot, aux, sc = training.targets(a["pc"], a["normals"], a["point_idxs"], np.zeros(3), np.eye(3), a["half_extents"], cfg)
        assert torch.equal(tr, a["targets_tr"]) and torch.equal(rot, a["targets_rot"]) and torch.equal(aux, a["targets_rot_aux"])
        closed = np.log(half) - np.log(cfg.scale_mean)
        assert np.array_equal(a["targets_scale"].cpu().numpy(), closed.astype(np.float32))


def _profile_distance(v, rad, y):
    """distance in the (radius, y) half plane from each point to the lathe profile of a necked_cylinder mesh"""
    ys = np.unique(np.round(v[:, 1], 12))
    rs = {yy: np.unique(np.round(np.hypot(v[np.isclose(v[:, 1], yy), 0], v[np.isclose(v[:, 1], yy), 2]), 12)) for yy in ys}
    # the profile: (0, -h) (R, -h) (R, ys) (r2, ys) (r2, h) (0, h)
    h0, h1 = ys[0], ys[-1]
    Rb, r2 = rs[h0].max(), rs[h1].max()
    ysh = ys[1]
    pts = np.array([[0, h0], [Rb, h0], [Rb, ysh], [r2, ysh], [r2, h1], [0, h1]], np.float64)
    P = np.stack([rad, y], -1)
    best = np.full(P.shape[0], np.inf)
    for a, b in zip(pts[:-1], pts[1:]):
        ab = b - a
        t = np.clip(((P - a) @ ab) / (ab @ ab), 0, 1)
        best = np.minimum(best, np.linalg.norm(P - a - t[:, None] * ab, axis=1))
    return best


def test_train_on_meshes_recovers_held_out_poses(dev, tmp_path):
    paths = _bottle_files(tmp_path, n=5, seed=1)
    penc, enc, losses = training.train_on_meshes("bottle", paths, dev, steps=3000, n_pairs=200000, seed=0)   # :230's 200 000 pairs
    assert losses[-1] < 0.7 * losses[0], losses
    held = M.MeshViewSampler(paths, "bottle", dev, seed=4242)           # views (poses, scales) no training step drew
    errs = []
    for j in range(12):
        ob = held.sample(canonical=False)
        pose = training.infer(penc, enc, ob, dev, seed=j)
        errs.append(training.pose_errors(pose, ob))
    med = {k: float(np.median([e[k] for e in errs])) for k in ("t_cells", "up_deg_mod_sign", "scale_rel")}
    print("held-out medians", med, [{k: round(e[k], 3) for k in med} for e in errs])
    assert med["t_cells"] <= 4.0 and med["up_deg_mod_sign"] <= 10.0 and med["scale_rel"] <= 0.2, errs
