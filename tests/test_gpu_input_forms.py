"""The input-form contract of the Python layer ("Input forms"): an entry point that takes the caller's data gives,
for ANY form of it -- a column slice of a wider array, strided rows, transposed storage, an offset into an allocation, a member
of a batch, another floating type, another index width, a zero-stride expand, a leaf that requires grad -- bit for bit the
result of x.to(dtype).contiguous(); the drop-in kernels of models/voting.py, which write in place, refuse instead; a tensor on
the wrong device is refused before anything is launched.

One small workload serves every test: a 257-point mug (odd: a whole-row offset into an f32[*,3] buffer is 4-byte but not 16-byte
aligned), 1 028 pairs, random-init encoders, 480 sphere bins.  Equality is exact: after the conversion both sides run the same
kernels on the same bits.  The canonical run itself is tied to the oracle once (test_canonical_pose_equals_oracle).

Forms that do not apply are left out of the tables: f64 / f16 / requires-grad on index and mask arguments, the other index width
on float arguments, transposed storage on arguments that are not 2-D, the zero-stride expand on anything but the bin uniforms
(every other argument would lose its content), and for the drop-in refusals the forms that ARE canonical for them (a contiguous
row offset, a batch member, a leaf)."""
import types

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
from cppf_amd import _lib, _torch_util as tu
from cppf_amd import inference, mesh_stats, meshes, zero_shot
from cppf_amd.evaluation import pose_metrics_device
from cppf_amd.inference import estimate_center, estimate_pose, grid_shape
from cppf_amd.models import model as model_mod, voting
from cppf_amd.models.model import PPFEncoder, PointEncoder
from cppf_amd.utils.util import backproject, estimate_normals, fibonacci_sphere, sparse_quantize

pytestmark = pytest.mark.gpu

N, K, SEED = 257, 4, 0
JUNK = 7                # what surrounds the data in the wider / longer buffers (a valid point index too)


# ------------------------------------------------------------------------------------------------ the forms
# form(x) -> (canonical tensor the result is compared with, the same values in another form)
def col_slice(x):
    c = x.shape[-1]
    wide = torch.full(tuple(x.shape[:-1]) + (3 * c,), JUNK, dtype=x.dtype, device=x.device)
    wide[..., c:2 * c] = x
    return x, wide[..., c:2 * c]


def row_stride(x):
    big = torch.full((2 * x.shape[0],) + tuple(x.shape[1:]), JUNK, dtype=x.dtype, device=x.device)
    big[::2] = x
    return x, big[::2]


def transposed_storage(x):
    return x, x.t().contiguous().t()


def row_offset(x):
    return x, torch.cat([torch.full_like(x[:1], JUNK), x])[1:]


def batch_member(x):
    return x, torch.stack([torch.full_like(x, JUNK), x])[1]


def f64(x):
    return x, x.double()


def f16(x):
    return x.half().float(), x.half()            # both sides see the values rounded through f16


def f32_of_f64(x):
    return x.float().double(), x.float()


def leaf(x):
    return x, x.clone().requires_grad_(True)


def other_int(x):
    return x, x.to(torch.int32 if x.dtype == torch.int64 else torch.int64)


def as_bool(x):
    return x, x.bool()


def expanded(x):
    row = x[:1].expand_as(x)
    return row.contiguous(), row


FLOAT_2D = [col_slice, row_stride, transposed_storage, row_offset, batch_member, f64, f16, leaf]
FLOAT_ND = [col_slice, row_stride, row_offset, batch_member, f64, f16, leaf]
F64_2D = [col_slice, row_stride, transposed_storage, row_offset, batch_member, f32_of_f64, f16, leaf]
F64_ND = [col_slice, row_stride, row_offset, batch_member, f32_of_f64, f16, leaf]
INDEX_2D = [col_slice, row_stride, transposed_storage, row_offset, batch_member, other_int]
INDEX_1D = [col_slice, row_stride, row_offset, batch_member, other_int]
UNIFORMS = FLOAT_2D + [expanded]


def _non_canonical(x, y):
    """the formed tensor really differs in form from the canonical one"""
    return (not y.is_contiguous()) or y.dtype != x.dtype or y.requires_grad or y.data_ptr() % 16 != 0 or y.storage_offset() != 0


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _same(want, got):
    assert want.keys() == got.keys()
    for k in want:
        a, b = _np(want[k]), _np(got[k])
        # (exact, position by position; a NaN equals the NaN in the same place)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k


# ------------------------------------------------------------------------------------------------ the workload
@pytest.fixture(scope="module")
def work(dev):
    ob = syn.make_object("mug", N, SEED)
    cfg = ob["cfg"]
    idx = syn.make_pairs(N, K, SEED)
    u_tr, u_rot = syn.make_uniforms(idx.shape[0], SEED)
    torch.manual_seed(SEED)
    enc = PPFEncoder(cfg.ppffcs, cfg.out_dim).eval()
    sd = {k: v.detach().numpy().copy() for k, v in enc.state_dict().items()}
    penc = PointEncoder(k=16, spfcs=[32, 64, 32, 32], num_layers=1, out_dim=32).eval()
    enc9 = PPFEncoder(cfg.ppffcs, 9).eval()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(SEED)
    t = dict(pc=d(ob["pc"]), pc_normal=d(ob["normals"]), feat=d(ob["feat"]), point_idxs=d(idx), u_tr=d(u_tr), u_rot=d(u_rot),
             probs=d(rng.uniform(0.5, 1.5, N).astype(np.float32)))
    return types.SimpleNamespace(ob=ob, cfg=cfg, idx=idx, u_tr=u_tr, u_rot=u_rot, enc=enc.to(dev), sd=sd, penc=penc.to(dev),
                                 enc9=enc9.to(dev), t=t, sph=np.array(fibonacci_sphere(480)), dev=dev, d=d,
                                 grid0=grid_shape(ob["pc"], cfg.res))


def run_pose(w, **a):
    a = dict(w.t, **a)
    with torch.no_grad():
        r = estimate_pose(w.enc, a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], a["u_tr"], a["u_rot"], w.cfg, w.sph)
    counts = r["ws"].counts.cpu().numpy()
    out = {k: r[k] for k in ("argmax", "peak", "n_surv", "T", "up", "right", "scale", "losses", "dims", "outputs", "heads")}
    out.update(counts_up=counts[0], counts_right=counts[1])
    return out


def run_center(w, _grid=None, **a):
    a = dict(w.t, **a)
    if _grid is not None:
        corners, dims = _grid
    elif a["pc"] is w.t["pc"]:
        corners, dims = w.grid0                  # (the canonical cloud's grid, laid once: a refusal test must not call the library)
    else:
        corners, dims = grid_shape(a["pc"].detach().float().cpu().numpy(), w.cfg.res)
    corner = torch.from_numpy(corners[0].copy()).to(w.dev)
    with torch.no_grad():
        oi, ov, outputs, heads, grid = estimate_center(w.enc, a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], a["u_tr"], w.cfg, corner,
                                                       dims, u_rot=a["u_rot"], probs=a["probs"])
    return dict(out_idx=oi, out_val=ov, outputs=outputs, heads=heads, grid=grid)


def run_with_idx(w, **a):
    a = dict(w.t, **a)
    with torch.no_grad():
        return dict(logits=w.enc.forward_with_idx(a["pc"], a["pc_normal"], a["feat"], a["point_idxs"]))


def run_forward(w, **a):
    a = dict(w.t, **a)
    with torch.no_grad():
        return dict(logits=w.enc(a["pc"][None], a["pc_normal"][None], a["feat"][None], idxs=a["point_idxs"]))


def run_decode(w, **a):
    a = dict(w.t, **a)
    with torch.no_grad():
        o, h = w.enc.forward_decode(a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], a["u_tr"], w.cfg.vote_range, a["u_rot"])
    return dict(outputs=o, heads=h)


def run_point_encoder(w, **a):
    a = dict(w.t, **a)
    with torch.no_grad():
        return dict(feat=w.penc(a["pc"][None], a["pc_normal"][None], None if a.get("dist") is None else a["dist"][None]))


def run_normals(w, **a):
    return dict(normals=estimate_normals(dict(w.t, **a)["pc"], 16))


def run_quantize(w, **a):
    coords, idx = sparse_quantize(dict(w.t, **a)["pc"], return_index=True, quantization_size=4 * w.cfg.res)
    return dict(coords=coords, idx=idx)


def run_distinct(w, **a):
    a = dict(w.t, **a)
    kept = zero_shot.distinct_pairs(a["pc"], a["pc_normal"], a["point_idxs"])
    assert kept.dtype == a["point_idxs"].dtype                   # (the kept pairs come back in the width they came in)
    return dict(kept=kept.long())


def run_scene(w, **a):
    a = dict(w.t, **a)
    r = zero_shot.zero_shot_scene(w.enc9, a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], w.cfg, thresh=1.0, margin=3, max_proposals=4)
    out = dict(preds=r["preds"], grid=r["grid"], loc=r["proposals"][0], val=r["proposals"][1], n=len(r["poses"]))
    for k, p in enumerate(r["poses"]):
        out.update({f"T{k}": p["T"], f"R{k}": p["R"], f"s{k}": p["scale_3d"], f"m{k}": p["point_mask"], f"n{k}": p["n_pairs"]})
    return out


POSE_ARGS = dict(pc=FLOAT_2D, pc_normal=FLOAT_2D, feat=FLOAT_2D, point_idxs=INDEX_2D, u_tr=UNIFORMS, u_rot=UNIFORMS)
ENC_ARGS = dict(pc=FLOAT_2D, pc_normal=FLOAT_2D, feat=FLOAT_2D, point_idxs=INDEX_2D)
ENTRIES = {
    "estimate_pose": (run_pose, POSE_ARGS),
    "estimate_center": (run_center, dict(POSE_ARGS, probs=FLOAT_ND)),
    "forward_with_idx": (run_with_idx, ENC_ARGS),
    "forward": (run_forward, ENC_ARGS),
    "forward_decode": (run_decode, POSE_ARGS),
    "point_encoder": (run_point_encoder, dict(pc=FLOAT_2D, pc_normal=FLOAT_2D, dist=FLOAT_2D)),
    "estimate_normals": (run_normals, dict(pc=FLOAT_2D)),
    "sparse_quantize": (run_quantize, dict(pc=FLOAT_2D)),
    "distinct_pairs": (run_distinct, dict(pc=FLOAT_2D, pc_normal=FLOAT_2D, point_idxs=INDEX_2D)),
    "zero_shot_scene": (run_scene, ENC_ARGS),
}
CASES = [(e, a, f) for e, (_, args) in ENTRIES.items() for a, forms in args.items() for f in forms]


def _tensors(w):
    if "dist" not in w.t:
        w.t["dist"] = torch.cdist(w.t["pc"], w.t["pc"])
    return w.t


@pytest.mark.parametrize("entry,arg,form", CASES, ids=[f"{e}-{a}-{f.__name__}" for e, a, f in CASES])
def test_one_argument_in_another_form(work, entry, arg, form):
    run = ENTRIES[entry][0]
    canonical, formed = form(_tensors(work)[arg])
    assert _non_canonical(canonical, formed) and torch.equal(canonical, formed.to(canonical.dtype))
    _same(run(work, **{arg: canonical}), run(work, **{arg: formed}))


ALL_AT_ONCE = dict(pc=row_stride, pc_normal=col_slice, feat=f64, point_idxs=other_int, u_tr=transposed_storage, u_rot=row_offset,
                   probs=f16, dist=batch_member)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_argument_in_another_form_at_once(work, entry):
    run, args = ENTRIES[entry]
    pairs = {a: ALL_AT_ONCE[a](_tensors(work)[a]) for a in args}
    _same(run(work, **{a: c for a, (c, _) in pairs.items()}), run(work, **{a: f for a, (_, f) in pairs.items()}))


def test_canonical_pose_equals_oracle(work, oracle):
    """the canonical run every comparison above starts from, against the oracle chain (the bounds of
    test_gpu_preproc.py::test_raw_points_to_pose_entirely_on_device); and both sign sums of the mug are non-zero, so a normal read
    in the wrong form has a sign to get wrong"""
    w = work
    r = run_pose(w)
    cfg = w.cfg
    ocfg = dict(res=cfg.res, tr_num_bins=32, rot_num_bins=36, vote_range=cfg.vote_range, scale_mean=cfg.scale_mean,
                regress_right=cfg.regress_right, ppffcs=cfg.ppffcs, out_dim=cfg.out_dim)
    o = oracle.estimate_pose(w.ob["pc"], w.ob["normals"], w.ob["feat"], w.idx, w.sd, ocfg, w.u_tr, w.u_rot, w.sph)
    print("n_surv", r["n_surv"], "argmax", r["argmax"], o["argmax"], "losses", r["losses"])
    assert r["argmax"] == o["argmax"] and r["n_surv"] == int(o["mask"].sum())
    assert np.allclose(r["T"], o["T"], atol=1e-9) and np.allclose(r["up"], o["up"], atol=1e-9)
    assert np.allclose(r["scale"], o["scale"], rtol=1e-5)
    assert cfg.regress_right and r["n_surv"] > 0
    assert np.all(r["losses"][:, :2] != 0)


# ------------------------------------------------------------------------------------------------ the other converting entry points
def test_backproject_forms(work):
    dev = work.dev
    rng = np.random.default_rng(3)
    H, W = 19, 23
    depth = rng.uniform(300, 900, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.2] = 0
    mask = (rng.random((H, W)) < 0.6).astype(np.uint8)
    Kmat = np.array([[591.0, 0, 11.5], [0, 590.0, 9.5], [0, 0, 1]])
    d, m = work.d(depth), work.d(mask)
    run = lambda dd, mm: dict(zip(("pts", "pix"), backproject(dd, Kmat, mm, return_device=True)))
    want = run(d, m)
    assert want["pts"].shape[0] > 50
    for form in FLOAT_2D:
        c, f = form(d)
        _same(run(c, m), run(f, m))
    for form in [col_slice, row_stride, transposed_storage, row_offset, batch_member, as_bool]:
        c, f = form(m)
        assert _non_canonical(c, f)
        _same(want, run(d, f))
    _same(want, run(row_stride(d)[1], col_slice(m)[1]))


def test_segment_instance_forms(work):
    w = work
    a = w.t
    corners, dims = grid_shape(w.ob["pc"], w.cfg.res)
    with torch.no_grad():
        outputs, _ = w.enc.forward_decode(a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], a["u_tr"], w.cfg.vote_range)
    centre = w.ob["pc"].mean(0)
    corner = torch.from_numpy(corners[0].copy()).to(w.dev)
    run = lambda pc, o, idx, cn: zero_shot.segment_instance(pc, o, idx, centre, cn, w.cfg.res, dims, tol=20 * w.cfg.res, min_contrib=1)
    want = run(a["pc"], outputs, a["point_idxs"], corner)
    for form in FLOAT_2D:
        c, f = form(a["pc"])
        _same(run(c, outputs, a["point_idxs"], corner), run(f, outputs, a["point_idxs"], corner))
        c, f = form(outputs)
        _same(run(a["pc"], c, a["point_idxs"], corner), run(a["pc"], f, a["point_idxs"], corner))
    for form in INDEX_2D:
        _same(want, run(a["pc"], outputs, form(a["point_idxs"])[1], corner))
    for form in [row_stride, row_offset, batch_member, f64, leaf]:
        _same(want, run(a["pc"], outputs, a["point_idxs"], form(corner)[1]))


def test_pose_metrics_device_forms(work):
    dev = work.dev
    rng = np.random.default_rng(9)
    def poses(n):
        RT = np.tile(np.eye(4), (n, 1, 1))
        for i in range(n):
            RT[i, :3, :3] = syn.random_rotation(rng)
            RT[i, :3, 3] = rng.uniform(-0.1, 0.1, 3)
        return RT, rng.uniform(0.1, 0.3, (n, 3))
    (pRT, psc), (gRT, gsc) = poses(3), poses(2)
    args = dict(pred_RTs=work.d(pRT), pred_scales=work.d(psc), gt_RTs=work.d(gRT), gt_scales=work.d(gsc),
                gt_up_syms=work.d(np.array([0, 1], np.int32)), pairs=work.d(np.array([[0, 0], [1, 1], [2, 0], [2, 1], [0, 1]], np.int32)),
                sweep=work.d(np.array([0, 1, 0, 1, 1], np.int32)))
    run = lambda **a: dict(zip(("iou", "deg", "cm"), pose_metrics_device(**dict(args, **a))))
    forms = dict(pred_RTs=F64_ND, gt_RTs=F64_ND, pred_scales=F64_2D, gt_scales=F64_2D, gt_up_syms=INDEX_1D, pairs=INDEX_2D, sweep=INDEX_1D)
    for name, fs in forms.items():
        for form in fs:
            c, f = form(args[name])
            _same(run(**{name: c}), run(**{name: f}))


def test_mesh_entry_points_forms(work):
    dev = work.dev
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int32)
    verts, faces, voff, foff = mesh_stats.upload_meshes([(v, f), (v * 2, f)], dev)
    run = lambda vv, ff: dict(zip(("pts", "fid", "status"), mesh_stats.sample_surface_packed(vv, ff, voff, foff, 33, seed=2)))
    want = run(verts, faces)
    for form in F64_2D:
        c, fo = form(verts)
        _same(run(c, faces), run(fo, faces))
    for form in [col_slice, row_stride, transposed_storage, row_offset, batch_member]:       # (faces are int32: another width raises)
        _same(want, run(verts, form(faces)[1]))
    with pytest.raises(TypeError, match="faces"):
        run(verts, faces.long())
    pts = want["pts"]
    stats = lambda p: dict(zip(("stats", "status"), mesh_stats.vote_stats_batch(p, n_pairs=500, seed=1)))
    for form in F64_ND:
        c, fo = form(pts)
        _same(stats(c), stats(fo))
    depth = torch.rand((21, 17), device=dev) * (torch.rand((21, 17), device=dev) > 0.3)
    def dp(x):                                                   # (rows behind `count` are unspecified)
        pts, count = meshes.depth_points(x)
        return dict(pts=pts[:int(count)], count=count)
    assert 50 < int(dp(depth)["count"]) < 21 * 17
    for form in FLOAT_2D:
        c, fo = form(depth)
        _same(dp(c), dp(fo))


def test_batch_runner_put_forms(work):
    """BatchPoseRunner.put takes device tensors in any form; the records of run() equal those of the canonical objects"""
    from cppf_amd.batch import BatchPoseRunner
    w = work
    runner = BatchPoseRunner({"mug": w.enc}, w.dev, n_lanes=1)
    canon_obj = dict(pc=w.t["pc"], normals=w.t["pc_normal"], feat=w.t["feat"], cfg=w.cfg, n_pairs=N * K)
    formed = dict(canon_obj, pc=row_stride(w.t["pc"])[1], normals=col_slice(w.t["pc_normal"])[1], feat=f64(w.t["feat"])[1])
    a, b = runner.put([canon_obj, canon_obj]), runner.put([formed, formed])
    for x, y in zip(a, b):
        assert x["dims"] == y["dims"]
        for k in ("pc", "normals", "feat"):
            assert y[k].is_contiguous() and y[k].dtype == torch.float32 and torch.equal(x[k], y[k])
    ra = runner.run(a, seed=3).cpu().numpy()
    rb = runner.run(b, seed=3).cpu().numpy()
    assert np.array_equal(ra, rb) and np.isfinite(ra[:, :12]).all()


def test_forward_nbrs_forms(work):
    """PointEncoder.forward_nbrs: the cloud, the normals and the caller's neighbour lists (int32 or int64) in every form"""
    w = work
    t = w.t
    nbrs = w.penc.neighbours(t["pc"])
    assert nbrs.dtype == torch.int32 and tuple(nbrs.shape) == (N, 16)

    def run(pc=t["pc"], nrm=t["pc_normal"], nb=nbrs):
        with torch.no_grad():
            return dict(feat=w.penc.forward_nbrs(pc[None], nrm[None], nb[None]))
    want = run()
    _same(want, run_point_encoder(w, dist=None))                      # (the lists the encoder would have chosen itself)
    for form in INDEX_2D:
        c, f = form(nbrs)
        assert _non_canonical(c, f)
        _same(want, run(nb=f))
    for form in FLOAT_2D:
        c, f = form(t["pc"])
        _same(run(pc=c), run(pc=f))
        c, f = form(t["pc_normal"])
        _same(run(nrm=c), run(nrm=f))


def test_forward_decode_sel_forms(work):
    """the second pass on selected pairs (after the first pass on the same arguments, whose per-point table it reuses): every
    float and index argument in every form; sel / n_sel / heads are another kernel's outputs and are checked, not converted"""
    w = work
    P = N * K
    sel = torch.arange(0, P, 3, dtype=torch.int32, device=w.dev)
    n_sel = torch.tensor([sel.numel() - 5], dtype=torch.int32, device=w.dev)

    def run(**a):
        a = dict(w.t, **a)
        with torch.no_grad():
            w.enc.forward_decode(a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], a["u_tr"], w.cfg.vote_range)
            heads = torch.full((P, 8), -3.0, device=w.dev)
            w.enc.forward_decode_sel(a["pc"], a["pc_normal"], a["feat"], a["point_idxs"], a["u_rot"], sel, n_sel, heads)
        return dict(heads=heads)
    want = run()
    full = run_decode(w)["heads"]
    rows = sel[:int(n_sel)].long()
    assert torch.equal(want["heads"][rows], full[rows]) and float((want["heads"] == -3.0).float().mean()) > 0.6
    for arg, forms in dict(ENC_ARGS, u_rot=UNIFORMS).items():
        for form in forms:
            c, f = form(w.t[arg])
            _same(run(**{arg: c}), run(**{arg: f}))
    pairs = {a: ALL_AT_ONCE[a](w.t[a]) for a in ("pc", "pc_normal", "feat", "point_idxs", "u_rot")}
    _same(run(**{a: c for a, (c, _) in pairs.items()}), run(**{a: f for a, (_, f) in pairs.items()}))


def test_forward_decode_batch_forms(work):
    """forward_decode_batch: two lists in one launch; each argument of one item in every form gives the bits of the canonical
    batch, which are the bits of one forward_decode call per item"""
    w = work
    t = w.t
    other = dict(t, u_tr=t["u_rot"], u_rot=t["u_tr"], point_idxs=t["point_idxs"].flip(0).contiguous())

    def run(**a):
        items = [dict(encoder=w.enc, pc=x["pc"], pc_normal=x["pc_normal"], feat=x["feat"], idxs=x["point_idxs"], u_tr=x["u_tr"],
                      u_rot=x["u_rot"], vote_range=w.cfg.vote_range) for x in (other, dict(t, **a))]
        with torch.no_grad():
            outs = model_mod.forward_decode_batch(items)
        return dict(o0=outs[0][0], h0=outs[0][1], o1=outs[1][0], h1=outs[1][1])
    want = run()
    single = run_decode(w)
    assert torch.equal(want["o1"], single["outputs"]) and torch.equal(want["h1"], single["heads"])
    for arg, forms in POSE_ARGS.items():
        for form in forms:
            c, f = form(t[arg])
            _same(run(**{arg: c}), run(**{arg: f}))
    pairs = {a: ALL_AT_ONCE[a](t[a]) for a in POSE_ARGS}
    _same(run(**{a: c for a, (c, _) in pairs.items()}), run(**{a: f for a, (_, f) in pairs.items()}))


# numpy forms of a host array: (canonical, formed)
def np_f64(a):
    return a, a.astype(np.float64)


def np_col_slice(a):
    wide = np.full((a.shape[0], 2 * a.shape[1]), JUNK, a.dtype)
    wide[:, a.shape[1]:] = a
    return a, wide[:, a.shape[1]:]


def np_row_stride(a):
    big = np.full((2 * a.shape[0],) + a.shape[1:], JUNK, a.dtype)
    big[::2] = a
    return a, big[::2]


def np_fortran(a):
    return a, np.asfortranarray(a)


NUMPY_FORMS = [np_f64, np_col_slice, np_row_stride, np_fortran]
POSE_KEYS = ("argmax", "peak", "n_surv", "T", "up", "right", "scale", "losses", "dims")


def test_training_infer_forms(work):
    """training.infer takes host arrays: a float64 cloud, `cloud[:, 3:6]` of a points-and-normals array, strided rows, Fortran order"""
    from cppf_amd import training
    w = work
    ob = dict(pc=w.ob["pc"], normals=w.ob["normals"], cfg=w.cfg)
    run = lambda **a: {k: v for k, v in training.infer(w.penc, w.enc, dict(ob, **a), w.dev, n_pairs=N * K, seed=1, sphere=w.sph).items()
                       if k in POSE_KEYS}
    want = run()
    assert want["n_surv"] > 0
    for arg in ("pc", "normals"):
        for form in NUMPY_FORMS:
            c, f = form(ob[arg])
            assert not f.flags.c_contiguous or f.dtype != c.dtype
            _same(want, run(**{arg: f}))
    _same(want, run(pc=np_col_slice(ob["pc"])[1], normals=np_f64(ob["normals"])[1]))


def test_batch_runner_one_argument_at_a_time(work):
    """BatchPoseRunner: put() of device tensors and run() of host arrays, each of pc / normals / feat of one object in every form
    (the pairs and bin uniforms are drawn on the device: an object carries no index or uniform argument on these paths)"""
    from cppf_amd.batch import BatchPoseRunner
    w = work
    runner = BatchPoseRunner({"mug": w.enc}, w.dev, n_lanes=1)
    dev_obj = dict(pc=w.t["pc"], normals=w.t["pc_normal"], feat=w.t["feat"], cfg=w.cfg, n_pairs=N * K)
    host_obj = dict(pc=w.ob["pc"], normals=w.ob["normals"], feat=w.ob["feat"], cfg=w.cfg, n_pairs=N * K)
    rec = lambda objs: runner.run(objs, seed=3).cpu().numpy()
    want = rec(runner.put([dev_obj, dev_obj]))
    assert np.isfinite(want[:, :12]).all() and np.array_equal(want, rec([host_obj, host_obj]))
    for key, arg in (("pc", "pc"), ("normals", "pc_normal"), ("feat", "feat")):
        for form in FLOAT_2D:
            c, f = form(w.t[arg])
            a = rec(runner.put([dev_obj, dict(dev_obj, **{key: c})]))
            b = rec(runner.put([dev_obj, dict(dev_obj, **{key: f})]))
            assert np.array_equal(a, b), (key, form.__name__)
        for form in NUMPY_FORMS:
            c, f = form(host_obj[key])
            assert np.array_equal(want, rec([host_obj, dict(host_obj, **{key: f})])), (key, form.__name__)
            assert np.array_equal(want, rec(runner.put([host_obj, dict(host_obj, **{key: f})]))), (key, form.__name__)


def test_frame_runner_forms(work):
    """FrameRunner.run takes a host depth image and host masks: a strided / Fortran-ordered depth, uint8, non-bool integer, strided
    and Fortran-ordered masks give the poses of the canonical frame (the reference's demo frame, two instances)"""
    import os
    from conftest import GOLDEN
    from cppf_amd import training
    from cppf_amd.config import CATEGORIES
    from cppf_amd.frames import FrameRunner
    from cppf_amd.utils.util import read_depth_png
    from test_real_frame import DEPTH, instances
    depth = read_depth_png(DEPTH)
    inst = [instances(depth)[i] for i in (0, 3)]
    assert [c for c, _ in inst] == ["mug", "mug"] and all(m.dtype == np.bool_ and m.flags.c_contiguous for _, m in inst)
    penc, enc = training.load_weights(os.path.join(GOLDEN, "trained_mug.npz"), CATEGORIES["mug"], work.dev)
    runner = FrameRunner({"mug": enc}, {"mug": penc}, work.dev, n_pairs=4000)
    keys = ("n_points", "argmax", "peak", "n_surv", "T", "up", "right", "scale")
    run = lambda d, ii: [{k: p[k] for k in keys} for p in runner.run(d, ii, seed=3)]
    want = run(depth, inst)
    assert all(p["n_points"] > 100 and p["n_surv"] > 0 for p in want)

    def check(got):
        for a, b in zip(want, got):
            _same(a, b)
    for form in (np_col_slice, np_row_stride, np_fortran):
        f = form(depth)[1]
        assert not f.flags.c_contiguous and f.dtype == np.uint16
        check(run(f, inst))
    mask_forms = [lambda m: m.astype(np.uint8), lambda m: m.astype(np.int32) * 5, lambda m: np_col_slice(m)[1], lambda m: np_fortran(m)[1],
                  lambda m: np_row_stride(m.astype(np.uint8))[1]]
    for mf in mask_forms:
        check(run(depth, [(inst[0][0], mf(inst[0][1])), inst[1]]))
    check(run(np_fortran(depth)[1], [(c, np_col_slice(m.astype(np.uint8))[1]) for c, m in inst]))


# ------------------------------------------------------------------------------------------------ autograd
def test_backward_with_strided_feat_and_gradient(work):
    """forward_with_idx under autograd (the shape of test_gpu_backward._run, 129 pairs): a feat that is a column slice and an
    upstream gradient with transposed storage give the parameter gradients and feat.grad of the canonical run bit for bit"""
    w = work
    P = 129
    rng = np.random.default_rng(P)
    R = w.d(rng.normal(0, 1, (P, w.cfg.out_dim)).astype(np.float32))
    idxs = w.t["point_idxs"][:P].contiguous()
    enc = w.enc.train()

    def run(feat_leaf, feat_used, weight):
        enc.zero_grad()
        logits = enc.forward_with_idx(w.t["pc"], w.t["pc_normal"], feat_used, idxs)
        (logits * weight).sum().backward()
        return dict(logits=logits.detach(), gf=feat_leaf.grad, **{n: p.grad.clone() for n, p in enc.named_parameters()})

    try:
        f0 = w.t["feat"].clone().requires_grad_(True)
        want = run(f0, f0, R)
        c = w.t["feat"].shape[1]
        wide = torch.full((N, 3 * c), float(JUNK), device=w.dev)
        wide[:, c:2 * c] = w.t["feat"]
        wide.requires_grad_(True)                                                     # the leaf is the wide buffer
        got = run(wide, wide[:, c:2 * c], transposed_storage(R)[1])
        assert not wide[:, c:2 * c].is_contiguous()
        got["gf"] = got["gf"][:, c:2 * c]
        assert float(wide.grad[:, :c].abs().sum()) == 0 and float(wide.grad[:, 2 * c:].abs().sum()) == 0
        _same(want, got)
        # a gradient that arrives strided: the sum over a transposed product hands the backward a transposed grad_out
        f1 = w.t["feat"].clone().requires_grad_(True)
        enc.zero_grad()
        logits = enc.forward_with_idx(w.t["pc"], w.t["pc_normal"], f1, idxs)
        (logits.t() * R.t().contiguous()).sum().backward()
        got2 = dict(logits=logits.detach(), gf=f1.grad, **{n: p.grad.clone() for n, p in enc.named_parameters()})
        _same(want, got2)
    finally:
        enc.eval()
        enc.zero_grad()


# ------------------------------------------------------------------------------------------------ refusals: never a launch
def _no_launch(monkeypatch):
    """from here on anything that would reach the library fails the test"""
    boom = lambda *a, **k: pytest.fail("launched")
    monkeypatch.setattr(tu, "call", boom)
    monkeypatch.setattr(tu, "fill", boom)
    for mod in (voting, model_mod, inference, zero_shot):
        monkeypatch.setattr(mod, "call", boom)
        if hasattr(mod, "fill"):
            monkeypatch.setattr(mod, "fill", boom)
    monkeypatch.setattr(_lib, "lib", boom)


def cpu(x):
    return x, x.cpu()


STRIDED, WRONG_TYPE = ValueError, TypeError
DROPIN_FORMS = [(col_slice, STRIDED), (row_stride, STRIDED), (transposed_storage, STRIDED), (f64, WRONG_TYPE), (f16, WRONG_TYPE),
                (other_int, WRONG_TYPE), (cpu, ValueError)]


def _applies(form, x):
    if form in (f64, f16):
        return x.dtype.is_floating_point
    if form is other_int:
        return not x.dtype.is_floating_point
    if form is transposed_storage:
        return x.dim() == 2
    if form is col_slice:
        return x.dim() >= 2                      # (a slice of a 1-D tensor is contiguous: canonical for the drop-ins)
    return True


def test_dropin_kernels_refuse_every_other_form(work, monkeypatch):
    """ppf_kernel / backvote_kernel / rot_voting_kernel write in place and never convert: every tensor argument in every other
    form raises dev_tensor's ValueError (strided, wrong device) / TypeError (dtype) and nothing is launched.  A second GPU is not
    assumed: a tensor on another GPU is covered by the stub test of tests/test_abi_and_host.py (and by dev_tensor's device check
    exercised here with the CPU as the other device)."""
    w = work
    dev, P, ROTS = w.dev, N * K, 72
    corners, dims = grid_shape(w.ob["pc"], w.cfg.res)
    idx32 = w.t["point_idxs"].int()
    outputs = torch.rand((P, 2), device=dev)
    grid = torch.zeros(dims, device=dev)
    corner = torch.from_numpy(corners[0].copy()).to(dev)
    res = np.float32(w.cfg.res)
    kernels = {
        "ppf": (voting.ppf_kernel, [w.t["pc"], outputs, w.t["probs"], idx32, grid, corner, res, P, ROTS, *dims, True]),
        "backvote": (voting.backvote_kernel, [w.t["pc"], outputs, torch.zeros((P, 3), device=dev), idx32, corner, res, P, ROTS, *dims,
                                              torch.zeros(3, device=dev), np.float32(3 * res)]),
        "rot": (voting.rot_voting_kernel, [w.t["pc"], outputs, torch.rand(P, device=dev), torch.zeros((P, ROTS, 3), device=dev), idx32,
                                           corner, res, P, ROTS, *dims]),
    }
    _no_launch(monkeypatch)
    n_cases = 0
    for name, (kernel, args) in kernels.items():
        for i, x in enumerate(args):
            if not isinstance(x, torch.Tensor) or (name == "rot" and i in (1, 5)):        # (rot_voting ignores `not_used` and corner)
                continue
            for form, exc in DROPIN_FORMS:
                if not _applies(form, x):
                    continue
                bad = list(args)
                bad[i] = form(x)[1]
                with pytest.raises(exc):
                    kernel((1, 1, 1), (512, 1, 1), tuple(bad))
                n_cases += 1
    assert n_cases > 60 and float(grid.abs().sum()) == 0


def test_host_resident_arguments_are_refused_before_any_launch(work, monkeypatch):
    """a pc_normal / feat / idxs / dist / u left on the CPU: refused by name by the encoders, estimate_center and estimate_pose, and
    nothing is launched (a numpy pair list is data to upload; a CPU tensor where a device tensor belongs is a mistake)"""
    w = work
    t = _tensors(w)
    _no_launch(monkeypatch)
    with torch.no_grad():
        for arg in ("pc_normal", "feat", "point_idxs"):
            for run in (run_with_idx, run_forward, run_decode, run_pose, run_center):
                with pytest.raises(ValueError, match="idxs" if arg == "point_idxs" else arg):
                    run(w, **{arg: t[arg].cpu()})
        for arg in ("u_tr", "u_rot"):
            for run in (run_decode, run_pose, run_center):
                with pytest.raises(ValueError, match=arg):
                    run(w, **{arg: t[arg].cpu()})
        with pytest.raises(ValueError, match="pc: expected a tensor on a HIP device"):
            run_pose(w, pc=t["pc"].cpu())
        with pytest.raises(ValueError, match="pc: expected a tensor on a HIP device"):
            run_center(w, _grid=w.grid0, pc=t["pc"].cpu())
        for run in (run_decode, run_with_idx, run_forward):               # (pc is looked at first: the error names it, not the pair list)
            with pytest.raises(_lib.CppfError, match="pc: PPFEncoder inference runs on a HIP device only"):
                run(w, pc=t["pc"].cpu())
        with pytest.raises(_lib.CppfError, match="PointEncoder inference runs on a HIP device only"):
            run_point_encoder(w, pc=t["pc"].cpu())
        with pytest.raises(ValueError, match="probs"):
            run_center(w, probs=t["probs"].cpu())
        for arg in ("pc_normal", "dist"):
            with pytest.raises(ValueError, match=arg):
                run_point_encoder(w, **{arg: t[arg].cpu()})
        with pytest.raises(ValueError, match="heads"):
            w.enc.forward_decode_sel(t["pc"], t["pc_normal"], t["feat"], t["point_idxs"], t["u_rot"], torch.zeros(N * K, dtype=torch.int32, device=w.dev),
                                     torch.zeros(1, dtype=torch.int32, device=w.dev), torch.zeros((N * K, 8)))
        nbrs = torch.zeros((N, 16), dtype=torch.int32, device=w.dev)
        with pytest.raises(ValueError, match="nbrs_idx: tensor on cpu"):
            w.penc.forward_nbrs(t["pc"][None], t["pc_normal"][None], nbrs.cpu()[None])
        for bad in (nbrs.short(), nbrs.float()):
            with pytest.raises(TypeError, match="nbrs_idx"):
                w.penc.forward_nbrs(t["pc"][None], t["pc_normal"][None], bad[None])
        # forward_decode_batch: the same rule for every member of the launch
        item = dict(encoder=w.enc, pc=t["pc"], pc_normal=t["pc_normal"], feat=t["feat"], idxs=t["point_idxs"], u_tr=t["u_tr"],
                    u_rot=t["u_rot"], vote_range=w.cfg.vote_range)
        for key, name in (("pc_normal", "pc_normal"), ("feat", "feat"), ("idxs", "idxs"), ("u_tr", "u_tr"), ("u_rot", "u_rot")):
            with pytest.raises(ValueError, match=name + ": tensor on cpu"):
                model_mod.forward_decode_batch([dict(item, **{key: item[key].cpu()}), item])
        with pytest.raises(_lib.CppfError, match="pc: PPFEncoder inference runs on a HIP device only"):
            model_mod.forward_decode_batch([dict(item, pc=t["pc"].cpu()), item])
        # the zero-shot functions: a numpy pair list / corner is host data, a CPU tensor beside device tensors is refused
        for fn in (lambda **a: zero_shot.distinct_pairs(**dict(dict(pc=t["pc"], nrm=t["pc_normal"], idx=t["point_idxs"]), **a)),
                   lambda **a: zero_shot.zero_shot_scene(w.enc9, **dict(dict(pc=t["pc"], nrm=t["pc_normal"], feat=t["feat"], idx=t["point_idxs"],
                                                                            cfg=w.cfg), **a))):
            with pytest.raises(ValueError, match="nrm: tensor on cpu"):
                fn(nrm=t["pc_normal"].cpu())
            with pytest.raises(ValueError, match="pair list: tensor on cpu"):
                fn(idx=t["point_idxs"].cpu())
            with pytest.raises(TypeError, match="pair list"):
                fn(idx=t["point_idxs"].float())
        seg = lambda **a: zero_shot.segment_instance(**dict(dict(pc=t["pc"], outputs=t["u_tr"], idx=t["point_idxs"], center=np.zeros(3),
                                                                 corner=w.grid0[0][0], res=w.cfg.res, dims=w.grid0[1]), **a))
        for arg, name in (("outputs", "outputs"), ("idx", "pair list"), ("corner", "corner")):
            x = dict(outputs=t["u_tr"], idx=t["point_idxs"], corner=torch.zeros(3, device=w.dev))[arg]
            with pytest.raises(ValueError, match=name + ": tensor on cpu"):
                seg(**{arg: x.cpu()})
        for bad in (t["point_idxs"].short(), t["point_idxs"].float()):
            with pytest.raises(TypeError, match="int64/int32|one of"):
                run_pose(w, point_idxs=bad)
            with pytest.raises(TypeError, match="int64/int32"):
                run_with_idx(w, point_idxs=bad)
