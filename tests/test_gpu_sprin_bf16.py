"""The bf16 point encoder (csrc/sprin_bf16.hip, PointEncoder.set_precision("bf16")) on the device.

1. shared tail and last layer, exactly: on a rounding-free weight set the bf16 output is the fp32 kernel's, bit for bit, in every form
2. against the CPU emulation E (tests/sprin_bf16_ref.py, k ascending): a point matches when every local column is within
   tol = 4 x the fp32 restatement's own order spread; at most 10 % of a case's points may miss, and those stay within 2 x max|E - F|
   of F; the global columns are one row repeated and are GlobalInfoProp of the device's own local columns
3. forward = forward_nbrs = forward_dyn = a member of point_encoder_forward_batch, bit for bit, under bf16
4. captured pipelines: replay == eager under bf16; fp32 -> bf16 -> fp32 gives a fresh fp32 encoder's records
5. the committed trained networks recover the held-out poses with the point encoder (and both encoders) in bf16, within the fp32
   test's own thresholds
6. refusals: mixed precisions in a batch, gradients, other architectures, the C return codes

Measured on one MI355X (DESIGN.md 3.5a carries the tables): see the figures each test prints."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
import sprin_bf16_cases as cases
import sprin_bf16_ref as R
from conftest import GOLDEN
from cppf_amd import _lib, training
from cppf_amd._torch_util import call, fill, scratch
from cppf_amd.inference import PosePipeline, grid_shape
from cppf_amd.models.model import PointEncoder, point_encoder_forward_batch
from test_gpu_configs import make_encoder, seeded_sd

pytestmark = pytest.mark.gpu
STD = [32, 64, 32, 32]


def penc_of(sd, dev, precision, k, num_layers=1):
    enc = PointEncoder(k=k, spfcs=STD, num_layers=num_layers, out_dim=32)
    enc.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in sd.items()})
    return enc.to(dev).eval().set_precision(precision)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def out_nbrs(enc, pc, nrm, nbrs, dev):
    with torch.no_grad():
        return enc.forward_nbrs(_t(pc[None], dev), _t(nrm[None], dev), _t(nbrs.astype(np.int64)[None], dev))[0].cpu().numpy()


def _padded(pc, nrm, nbrs, cap, k, dev, ready=True):
    n = pc.shape[0]
    pcd, nrmd = torch.full((cap, 3), 7.0, device=dev), torch.full((cap, 3), 7.0, device=dev)
    pcd[:n], nrmd[:n] = _t(pc, dev), _t(nrm, dev)
    nb = torch.full((cap, k), -5, dtype=torch.int32, device=dev)
    if ready:
        nb[:n] = _t(nbrs.astype(np.int32), dev)
    return dict(pc=pcd, nrm=nrmd, n_dev=torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev), nbrs=nb, nbrs_ready=ready,
                out=torch.full((cap, 40), -3.0, device=dev))


def out_dyn(enc, pc, nrm, nbrs, cap, dev, ready=True):
    """forward_dyn in capacity-sized buffers; rows beyond the point count must stay untouched"""
    m = _padded(pc, nrm, nbrs, cap, enc.k, dev, ready)
    with torch.no_grad():
        out = enc.forward_dyn(m["pc"], m["nrm"], m["n_dev"], out=m["out"], nbrs=m["nbrs"], nbrs_ready=ready)
    assert bool((out[pc.shape[0]:] == -3.0).all())
    return out[:pc.shape[0]].cpu().numpy()


def out_batch(encs, clouds, caps, dev, ready=None):
    """point_encoder_forward_batch; clouds: (pc, nrm, nbrs) per member"""
    ready = ready or [True] * len(encs)
    members = [dict(_padded(pc, nrm, nbrs, cap, e.k, dev, r), encoder=e) for e, (pc, nrm, nbrs), cap, r in zip(encs, clouds, caps, ready)]
    with torch.no_grad():
        outs = point_encoder_forward_batch(members)
    assert outs is not None
    for o, (pc, _, _) in zip(outs, clouds):
        assert bool((o[pc.shape[0]:] == -3.0).all())
    return [o[:c[0].shape[0]].cpu().numpy() for o, c in zip(outs, clouds)]


# ------------------------------------------------------------------------------------------------ 1. shared tail, layer 5
@pytest.mark.parametrize("num_layers", [1, 2])
@pytest.mark.parametrize("n,k", cases.EXACT_NK)
def test_rounding_free_set_equals_the_fp32_kernel_bit_for_bit(dev, n, k, num_layers):
    sd = cases.exact_weights(num_layers)
    e32, e16 = penc_of(sd, dev, "fp32", k, num_layers), penc_of(sd, dev, "bf16", k, num_layers)
    if k > n:       # more neighbours than points: neither precision serves it, and both say so the same way
        pc, nrm = cases._cloud(n, 5 * n + k)
        nbrs = np.zeros((n, k), np.int32)
        for e in (e32, e16):
            with pytest.raises(_lib.CppfError, match="no device kernel"):
                out_nbrs(e, pc, nrm, nbrs, dev)
        return
    pc, nrm, nbrs = cases.cloud(n, k)
    E, changed = R.forward(sd, pc, nrm, nbrs, "asc", True, num_layers)
    assert not changed                                   # (on the CPU: no bf() changed anything, and kern is exact in any order)
    g32, g16 = out_nbrs(e32, pc, nrm, nbrs, dev), out_nbrs(e16, pc, nrm, nbrs, dev)
    assert g16.shape == (n, 40) and np.isfinite(g16).all()
    np.testing.assert_allclose(g32, E, atol=2e-5, rtol=0)     # the case is what the CPU says it is
    assert np.array_equal(g16, g32), np.argwhere(g16 != g32)[:4]
    assert np.array_equal(out_dyn(e16, pc, nrm, nbrs, n + 3, dev), g32)
    assert np.array_equal(out_dyn(e32, pc, nrm, nbrs, n + 3, dev), g32)
    if num_layers == 1:
        (b16,) = out_batch([e16], [(pc, nrm, nbrs)], [n + 5], dev)
        assert np.array_equal(b16, g32)


# ------------------------------------------------------------------------------------------------ 2. numerics
@pytest.mark.parametrize("name,n,k,num_layers", cases.NUMERIC_CASES)
def test_against_the_emulation(dev, name, n, k, num_layers):
    """Measured on one MI355X: DESIGN.md 3.5a holds max|G - E|, its ratio to the fp32 order spread, the unmatched share and the
    unmatched points' max|G - F| per case."""
    b = cases.bounds(name, n, k, num_layers)
    pc, nrm, nbrs = cases.cloud(n, k, name)
    sd = cases.weights(name, num_layers)
    G = out_nbrs(penc_of(sd, dev, "bf16", k, num_layers), pc, nrm, nbrs, dev).astype(np.float64)
    err = np.abs(G - b["E"])[:, :32].max(1)
    matched = err <= b["tol"]
    share, spread = float(np.mean(~matched)), b["tol"] / 4.0
    worst = float(np.abs(G - b["F"])[~matched][:, :32].max()) if (~matched).any() else 0.0
    print(f"{name} N={n} k={k} layers={num_layers}: fp32 order spread {spread:.3g}, tol {b['tol']:.3g}; max|G-E| = {err.max():.3g}; matched points: "
          f"max|G-E| = {err[matched].max() if matched.any() else float('nan'):.3g} = "
          f"{err[matched].max() / spread if matched.any() else float('nan'):.2f} x spread; unmatched share {share:.2%}; "
          f"unmatched max|G-F| = {worst:.3g}, cap {b['cap']:.3g}")
    assert share <= 0.10
    assert worst <= b["cap"]
    # the global columns: one row repeated, and GlobalInfoProp (linear + maximum) of the device's own local columns
    assert np.array_equal(G[:, 32:], np.broadcast_to(G[:1, 32:], (n, 8)))
    want = R.global_columns(sd, num_layers - 1, G[:, :32].astype(np.float32)).astype(np.float64)
    assert np.abs(G[0, 32:] - want).max() <= b["tol"]


# ------------------------------------------------------------------------------------------------ 3. forms
def test_forms_agree_bit_for_bit_under_bf16(dev):
    sizes, k = (64, 130, 700, 9, 257), 9
    ready = [False, True, False, True, True]
    encs = [penc_of(cases.weights(("trained_bottle", "random")[i % 2]), dev, "bf16", k) for i in range(len(sizes))]
    clouds, want = [], []
    for i, n in enumerate(sizes):
        pc, nrm = cases._cloud(n, 700 + i)
        with torch.no_grad():
            nbrs = encs[i].neighbours(_t(pc, dev)).cpu().numpy()
            fwd = encs[i](_t(pc[None], dev), _t(nrm[None], dev))[0].cpu().numpy()
        assert np.array_equal(nbrs, cases.knn(pc, k))
        assert np.array_equal(out_nbrs(encs[i], pc, nrm, nbrs, dev), fwd), i
        for rdy in (True, False):
            assert np.array_equal(out_dyn(encs[i], pc, nrm, nbrs, 2 * n, dev, rdy), fwd), (i, rdy)
        clouds.append((pc, nrm, nbrs))
        want.append(fwd)
    for i, got in enumerate(out_batch(encs, clouds, [2 * n for n in sizes], dev, ready)):
        assert np.array_equal(got, want[i]), i
    assert not np.array_equal(want[0][:9], want[3])       # (two weight sets, two clouds: the members really differ)


# ------------------------------------------------------------------------------------------------ 4. pipelines
def _pose_pipe(dev, sph, ppf, penc, use_graph=True):
    ob = syn.make_object("mug", 700, 11)
    idx = syn.make_pairs(700, 24, 11)
    u_tr, u_rot = syn.make_uniforms(idx.shape[0], 11)
    corners, dims = grid_shape(ob["pc"], ob["cfg"].res)
    p = PosePipeline(ppf, ob["cfg"], 700, idx.shape[0], dims, dev, sph, point_encoder=penc, use_graph=use_graph)
    p.load(ob["pc"], ob["normals"], None, idx, u_tr, u_rot, corners[0].copy())
    return p


def _rec(p, **kw):
    p.run(**kw)
    return p.ws.rec.cpu().numpy().copy(), p.feat.cpu().numpy().copy()


def test_pose_pipeline_replay_equals_eager_and_the_precision_switch(golden, dev):
    sph = golden("sphere.npz")["pts"]
    ppf = make_encoder(seeded_sd(0, 4.0), dev)
    sd = cases.weights("trained_mug")
    penc = penc_of(sd, dev, "fp32", 60)
    p = _pose_pipe(dev, sph, ppf, penc)
    rec32, feat32 = _rec(p)
    assert np.array_equal(_rec(p)[0], rec32)             # capture, then replay
    penc.set_precision("bf16")
    got = [_rec(p) for _ in range(3)]                    # capture again (never the fp32 graph), replay, replay
    rec16, feat16 = _rec(_pose_pipe(dev, sph, ppf, penc, use_graph=False))      # eager
    for r, f in got:
        assert np.array_equal(r, rec16) and np.array_equal(f, feat16)
    assert not np.array_equal(feat16, feat32) and not np.array_equal(rec16, rec32)     # the switch really changed the arithmetic
    penc.set_precision("fp32")
    back = [_rec(p) for _ in range(2)]
    recf, featf = _rec(_pose_pipe(dev, sph, ppf, penc_of(sd, dev, "fp32", 60)))
    assert np.array_equal(recf, rec32) and np.array_equal(featf, feat32)
    for r, f in back:
        assert np.array_equal(r, rec32) and np.array_equal(f, feat32)
    # check_weights=False looks at no image: the precision alone must keep the stale graph from replaying
    penc.set_precision("bf16")
    r, f = _rec(p, check_weights=False)
    assert np.array_equal(r, rec16) and np.array_equal(f, feat16)


def test_batch_runner_replay_equals_eager(dev):
    from cppf_amd.batch import BatchPoseRunner
    cats = ["bottle", "mug", "bowl"]
    sd = seeded_sd(0, 4.0)
    objects = []
    for j in range(4):
        ob = syn.make_object(cats[j % 3], 600 + 50 * j, 400 + j)
        idx = syn.make_pairs(ob["pc"].shape[0], 24, 400 + j)
        u_tr, u_rot = syn.make_uniforms(idx.shape[0], 400 + j)
        objects.append(dict(pc=ob["pc"], normals=ob["normals"], point_idxs=idx, u_tr=u_tr, u_rot=u_rot, cfg=ob["cfg"]))
    encs = {c: make_encoder(sd, dev) for c in cats}
    pencs = {c: penc_of(cases.weights(("trained_bottle", "trained_mug", "random")[i]), dev, "bf16", 60) for i, c in enumerate(cats)}
    want = BatchPoseRunner(encs, dev, use_graph=False, chain_len=1, point_encoders=pencs).run(objects).cpu().numpy()
    runner = BatchPoseRunner(encs, dev, chain_len=2, point_encoders=pencs)
    for rep in range(3):                                 # solo graphs, chains captured, chains replayed
        np.testing.assert_array_equal(runner.run(objects).cpu().numpy(), want)
    for e in pencs.values():
        e.set_precision("fp32")
    got32 = runner.run(objects).cpu().numpy()
    fresh = BatchPoseRunner(encs, dev, chain_len=2, point_encoders={c: penc_of(cases.weights(("trained_bottle", "trained_mug", "random")[i]), dev, "fp32", 60)
                                                                    for i, c in enumerate(cats)})
    np.testing.assert_array_equal(got32, fresh.run(objects).cpu().numpy())
    assert not np.array_equal(got32, want)


def test_frame_runner_equals_the_eager_loop_with_both_encoders_in_bf16(dev):
    from cppf_amd.config import CATEGORIES
    from cppf_amd.frames import FrameRunner, frame_poses
    from cppf_amd.utils.util import read_depth_png
    from test_real_frame import DEPTH, instances
    depth = read_depth_png(DEPTH)
    inst = instances(depth)[:5]                           # (the laptop needs a many-tile pipeline: eager on first sight, no new ground)
    encs, pencs = {}, {}
    for cat, src in (("mug", "mug"), ("bowl", "bottle"), ("can", "bottle")):
        penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{src}.npz"), CATEGORIES[src], dev)
        encs[cat], pencs[cat] = enc, penc
    want32 = frame_poses(depth, inst, encs, pencs, n_pairs=20000, device=dev, seed=3)
    for c in encs:
        encs[c].set_precision("bf16")
        pencs[c].set_precision("bf16")
    want = frame_poses(depth, inst, encs, pencs, n_pairs=20000, device=dev, seed=3)
    runner = FrameRunner(encs, pencs, dev, n_pairs=20000)
    for rep in range(4):                                  # members' own graphs, chains captured, replays
        got = runner.run(depth, inst, seed=3)
        for i, (w, g) in enumerate(zip(want, got)):
            assert w is not None and g is not None, (rep, i)
            assert g["n_points"] == w["n_points"] and g["argmax"] == w["argmax"] and g["n_surv"] == w["n_surv"], (rep, i)
            for key in ("T", "up", "right", "scale", "R"):
                assert np.array_equal(g[key], w[key]), (rep, i, key)
    assert any(a["n_surv"] != b["n_surv"] or not np.array_equal(a["up"], b["up"]) for a, b in zip(want, want32))


# ------------------------------------------------------------------------------------------------ 5. poses
def _med(errs, key):
    return float(np.median([e[key] for e in errs]))


@pytest.mark.parametrize("cat", ["bottle", "mug", "laptop"])
def test_committed_trained_weights_recover_held_out_poses_under_bf16(dev, cat):
    """tests/test_gpu_trained.py::test_committed_trained_weights_recover_held_out_poses with the point encoder in bf16 (pair encoder
    fp32), then with both in bf16: the same networks, the same held-out objects, the same thresholds"""
    from test_gpu_trained import _held_out
    cfg = syn.CATEGORIES[cat]
    penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
    keys = ("t_cells", "up_deg_mod_sign", "scale_rel") + (("right_deg_mod_sign",) if cfg.regress_right else ())
    errs32 = _held_out(penc, enc, cat, dev)
    runs = {"point bf16": _held_out(penc.set_precision("bf16"), enc, cat, dev),
            "both bf16": _held_out(penc, enc.set_precision("bf16"), cat, dev)}
    for what, errs in runs.items():
        print(cat, f"medians fp32 | {what}:", {k: (round(_med(errs32, k), 3), round(_med(errs, k), 3)) for k in keys},
              "min survivors", min(e["n_surv"] for e in errs32), "|", min(e["n_surv"] for e in errs))
    for what, errs in runs.items():
        assert _med(errs, "t_cells") <= 2.0 and max(e["t_cells"] for e in errs) <= 4.0, (what, errs)
        assert _med(errs, "up_deg_mod_sign") <= 5.0 and max(e["up_deg_mod_sign"] for e in errs) <= 12.0, (what, errs)
        assert _med(errs, "scale_rel") <= 0.10 and max(e["scale_rel"] for e in errs) <= 0.2, (what, errs)
        if cat == "bottle":
            assert sum(e["up_deg"] < 15 for e in errs) >= len(errs) - 1, (what, errs)
        if cfg.regress_right:
            assert _med(errs, "right_deg_mod_sign") <= 10.0, (what, errs)
        assert min(e["n_surv"] for e in errs) > 0.05 * 100000, what


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(dev):
    n, k = 96, 16
    pc, nrm, nbrs = cases.cloud(n, k)
    sd = cases.weights("random")
    e16, e32 = penc_of(sd, dev, "bf16", k), penc_of(sd, dev, "fp32", k)
    pcd, nrmd, nbd = _t(pc, dev), _t(nrm, dev), _t(nbrs, dev)
    # members of different precisions in one batch
    members = [dict(_padded(pc, nrm, nbrs, n, k, dev), encoder=e) for e in (e32, e16)]
    with torch.no_grad(), pytest.raises(_lib.CppfError, match="fp32.*bf16|bf16.*fp32"):
        point_encoder_forward_batch(members)
    # gradients: training mode, parameters or inputs that require grad under autograd; under no_grad it is inference
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16.train()(pcd[None], nrmd[None])
    e16.eval()
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16(pcd[None], nrmd[None])                       # (its parameters require grad and autograd is on)
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16.forward_nbrs(pcd[None], nrmd[None], nbd[None].long())
    m = _padded(pc, nrm, nbrs, n, k, dev)
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16.forward_dyn(m["pc"], m["nrm"], m["n_dev"], out=m["out"], nbrs=m["nbrs"], nbrs_ready=True)
    with pytest.raises(_lib.CppfError, match="inference only"):
        point_encoder_forward_batch([dict(m, encoder=e16)])
    for p in e16.parameters():
        p.requires_grad_(False)
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16(pcd[None].clone().requires_grad_(True), nrmd[None])
    out = e16(pcd[None], nrmd[None])                     # eval, nothing requires grad: inference even with autograd on
    assert out.shape == (1, n, 40) and not out.requires_grad
    # other architectures: refused, never served in fp32 behind the caller's back
    with pytest.raises(_lib.CppfError, match="bf16"):
        PointEncoder(k=60, spfcs=[32, 64, 64, 32], num_layers=1, out_dim=32).to(dev).set_precision("bf16")
    # the C entries
    packed, desc = e16._packed_weights(dev)
    hid, bad = (C.c_int * 4)(*STD), (C.c_int * 4)(32, 64, 64, 32)
    need = int(_lib.lib().cppf_point_encoder_workspace_bytes(n, 32, 8, 1))
    ws, small = torch.empty(need, dtype=torch.uint8, device=dev), torch.empty(need - 1, dtype=torch.uint8, device=dev)
    outd = torch.full((n, 40), -3.0, device=dev)
    fwd = lambda n_, k_, packed_, h_, ws_, pc_=pcd: call("cppf_point_encoder_bf16_forward", dev, pc_, nrmd, nbd, n_, k_, packed_, h_, 4, 32, 2,
                                                          32, 8, 1, outd, scratch(ws_), ok=(-1, -2, -3))
    assert fwd(n, k, packed, bad, ws) == _lib.EUNSUPPORTED
    assert fwd(n, 65, packed, hid, ws) == _lib.EUNSUPPORTED
    assert fwd(n, k, packed, hid, small) == -2           # CPPF_EWORKSPACE
    assert fwd(n, k, None, hid, ws) == -1                # CPPF_EINVAL
    assert fwd(n, k, packed, hid, ws, None) == -1
    assert fwd(0, k, packed, hid, ws) == 0 and bool((outd == -3.0).all())          # n_points == 0: a no-op
    dyn = lambda n_dev, ws_: call("cppf_point_encoder_bf16_forward_dyn", dev, pcd, nrmd, nbd, n, n_dev, k, packed, hid, 4, 32, 2, 32, 8, 1,
                                  outd, scratch(ws_), ok=(-1, -2, -3))
    assert dyn(None, ws) == -1 and dyn(m["n_dev"], small) == -2
    arr = (_lib.PointEncItem * 1)()
    bat = lambda k_, h_, layers: call("cppf_point_encoder_bf16_forward_batch", dev, 1, arr, k_, h_, 4, 32, 2, 32, 8, layers, ok=(-1, -2, -3))
    assert bat(k, bad, 1) == _lib.EUNSUPPORTED and bat(65, hid, 1) == _lib.EUNSUPPORTED and bat(k, hid, 2) == _lib.EUNSUPPORTED
    fill(arr[0], dev, pc=pcd, nrm=nrmd, nbrs=nbd, out=outd, n_dev=m["n_dev"], packed=packed, workspace=scratch(small), n_cap=n, nbrs_ready=True)
    assert bat(k, hid, 1) == -2
    fill(arr[0], dev, packed=None, workspace=scratch(ws))
    assert bat(k, hid, 1) == -1
    assert bool((outd == -3.0).all())                    # nothing was launched by any refused call
    assert call("cppf_point_encoder_bf16_pack_device", dev, None, hid, 4, 32, 2, 32, 8, 1, packed, ok=(-1,)) == -1
    assert call("cppf_point_encoder_bf16_pack_device", dev, packed, bad, 4, 32, 2, 32, 8, 1, packed, ok=(-3,)) == _lib.EUNSUPPORTED
