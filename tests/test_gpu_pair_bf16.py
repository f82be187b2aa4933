"""The bf16 pair encoder (csrc/pair_mlp_bf16.hip, PPFEncoder.set_precision("bf16")) on the device.

1. layout, exactly: on a rounding-free case the bf16 logits are the fp32 kernel's, bit for bit (k permutation, packer, every tail)
2. logits against the CPU emulation E (tests/pair_bf16_ref.py): a pair matches when every logit is within tol = 4 x the fp32
   restatement's own order spread; at most 2 % of a case's pairs may miss, and those stay within 2 x max|E - F| of F
3. the fused decode equals the stand-alone decode kernels on the bf16 forward's own logits, bit for bit
4. a batch equals its single lists bit for bit, in both workgroup mappings
5. the sel pass writes the survivors' rows of the all-heads first pass and nothing else
6. captured pipelines: replay == eager under bf16; fp32 -> bf16 -> fp32 gives a fresh fp32 encoder's records
7. the committed trained networks recover the held-out poses under bf16 within the fp32 test's own thresholds
8. refusals: mixed precisions in a batch, gradients, other architectures, second_pass 1 and 2 in one tail batch

Measured on one MI355X (DESIGN.md "bf16 pair encoder" carries the table): see the figures each test prints."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cppf_amd.synthetic as syn
import pair_bf16_cases as cases
from conftest import GOLDEN
from cppf_amd import _lib, training
from cppf_amd._torch_util import call
from cppf_amd.inference import PoseChain, PosePipeline, grid_shape
from cppf_amd.models.model import PPFEncoder, batch_plan, forward_decode_batch
from test_gpu_configs import make_encoder, seeded_sd

pytestmark = pytest.mark.gpu
STD = [84, 32, 32, 16]


def enc_of(sd, dev, precision, out_dim=141):
    enc = PPFEncoder(STD, out_dim)
    enc.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return enc.to(dev).eval().set_precision(precision)


def dev_inputs(c, dev):
    return tuple(torch.from_numpy(c[k]).to(dev) for k in ("pc", "nrm", "feat"))


def logits_of(enc, c, dev, P, i32=False):
    pc, nrm, feat = dev_inputs(c, dev)
    idx = torch.from_numpy(c["idxs"][:P].astype(np.int32) if i32 else c["idxs"][:P]).to(dev)
    with torch.no_grad():
        return enc.forward_with_idx(pc, nrm, feat, idx).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("out_dim", [141, 9])
def test_rounding_free_case_equals_the_fp32_kernel_bit_for_bit(dev, out_dim):
    import pair_bf16_ref as R
    d = cases.dyadic_case(out_dim)
    E, changed = R.forward(d["sd"], d["pc"], d["nrm"], d["feat"], d["idxs"], "asc", True)
    assert not changed                                  # (on the CPU: no bf() changed anything, so both precisions are exact)
    e32, e16 = enc_of(d["sd"], dev, "fp32", out_dim), enc_of(d["sd"], dev, "bf16", out_dim)
    for P in cases.P_CASES:
        for i32 in (False, True):
            g32, g16 = logits_of(e32, d, dev, P, i32), logits_of(e16, d, dev, P, i32)
            assert g16.shape == (P, out_dim)
            assert np.array_equal(g32, E[:P]), (P, i32)          # the case really is order-free: the fp32 kernel gives the CPU's bits
            assert np.array_equal(g16, g32), (P, i32, np.argwhere(g16 != g32)[:4])


# ------------------------------------------------------------------------------------------------ 2. numerics
@pytest.mark.parametrize("weights,out_dim", [("trained_bottle", 141), ("random", 141), ("random", 9)])
def test_logits_against_the_emulation(dev, weights, out_dim):
    """Measured on one MI355X: see DESIGN.md "bf16 pair encoder" for max|G - E| / spread and the unmatched share per case."""
    c, b = cases.case(weights, out_dim), cases.bounds(weights, out_dim)
    e16 = enc_of(c["sd"], dev, "bf16", out_dim)
    G = logits_of(e16, c, dev, cases.P_MAX).astype(np.float64)
    err = np.max(np.abs(G - b["E"]), -1)
    matched = err <= b["tol"]
    share = float(np.mean(~matched))
    spread = b["tol"] / 4.0
    print(f"{weights}/{out_dim}: |logit| <= {b['logit_max']:.3g}, fp32 order spread {spread:.3g}, tol {b['tol']:.3g}; matched pairs: "
          f"max|G-E| = {err[matched].max() if matched.any() else float('nan'):.3g} = {err[matched].max() / spread if matched.any() else float('nan'):.2f} x spread; "
          f"unmatched share {share:.4%} (emulation orders: {b['emu_share']:.4%}); "
          f"unmatched max|G-F| = {np.max(np.abs(G - b['F'])[~matched]) if (~matched).any() else 0.0:.3g}, cap {b['cap']:.3g}")
    assert share <= 0.02
    if (~matched).any():
        assert np.max(np.abs(G - b["F"])[~matched]) <= b["cap"]
    # every shorter list (tile tails, a last partial block) and both index widths: the same pairs, the same bits
    for P in cases.P_CASES:
        for i32 in (False, True):
            assert np.array_equal(logits_of(e16, c, dev, P, i32), G[:P].astype(np.float32)), (P, i32)


# ------------------------------------------------------------------------------------------------ 3. fusion
def _uniforms(P, seed, dev):
    rng = np.random.default_rng(seed)
    u_tr, u_rot = rng.random((P, 2), dtype=np.float32), rng.random((P, 2), dtype=np.float32)
    u_tr[::7] = -1.0                                     # arg-max mode
    u_rot[::5, 1] = -1.0
    u_rot[3::11, 0] = -1.0
    return torch.from_numpy(u_tr).to(dev), torch.from_numpy(u_rot).to(dev)


@pytest.mark.parametrize("weights", cases.WEIGHTS)
def test_fused_decode_equals_decode_kernels_on_the_bf16_logits(dev, weights):
    c = cases.case(weights)
    e16 = enc_of(c["sd"], dev, "bf16")
    pc, nrm, feat = dev_inputs(c, dev)
    vr = c["cfg"].vote_range
    for P in (17, 1000, 4099):
        idx = torch.from_numpy(c["idxs"][:P]).to(dev)
        u_tr, u_rot = _uniforms(P, P, dev)
        with torch.no_grad():
            logits = e16.forward_with_idx(pc, nrm, feat, idx)
            want_o = torch.empty((P, 2), dtype=torch.float32, device=dev)
            want_h = torch.empty((P, 8), dtype=torch.float32, device=dev)
            call("cppf_decode_center", dev, logits, P, 141, 32, float(vr[0]), float(vr[1]), u_tr, want_o)
            call("cppf_decode_rot", dev, logits, P, 141, 141, 32, 36, u_rot, want_h)
            got_o, got_h = e16.forward_decode(pc, nrm, feat, idx, u_tr, vr, u_rot)
            only_o, none = e16.forward_decode(pc, nrm, feat, idx, u_tr, vr)
        assert none is None
        assert torch.equal(got_o, want_o) and torch.equal(only_o, want_o), P
        assert torch.equal(got_h, want_h), P


# ------------------------------------------------------------------------------------------------ 4. batch
@pytest.mark.parametrize("lengths,per_xcd", [((4099,), 8), ((2000, 2000), 4), ((1000,) * 8, 1), ((1000, 17, 4099), 0),
                                             ((4099, 1), 0), ((16, 15, 17, 1, 1000, 333, 2048, 64), 0), ((1500, 1500, 1500), 0)])
def test_batch_equals_single_lists_bit_for_bit(dev, lengths, per_xcd):
    assert batch_plan(lengths)["per_xcd"] == per_xcd     # which of the two workgroup mappings this launch takes
    cs = [cases.case("trained_bottle"), cases.case("random")]
    encs = [enc_of(c["sd"], dev, "bf16") for c in cs]
    items, want = [], []
    for i, P in enumerate(lengths):
        c, enc = cs[i % 2], encs[i % 2]
        pc, nrm, feat = dev_inputs(c, dev)
        lo = (37 * i) % (cases.P_MAX - P + 1)
        idx = torch.from_numpy(c["idxs"][lo:lo + P] if i % 3 else c["idxs"][lo:lo + P].astype(np.int32)).to(dev)
        u_tr, u_rot = _uniforms(P, 100 + i, dev)
        items.append(dict(encoder=enc, pc=pc, pc_normal=nrm, feat=feat, idxs=idx, u_tr=u_tr, u_rot=u_rot, vote_range=c["cfg"].vote_range))
        with torch.no_grad():
            want.append(enc.forward_decode(pc, nrm, feat, idx, u_tr, c["cfg"].vote_range, u_rot))
    for heads in (True, False):
        its = items if heads else [{k: v for k, v in it.items() if k != "u_rot"} for it in items]
        with torch.no_grad():
            got = forward_decode_batch(its)
        for i, ((o, h), (wo, wh)) in enumerate(zip(got, want)):
            assert torch.equal(o, wo), (i, heads)
            assert (h is None) if not heads else torch.equal(h, wh), (i, heads)


# ------------------------------------------------------------------------------------------------ 5. sel pass
def test_sel_pass_writes_the_survivors_rows_only(dev):
    c = cases.case("trained_bottle")
    e16 = enc_of(c["sd"], dev, "bf16")
    pc, nrm, feat = dev_inputs(c, dev)
    P = 4099
    idx = torch.from_numpy(c["idxs"][:P]).to(dev)
    u_tr, u_rot = _uniforms(P, 3, dev)
    rng = np.random.default_rng(8)
    surv = np.sort(rng.choice(P, 1234, replace=False)).astype(np.int32)
    surv[-1] = P - 1                                     # the last pair of the last, partial block
    sel = torch.from_numpy(surv).to(dev)
    with torch.no_grad():
        _, all_heads = e16.forward_decode(pc, nrm, feat, idx, u_tr, c["cfg"].vote_range, u_rot)     # leaves the per-point table
        for n_sel, max_sel in ((1234, None), (1234, 500), (17, None), (0, None)):
            heads = torch.full((P, 8), -7.5, dtype=torch.float32, device=dev)
            e16.forward_decode_sel(pc, nrm, feat, idx, u_rot, sel, torch.tensor([n_sel], dtype=torch.int32, device=dev), heads,
                                   max_sel=max_sel)
            n = min(n_sel, P if max_sel is None else max_sel)
            rows = torch.from_numpy(surv[:n].astype(np.int64)).to(dev)
            assert torch.equal(heads[rows], all_heads[rows]), (n_sel, max_sel)
            rest = torch.ones(P, dtype=torch.bool, device=dev)
            rest[rows] = False
            assert bool((heads[rest] == -7.5).all()), (n_sel, max_sel)


# ------------------------------------------------------------------------------------------------ 6. pipelines
def _members(dev, sph, enc, specs, use_graph=True):
    pipes = []
    for cat, n, k, seed in specs:
        ob = syn.make_object(cat, n, seed)
        idx = syn.make_pairs(n, k, seed)
        u_tr, u_rot = syn.make_uniforms(idx.shape[0], seed)
        corners, dims = grid_shape(ob["pc"], ob["cfg"].res)
        p = PosePipeline(enc, ob["cfg"], n, idx.shape[0], dims, dev, sph, use_graph=use_graph)
        p.load(ob["pc"], ob["normals"], ob["feat"], idx, u_tr, u_rot, corners[0].copy())
        pipes.append(p)
    return pipes


def _rec(p):
    p.run()
    return p.ws.rec.cpu().numpy().copy(), p.outputs.cpu().numpy().copy()


SPECS = [("bottle", 700, 24, 1), ("mug", 640, 30, 2), ("laptop", 800, 20, 3)]


def test_pose_pipeline_replay_equals_eager_and_the_precision_switch(golden, dev):
    sph = golden("sphere.npz")["pts"]
    sd = seeded_sd(0, 4.0)
    enc = make_encoder(sd, dev)
    (p,) = _members(dev, sph, enc, SPECS[:1])
    rec32, out32 = _rec(p)
    rec32b, _ = _rec(p)                                 # capture, then replay
    assert np.array_equal(rec32, rec32b)
    enc.set_precision("bf16")
    got = [_rec(p) for _ in range(3)]                    # capture again (never the fp32 graph), replay, replay
    (q,) = _members(dev, sph, enc, SPECS[:1], use_graph=False)
    rec16, out16 = _rec(q)                               # eager
    for r, o in got:
        assert np.array_equal(r, rec16) and np.array_equal(o, out16)
    assert not np.array_equal(out16, out32)             # the switch really changed the arithmetic
    enc.set_precision("fp32")
    back = [_rec(p) for _ in range(2)]
    fresh = make_encoder(sd, dev)
    (f,) = _members(dev, sph, fresh, SPECS[:1])
    recf, outf = _rec(f)
    assert np.array_equal(recf, rec32) and np.array_equal(outf, out32)
    for r, o in back:
        assert np.array_equal(r, rec32) and np.array_equal(o, out32)
    # check_weights=False looks at no image: the precision alone must keep the stale graph from replaying
    enc.set_precision("bf16")
    p.run(check_weights=False)
    assert np.array_equal(p.ws.rec.cpu().numpy(), rec16)


@pytest.mark.parametrize("full_first", [False, True])
def test_pose_chain_replay_equals_eager(golden, dev, full_first):
    sph = golden("sphere.npz")["pts"]
    enc = make_encoder(seeded_sd(0, 4.0), dev).set_precision("bf16")
    pipes = _members(dev, sph, enc, SPECS)
    chain = PoseChain(pipes)
    chain.full_first = full_first
    recs = torch.zeros((3, 21), dtype=torch.float64, device=dev)
    chain.run_async(list(recs), eager=True)
    torch.cuda.synchronize()
    want = recs.cpu().numpy().copy()
    for rep in range(3):
        recs.zero_()
        chain.run_async(list(recs))
        torch.cuda.synchronize()
        assert np.array_equal(recs.cpu().numpy(), want), rep
    for j, p in enumerate(pipes):                        # and the chain's member records are the members' own pipelines'
        p.adapt(p.idx.shape[0] if full_first else 0)
        p.run()
        assert np.array_equal(p.ws.rec.cpu().numpy(), want[j]), j
    # fp32 -> the fp32 chain's records are those of a chain that never saw bf16
    enc.set_precision("fp32")
    chain.run_async(list(recs))
    torch.cuda.synchronize()
    got32 = recs.cpu().numpy().copy()
    fresh = PoseChain(_members(dev, sph, make_encoder(seeded_sd(0, 4.0), dev), SPECS))
    fresh.full_first = full_first
    recs2 = torch.zeros((3, 21), dtype=torch.float64, device=dev)
    fresh.run_async(list(recs2))
    torch.cuda.synchronize()
    assert np.array_equal(got32, recs2.cpu().numpy())
    assert not np.array_equal(got32, want)


def test_batch_runner_replay_equals_eager(dev):
    from cppf_amd.batch import BatchPoseRunner
    from cppf_amd.config import NOCS_CATEGORIES
    sd = seeded_sd(0, 4.0)
    objects = []
    for j in range(4):
        ob = syn.make_object(NOCS_CATEGORIES[j % 6], 600 + 50 * j, 400 + j)
        idx = syn.make_pairs(ob["pc"].shape[0], 24, 400 + j)
        u_tr, u_rot = syn.make_uniforms(idx.shape[0], 400 + j)
        objects.append(dict(pc=ob["pc"], normals=ob["normals"], feat=ob["feat"], point_idxs=idx, u_tr=u_tr, u_rot=u_rot, cfg=ob["cfg"]))
    encs = {c: make_encoder(sd, dev).set_precision("bf16") for c in NOCS_CATEGORIES}
    eager = BatchPoseRunner(encs, dev, use_graph=False, chain_len=1)
    want = eager.run(objects).cpu().numpy()
    runner = BatchPoseRunner(encs, dev, chain_len=2)
    for rep in range(3):                                 # solo graphs, chains captured, chains replayed
        np.testing.assert_array_equal(runner.run(objects).cpu().numpy(), want)
    assert runner._chains
    for e in encs.values():
        e.set_precision("fp32")
    got32 = runner.run(objects).cpu().numpy()
    got32b = runner.run(objects).cpu().numpy()
    fresh = BatchPoseRunner({c: make_encoder(sd, dev) for c in NOCS_CATEGORIES}, dev, chain_len=2)
    want32 = fresh.run(objects).cpu().numpy()
    np.testing.assert_array_equal(got32, want32)
    np.testing.assert_array_equal(got32b, want32)
    assert not np.array_equal(want32, want)


# ------------------------------------------------------------------------------------------------ 7. poses
def _med(errs, key):
    return float(np.median([e[key] for e in errs]))


@pytest.mark.parametrize("cat", ["bottle", "mug", "laptop"])
def test_committed_trained_weights_recover_held_out_poses_under_bf16(dev, cat):
    """tests/test_gpu_trained.py::test_committed_trained_weights_recover_held_out_poses with the pair encoder in bf16: the same
    networks, the same held-out objects, the same thresholds"""
    from test_gpu_trained import _held_out
    cfg = syn.CATEGORIES[cat]
    penc, enc = training.load_weights(os.path.join(GOLDEN, f"trained_{cat}.npz"), cfg, dev)
    keys = ("t_cells", "up_deg_mod_sign", "scale_rel") + (("right_deg_mod_sign",) if cfg.regress_right else ())
    errs32 = _held_out(penc, enc, cat, dev)
    errs = _held_out(penc, enc.set_precision("bf16"), cat, dev)
    print(cat, "medians fp32 | bf16:", {k: (round(_med(errs32, k), 3), round(_med(errs, k), 3)) for k in keys},
          "min survivors", min(e["n_surv"] for e in errs32), "|", min(e["n_surv"] for e in errs))
    assert _med(errs, "t_cells") <= 2.0 and max(e["t_cells"] for e in errs) <= 4.0, errs
    assert _med(errs, "up_deg_mod_sign") <= 5.0 and max(e["up_deg_mod_sign"] for e in errs) <= 12.0, errs
    assert _med(errs, "scale_rel") <= 0.10 and max(e["scale_rel"] for e in errs) <= 0.2, errs
    if cat == "bottle":
        assert sum(e["up_deg"] < 15 for e in errs) >= len(errs) - 1, errs
    if cfg.regress_right:
        assert _med(errs, "right_deg_mod_sign") <= 10.0, errs
    assert min(e["n_surv"] for e in errs) > 0.05 * 100000


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(golden, dev):
    c = cases.case("random")
    pc, nrm, feat = dev_inputs(c, dev)
    idx = torch.from_numpy(c["idxs"][:64]).to(dev)
    u_tr, u_rot = _uniforms(64, 1, dev)
    e16, e32 = enc_of(c["sd"], dev, "bf16"), enc_of(c["sd"], dev, "fp32")
    item = lambda e: dict(encoder=e, pc=pc, pc_normal=nrm, feat=feat, idxs=idx, u_tr=u_tr, u_rot=u_rot, vote_range=c["cfg"].vote_range)
    with pytest.raises(_lib.CppfError, match="fp32.*bf16|bf16.*fp32"):
        forward_decode_batch([item(e32), item(e16)])
    # gradients: training mode, and inputs that require grad; eval + no such input is inference even with autograd on
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16.train()(pc[None], nrm[None], feat[None], idxs=idx)
    e16.eval()
    with pytest.raises(_lib.CppfError, match="inference only"):
        e16.forward_with_idx(pc, nrm, feat.clone().requires_grad_(True), idx)
    out = e16.forward_with_idx(pc, nrm, feat, idx)
    assert out.shape == (64, 141) and not out.requires_grad
    # other architectures: refused, never served in fp32 behind the caller's back
    with pytest.raises(_lib.CppfError, match="bf16"):
        PPFEncoder([84, 64, 64, 16], 141).to(dev).set_precision("bf16")
    dims = (C.c_int * 4)(84, 64, 64, 16)
    arr = (_lib.PairMlpItem * 1)()
    assert call("cppf_pair_mlp_bf16_decode_batch", dev, 1, arr, 40, dims, 3, 141, 32, 36, ok=(_lib.EUNSUPPORTED,)) == _lib.EUNSUPPORTED
    std = (C.c_int * 4)(*STD)
    assert call("cppf_pair_mlp_bf16_decode_batch", dev, 1, arr, 40, std, 3, 141, 32, 30, ok=(_lib.EUNSUPPORTED,)) == _lib.EUNSUPPORTED
    assert call("cppf_pair_mlp_bf16_decode_sel_batch", dev, 1, arr, 40, std, 3, 100, 32, 36, ok=(_lib.EUNSUPPORTED,)) == _lib.EUNSUPPORTED
    assert call("cppf_pair_mlp_bf16_decode_batch", dev, 1, arr, 40, std, 3, 141, 32, 36) == 0          # P = 0: a no-op
    # a short workspace
    from cppf_amd._torch_util import fill, scratch
    outputs = torch.empty((64, 2), dtype=torch.float32, device=dev)
    small = torch.empty(256, dtype=torch.uint8, device=dev)
    fill(arr[0], dev, pc=pc, nrm=nrm, feat=feat, idxs=idx, packed=e16._packed_weights(dev), u_tr=u_tr, outputs=outputs,
         workspace=scratch(small), n_points=pc.shape[0], n_pairs=64, vr0=1.0, vr1=1.0, idx_is_i64=True)
    assert call("cppf_pair_mlp_bf16_decode_batch", dev, 1, arr, 40, std, 3, 141, 32, 36, ok=(-2,)) == -2   # CPPF_EWORKSPACE
    # second_pass 1 and 2 in one pose-tail batch
    sph = golden("sphere.npz")["pts"]
    enc_a, enc_b = make_encoder(seeded_sd(0, 4.0), dev), make_encoder(seeded_sd(0, 4.0), dev).set_precision("bf16")
    pa = _members(dev, sph, enc_a, SPECS[:1])
    pb = _members(dev, sph, enc_b, SPECS[1:2])
    with pytest.raises(_lib.CppfError, match="precision"):
        PoseChain(pa + pb).run_async(None, eager=True)
    tail = (_lib.PoseTailItem * 2)()
    dummy = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)          # (passes every size check: the refusal is the mix's)
    for k, sp in enumerate((1, 2)):
        fill(tail[k], dev, **{f: dummy for f in ("pc", "nrm", "feat", "idx32", "outputs", "u_rot", "heads", "corner", "argmax_idx", "rec", "T32",
                                                 "mask", "chunk_counts", "surv", "count", "counts", "ticket", "packed")},
             mlp_workspace=scratch(dummy), sums_workspace=scratch(dummy), tail0=scratch(dummy), n_points=8, n_pairs=16, res64=0.1, res=0.1,
             tol=0.3, gx=4, gy=4, gz=4, n_dirs=1, second_pass=sp)
    sph32 = torch.from_numpy(sph.astype(np.float32)).to(dev)
    sph64 = torch.from_numpy(sph).to(dev)
    rc = call("cppf_pose_tail_batch", dev, 2, tail, 40, std, 3, 141, 32, 36, 72, sph32, sph64, sph.shape[0], 1, 0.9, 100, ok=(-1,))
    assert rc == -1                                      # CPPF_EINVAL, before anything is launched
