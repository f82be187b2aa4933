"""The back-vote's two shortcuts at their edges, on the device: every form of backvote_body (csrc/pose_tail.hip) and
backvote_multi_kernel (csrc/scene_multi.hip) on the boundary family of tests/backvote_cases.py, bit for bit against oracle.backvote --
the exhaustive loop that tests/test_ref_vote_cpu.py pins on the reference's executed text.  The device must equal the oracle, never
the other way round: a mask bit that differs is a shortcut that is no superset (csrc/backvote_common.h), a wrong offset among
survivors is a wrong winner among several passing rotations.

tests/test_backvote_cases_cpu.py proves, with no GPU, that these inputs sit where a margin-free screen or arc loses pairs.  What the
device's v_sqrt / v_rcp / acos_approx / atan2_approx take out of the margins is measured here; the figures (pytest -s) are in
DESIGN.md, "Back-vote at its edges".
"""
import functools

import numpy as np
import pytest
import torch

import backvote_cases as BC
from cppf_amd import _lib, scene_stage
from cppf_amd._torch_util import stream_ptr, workspace
from cppf_amd.models import voting

pytestmark = pytest.mark.gpu
F = np.float32
IDS = [f"gt{BC.CENTRES.index(g)}-res{r:g}-rots{n}" for g, r, n in BC.CONFIGS]
VOTE_TAB_STAMP = 0x43505046726F7400          # csrc/vote_common.h


@functools.lru_cache(maxsize=None)
def truth(cfg):
    from oracle import oracle as O
    c = BC.family(*cfg)
    oo, mask = O.backvote(c["points"], c["outputs"], c["idx"], c["corner"], c["res"], c["n_rots"], c["dims"], c["gt"], F(c["tol"]))
    return c, oo, mask


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Dev:
    """a case's arrays on the device (named: a temporary's data_ptr() dangles once it is freed)"""

    def __init__(self, c, dev, gt=None):
        self.dev, self.c, self.P = dev, c, c["idx"].shape[0]
        self.pts, self.out, self.idx, self.cor = (t(c[k], dev) for k in ("points", "outputs", "idx", "corner"))
        self.gt = t(c["gt"] if gt is None else np.asarray(gt, F), dev)
        self.dims = tuple(int(d) for d in c["dims"])
        self.shape = t(np.array([c["points"].shape[0], *self.dims], np.int32), dev)
        self.n_chunks = (self.P + 1023) // 1024

    def head(self):
        return self.pts.data_ptr(), self.out.data_ptr()

    def tail(self):
        return self.gt.data_ptr(), float(F(self.c["tol"]))


def chunk_sums(mask):
    n = (mask.size + 1023) // 1024
    pad = np.zeros(n * 1024, np.int64)
    pad[:mask.size] = mask
    return pad.reshape(n, 1024).sum(1)


def mask_ws(d, vote_ws=None):
    """cppf_backvote_ws, mask only"""
    L, c = _lib.lib(), d.c
    m = torch.full((d.P,), 7, dtype=torch.uint8, device=d.dev)
    _lib.check(L.cppf_backvote_ws(*d.head(), None, d.idx.data_ptr(), d.cor.data_ptr(), c["res"], d.P, c["n_rots"], *d.dims, None, *d.tail(),
                                  m.data_ptr(), None if vote_ws is None else vote_ws.data_ptr(), stream_ptr(d.dev)), "backvote_ws")
    return m.cpu().numpy()


def counted(d, form):
    """cppf_backvote_count (int32 list) / cppf_backvote_count64 (int64 list), then cppf_compact_scatter -> mask, chunk counts, survivors"""
    L, c = _lib.lib(), d.c
    m = torch.full((d.P,), 7, dtype=torch.uint8, device=d.dev)
    cc = torch.zeros(d.n_chunks, dtype=torch.int32, device=d.dev)
    surv = torch.full((d.P,), -1, dtype=torch.int32, device=d.dev)
    cnt = torch.full((1,), -5, dtype=torch.int32, device=d.dev)
    if form == "count":
        _lib.check(L.cppf_backvote_count(*d.head(), d.idx.data_ptr(), d.cor.data_ptr(), c["res"], d.P, c["n_rots"], *d.dims, None, *d.tail(),
                                         m.data_ptr(), cc.data_ptr(), None, stream_ptr(d.dev)), "backvote_count")
    else:
        idx64, idx32 = d.idx.to(torch.int64), torch.full((d.P, 2), -1, dtype=torch.int32, device=d.dev)
        _lib.check(L.cppf_backvote_count64(*d.head(), idx64.data_ptr(), idx32.data_ptr(), d.cor.data_ptr(), c["res"], d.P, c["n_rots"], 1, 1, 1,
                                           d.shape.data_ptr(), *d.tail(), m.data_ptr(), cc.data_ptr(), None, stream_ptr(d.dev)),
                   "backvote_count64")
        torch.cuda.synchronize()
        assert torch.equal(idx32, d.idx)
    _lib.check(L.cppf_compact_scatter(m.data_ptr(), d.P, cc.data_ptr(), surv.data_ptr(), cnt.data_ptr(), stream_ptr(d.dev)), "compact_scatter")
    torch.cuda.synchronize()
    return m.cpu().numpy(), cc.cpu().numpy(), surv.cpu().numpy()[:int(cnt.item())]


def check_counted(got, mask, what):
    m, cc, surv = got
    np.testing.assert_array_equal(m.astype(bool), mask, err_msg=what)
    assert m.max() <= 1
    np.testing.assert_array_equal(cc, chunk_sums(mask), err_msg=what)
    np.testing.assert_array_equal(surv, np.nonzero(mask)[0], err_msg=what)


def figures(cfg, c, mask):
    """survivors, how close to tol the loop's own decisions come (fp64 of its fp32 distances), and the arc's length"""
    from oracle import oracle as O
    passing, dist, fr = BC.exhaustive(O, c)
    tol = float(F(c["tol"]))
    near = dist.astype(np.float64).min(1)
    acc = np.abs(np.where(passing, dist, np.inf).astype(np.float64).min(1)[mask] - tol).min() / tol
    rej = np.abs(near[~mask & np.isfinite(near)] - tol).min() / tol
    _, cnt = BC.arc(c, fr)
    print(f"[{cfg}] pairs {mask.size}, survivors {int(mask.sum())}, smallest |dist - tol| / tol: accepted {acc:.2e}, rejected {rej:.2e}; "
          f"largest arc {int(cnt[cnt < fr['nr']].max())} of {c['n_rots']} rotations")


@pytest.mark.parametrize("cfg", BC.CONFIGS, ids=IDS)
def test_offsets_and_every_mask_form_equal_the_oracle(dev, cfg):
    c, oo, mask = truth(cfg)
    figures(cfg, c, mask)
    d = Dev(c, dev)
    # the drop-in (voting.backvote_kernel = cppf_backvote): offsets bit for bit -- the winner among several passing rotations
    offs = torch.zeros((d.P, 3), dtype=torch.float32, device=dev)
    voting.backvote_kernel(((d.P + 511) // 512, 1, 1), (512, 1, 1),
                           (d.pts, d.out, offs, d.idx, d.cor, F(c["res"]), d.P, c["n_rots"], *d.dims, d.gt, F(c["tol"])))
    torch.cuda.synchronize()
    got = offs.cpu().numpy()
    wrong = np.nonzero((got != oo).any(1))[0]
    assert wrong.size == 0, (f"{wrong.size} pairs differ, of them {int((got[wrong].any(1) != mask[wrong]).sum())} in the mask; first: pair "
                             f"{wrong[0]}, group {BC.GROUP_NAMES[c['group'][wrong[0]]]}, eps {c['eps'][wrong[0]]}, n {c['n'][wrong[0]]}, "
                             f"device {got[wrong[0]]}, oracle {oo[wrong[0]]}")
    # mask only; mask + chunk counts from the int32 and the int64 list (dims by value / in a device record); cppf_backvote_dyn
    np.testing.assert_array_equal(mask_ws(d).astype(bool), mask)
    check_counted(counted(d, "count"), mask, "cppf_backvote_count")
    check_counted(counted(d, "count64"), mask, "cppf_backvote_count64")
    L = _lib.lib()
    m = torch.full((d.P,), 7, dtype=torch.uint8, device=dev)
    offs.zero_()
    _lib.check(L.cppf_backvote_dyn(*d.head(), offs.data_ptr(), d.idx.data_ptr(), d.cor.data_ptr(), c["res"], d.P, c["n_rots"],
                                   d.shape.data_ptr(), *d.tail(), m.data_ptr(), stream_ptr(dev)), "backvote_dyn")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(offs.cpu().numpy(), oo)
    np.testing.assert_array_equal(m.cpu().numpy().astype(bool), mask)


@pytest.mark.parametrize("n_rots", BC.ROTATIONS)
def test_rotation_table_from_a_stamped_workspace_gives_the_same_bits(dev, n_rots):
    """The table loaded from the workspace that vote_argmax of the same n_rots has just stamped (bv_load_rot_table), and the table
    built in LDS: the same mask, the oracle's.  (120 rotations keep no table: both runs take rot_cs.)"""
    cfg = ((0.1, -0.05, 0.7), 4e-3, n_rots)
    c, oo, mask = truth(cfg)
    d = Dev(c, dev)
    pc = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], F)
    idx = np.array([[1, 0], [2, 0], [3, 0], [1, 2]], np.int32)
    out = np.array([[0.1, 0.05], [0.1, 0.003], [0.0, 0.01], [0.05, 0.25]], F)
    grid = torch.zeros((20, 20, 20), dtype=torch.float32, device=dev)
    voting.vote_argmax(t(pc, dev), t(out, dev), None, t(idx, dev), grid, t(np.array([-0.2, -0.2, -0.2], F), dev), 0.02, n_rots, True,
                       accumulate=False)
    torch.cuda.synchronize()
    ws = workspace(256, dev, "vote")                                   # the buffer that vote has just used
    assert ws.numel() >= 1 << 16
    stamp = int(ws[248:256].view(torch.int64).item())
    if n_rots <= 72:
        assert stamp == VOTE_TAB_STAMP ^ n_rots
    with_ws, without = mask_ws(d, ws), mask_ws(d)
    np.testing.assert_array_equal(with_ws, without)
    np.testing.assert_array_equal(with_ws.astype(bool), mask)


@functools.lru_cache(maxsize=None)
def multi_truth(cfg):
    from oracle import oracle as O
    c, _, _ = truth(cfg)
    cs = BC.centres(c)
    bits = np.zeros(c["idx"].shape[0], np.uint32)
    for k in range(32):
        _, m = O.backvote(c["points"], c["outputs"], c["idx"], c["corner"], c["res"], c["n_rots"], c["dims"], cs[k], F(c["tol"]))
        bits |= m.astype(np.uint32) << np.uint32(k)
    return cs, bits


@pytest.mark.parametrize("cfg", BC.CONFIGS, ids=IDS)
def test_multi_bits_equal_the_oracle_and_the_single_centre_kernel(dev, cfg):
    """bit k of cppf_backvote_multi = the oracle's mask at centre k = cppf_backvote_ws at centre k: the two copies of the stage-1
    screen agree with the truth on the same inputs, at 1, 5 and 32 centres"""
    c, _, mask = truth(cfg)
    cs, want = multi_truth(cfg)
    assert np.array_equal((want & 1).astype(bool), mask)
    d = Dev(c, dev)
    d_cs = t(cs, dev)
    for K in (1, 5, 32):
        bits = scene_stage.backvote_multi(d.pts, d.out, d.idx, d.cor, c["res"], d.dims, d_cs[:K], c["n_rots"], float(F(c["tol"])))
        torch.cuda.synchronize()
        got = bits.cpu().numpy().view(np.uint32)
        keep = np.uint32((1 << K) - 1) if K < 32 else np.uint32(0xFFFFFFFF)
        diff = got ^ (want & keep)
        bad = np.nonzero(diff)[0]
        assert bad.size == 0, f"K = {K}: {bad.size} pairs differ; first: pair {bad[0]}, device {got[bad[0]]:#x}, oracle {want[bad[0]] & keep:#x}"
    single = np.zeros(d.P, np.uint32)
    for k in range(32):
        single |= mask_ws(Dev(c, dev, cs[k])).astype(np.uint32) << np.uint32(k)
    np.testing.assert_array_equal(single, want)
    print(f"[{cfg}] survivors per centre: {[int(((want >> np.uint32(k)) & 1).sum()) for k in range(32)]}")


@pytest.mark.parametrize("order", ["shuffled", "by-eps"])
@pytest.mark.parametrize("cfg", [BC.CONFIGS[4], BC.CONFIGS[0], BC.CONFIGS[16]], ids=[IDS[4], IDS[0], IDS[16]])
def test_list_order_shuffled_and_sorted_by_eps(dev, cfg, order):
    """The per-wave queue (bv_push, drained at 64) sees waves in which nearly every lane passes stage 1 and waves in which one does
    (sorted by eps: the classes lie together), and a mixture (shuffled)"""
    c, oo, mask = truth(cfg)
    if order == "shuffled":
        perm = np.random.default_rng(5).permutation(mask.size)
    else:
        perm = np.argsort(np.where(np.isnan(c["eps"]), 1.0, c["eps"]), kind="stable")
    cp = BC.reorder(c, perm)
    d = Dev(cp, dev)
    check_counted(counted(d, "count"), mask[perm], order)
    offs = torch.zeros((d.P, 3), dtype=torch.float32, device=dev)
    voting.backvote_kernel(((d.P + 511) // 512, 1, 1), (512, 1, 1),
                           (d.pts, d.out, offs, d.idx, d.cor, F(c["res"]), d.P, c["n_rots"], *d.dims, d.gt, F(c["tol"])))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(offs.cpu().numpy(), oo[perm])
    cs, want = multi_truth(cfg)
    bits = scene_stage.backvote_multi(d.pts, d.out, d.idx, d.cor, c["res"], d.dims, t(cs, dev), c["n_rots"], float(F(c["tol"])))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), want[perm])
