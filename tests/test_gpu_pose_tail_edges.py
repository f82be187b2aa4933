"""The pose tail's reductions and its bin arg-max at their trips, ties and ends (csrc/pose_tail.hip: pose_sums_kernel,
axis_sign_kernel, scale_sum_kernel<EXP>, reduce_final_kernel, counts_argmax_select_kernel), on the inputs of tests/pose_tail_cases.py.

Every kernel strides by RED_BLOCKS * RED_THREADS = 65 536 and pose_sums_body loads a thread's first pair before the arg-max and
reloads on later trips; the sizes run from nothing through one ragged block, one full trip, its ragged end and a third trip.  Each
size is reached through the device count (with the full list's length as the host bound) and through the host count alone, with
sel = NULL (identity) and with sel a shuffled permutation of the same rows: the kernels promise sums, not an order.

Reference: a float64 restatement of nocs/inference.py:287-301,335 (pose_tail_cases.bce_terms), summed by math.fsum.
Tolerance, derived and not measured: any summation order of n fp64 terms is off by at most n 2^-53 sum|term|; exactly that, per
component.  The scale logits are integers: their sums are exact in fp64 in any order, and equality is demanded.  The sums of
expf(logit) get the same bound plus one fp32 ulp per term, 2^-23 sum|term|: the device's expf is the only fp32 operation in them.
"""
import math

import numpy as np
import pytest
import torch

import pose_tail_cases as PC
from cppf_amd import _lib
from cppf_amd._torch_util import stream_ptr
from cppf_amd.utils.util import fibonacci_sphere

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
BIN0, BIN1, N_SPHERE = 5, 300, 480


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def tail(dev):
    pc, nrm = PC.cloud()
    idx, heads = PC.pairs()
    sph = np.array(fibonacci_sphere(N_SPHERE), D)
    sph[BIN0] = (0.0, 1.0, 0.0)                                             # exact: normals orthogonal to it give proj == 0
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 50, (2, N_SPHERE)).astype(np.int32)
    counts[0, BIN0], counts[1, BIN1] = 60, 61
    terms = [PC.bce_terms(pc, nrm, idx, heads[:, 2 + j], sph[b]) for j, b in enumerate((BIN0, BIN1))]
    # the exact rows reach their comparisons with zero: d == 0 without a flip, proj == 0 with target 0
    rows = np.arange(0, PC.PAIRS, 97)
    n_fl, d = PC.flipped_normals(pc, nrm, idx[rows])
    d_all = PC.flipped_normals(pc, nrm, idx[:5000])[1]
    assert (d == 0).sum() >= 0.5 * rows.size and (d_all < 0).sum() > 1000 and (d_all > 0).sum() > 1000
    assert np.array_equal(n_fl[d == 0], nrm[idx[rows, 0]][d == 0])
    proj0 = n_fl.astype(D) @ sph[BIN0]
    assert ((proj0 == 0) & (terms[0][2][rows] == 0)).sum() >= 0.2 * rows.size and (proj0 > 0).any() and (proj0 < 0).any()
    L = _lib.lib()
    ns = dict(pc=pc, nrm=nrm, idx=idx, heads=heads, sph=sph, counts=counts, terms=terms, L=L, dev=dev,
              d_pc=t(pc, dev), d_nrm=t(nrm, dev), d_idx=t(idx, dev), d_heads=t(heads, dev), d_sph=t(sph, dev), d_counts=t(counts, dev),
              ws=torch.empty(int(L.cppf_pose_sums_workspace_bytes()), dtype=torch.uint8, device=dev),
              ws_red=torch.empty(int(L.cppf_reduce_workspace_bytes()), dtype=torch.uint8, device=dev))
    return ns


def selections(n, dev):
    """(name, sel tensor or None): identity, and the same rows shuffled"""
    perm = np.random.default_rng(n).permutation(n).astype(np.int32)
    return [("identity", None), ("shuffled", t(perm if n else np.zeros(1, np.int32), dev))]


def counts_forms(n, dev):
    """(name, n_sel_dev tensor or None, n_sel_host): the device count under the full list's bound; the host count alone"""
    return [("device", torch.tensor([n], dtype=torch.int32, device=dev), PC.PAIRS), ("host", None, n)]


def ptr(x):
    return None if x is None else x.data_ptr()


def want_sums(tail, n):
    """per direction (up, down) and per scale column: (exact sum, bound)"""
    sign = [[PC.fsum_bound(tail["terms"][j][k][:n]) for k in (0, 1)] for j in (0, 1)]
    scale = [float(tail["heads"][:n, 4 + c].astype(D).sum()) for c in range(3)]
    return sign, scale


@pytest.mark.parametrize("n", PC.SIZES)
def test_pose_sums_at_every_trip(tail, dev, n):
    L = tail["L"]
    sign_w, scale_w = want_sums(tail, n)
    for n_dirs in (1, 2):
        for cname, n_dev, n_host in counts_forms(n, dev):
            for sname, sel in selections(n, dev):
                what = f"n_sel {n}, n_dirs {n_dirs}, {cname} count, {sname} sel"
                best_idx = torch.full((2,), -1, dtype=torch.int64, device=dev)
                best_dir = torch.full((2, 3), 9.0, dtype=torch.float64, device=dev)
                sign = torch.full((2, 3), 9.0, dtype=torch.float64, device=dev)
                scale = torch.full((4,), 9.0, dtype=torch.float64, device=dev)
                ticket = torch.zeros(4, dtype=torch.int32, device=dev)
                runs = []
                for _ in range(2):                                          # the ticket is left at 0: a second call, the same bits
                    _lib.check(L.cppf_pose_sums(ptr(tail["d_pc"]), ptr(tail["d_nrm"]), ptr(tail["d_idx"]), ptr(sel), ptr(n_dev), n_host,
                                                tail["d_heads"].data_ptr() + 8, 8, n_dirs, ptr(tail["d_counts"]), N_SPHERE, N_SPHERE,
                                                ptr(tail["d_sph"]), tail["d_heads"].data_ptr() + 16, 8, ptr(best_idx), ptr(best_dir),
                                                ptr(sign), ptr(scale), ptr(tail["ws"]), tail["ws"].numel(), ptr(ticket), stream_ptr(dev)),
                               "pose_sums")
                    torch.cuda.synchronize()
                    assert int(ticket[0].item()) == 0, what
                    runs.append([x.cpu().numpy().copy() for x in (best_idx, best_dir, sign, scale)])
                for a, b in zip(*runs):
                    assert a.tobytes() == b.tobytes(), what
                bi, bd, sg, sc = runs[0]
                for j, b in enumerate((BIN0, BIN1)[:n_dirs]):
                    assert bi[j] == b and bd[j].tobytes() == tail["sph"][b].tobytes(), what
                    for k in (0, 1):
                        want, bound = sign_w[j][k]
                        print(f"{what}: direction {j} {'up' if k == 0 else 'down'} sum {sg[j, k]!r}, off by {abs(sg[j, k] - want):.3e}, bound {bound:.3e}")
                        assert np.isfinite(sg[j, k]) and abs(sg[j, k] - want) <= bound, (what, j, k, sg[j, k], want, bound)
                    assert sg[j, 2] == n, what
                if n_dirs == 1:                                             # the second direction's outputs are not touched
                    assert bi[1] == -1 and (bd[1] == 9.0).all() and (sg[1] == 9.0).all(), what
                assert sc[3] == n and list(sc[:3]) == scale_w, (what, sc, scale_w)
                if n == 0:
                    assert not sg[:n_dirs, :2].any() and not sc[:3].any(), what
                if n == 1:                                                  # the -1e4 row (target 1): 0 + 1e4 and 0, nothing else
                    assert list(sg[0, :2]) == [1e4, 0.0], sg[0]


@pytest.mark.parametrize("n", PC.SIZES)
def test_axis_sign_and_scale_sums_at_every_trip(tail, dev, n):
    L = tail["L"]
    sign_w, scale_w = want_sums(tail, n)
    ex = np.exp(tail["heads"][:n, 4:7].astype(D)).astype(F).astype(D)       # fp32 exp of each logit, as float64 terms
    ws = tail["ws_red"]
    for cname, n_dev, n_host in counts_forms(n, dev):
        for sname, sel in selections(n, dev):
            what = f"n_sel {n}, {cname} count, {sname} sel"
            for j, b in enumerate((BIN0, BIN1)):
                out = torch.full((3,), 9.0, dtype=torch.float64, device=dev)
                bd = t(tail["sph"][b], dev)
                _lib.check(L.cppf_axis_sign(ptr(tail["d_pc"]), ptr(tail["d_nrm"]), ptr(tail["d_idx"]), ptr(sel), ptr(n_dev), n_host,
                                            tail["d_heads"].data_ptr() + 8 + 4 * j, 8, ptr(bd), ptr(out), ptr(ws), ws.numel(), stream_ptr(dev)),
                           "axis_sign")
                o = out.cpu().numpy()
                for k in (0, 1):
                    want, bound = sign_w[j][k]
                    assert np.isfinite(o[k]) and abs(o[k] - want) <= bound, (what, j, k, o[k], want, bound)
                assert o[2] == n, what
            out4 = torch.full((4,), 9.0, dtype=torch.float64, device=dev)
            _lib.check(L.cppf_scale_sum(tail["d_heads"].data_ptr() + 16, 8, ptr(sel), ptr(n_dev), n_host, ptr(out4), ptr(ws), ws.numel(),
                                        stream_ptr(dev)), "scale_sum")
            o4 = out4.cpu().numpy()
            assert o4[3] == n and list(o4[:3]) == scale_w, (what, o4, scale_w)
            out4.fill_(9.0)
            _lib.check(L.cppf_scale_exp_sum(tail["d_heads"].data_ptr() + 16, 8, ptr(sel), ptr(n_dev), n_host, ptr(out4), ptr(ws), ws.numel(),
                                            stream_ptr(dev)), "scale_exp_sum")
            o4 = out4.cpu().numpy()
            assert o4[3] == n, what
            for c in range(3):
                want, bound = PC.fsum_bound(ex[:, c])
                bound += 2.0 ** -23 * math.fsum(ex[:, c])
                assert abs(o4[c] - want) <= bound, (what, c, o4[c], want, bound)


def argmax_cases(S):
    """(name, counts i32[S], winner): the maximum at the ends, at the wave and block-stride seams, tied across waves and strides"""
    rng = np.random.default_rng(S)
    base = rng.integers(0, 1000, S).astype(np.int32)
    out = [("all zero", np.zeros(S, np.int32), 0)]
    for i in (0, S - 1, 63, 64, 255, 256):
        if i < S:
            c = base.copy()
            c[i] = 5000
            out.append((f"maximum at {i}", c, i))
    for lo, hi in ((10, 70), (5, 5 + 256), (63, 64), (255, 256), (0, S - 1)):       # other wave; other stride of the same thread; seams
        if hi < S and lo != hi:
            c = base.copy()
            c[lo] = c[hi] = 7000
            out.append((f"tie at {lo} and {hi}", c, lo))
    c = base.copy()
    c[S // 2] = 2 ** 31 - 1
    out.append(("a count of 2^31 - 1", c, S // 2))
    c = np.full(S, 2 ** 31 - 1, np.int32)
    out.append(("every count 2^31 - 1", c, 0))
    return out


@pytest.mark.parametrize("S", [1, 255, 256, 257, 423, 480, 4096])
def test_bin_argmax_ties_and_ends(tail, dev, S):
    """counts_argmax_select_kernel and the arg-max inside pose_sums_body: np.argmax's first maximum, best_dir the bits of
    sphere64[best]; the second direction's row lies counts_dir_step > n_sphere further on, with poison between the rows"""
    L = tail["L"]
    sph = np.random.default_rng(S + 1).normal(size=(S, 3))
    d_sph = t(sph, dev)
    cases = argmax_cases(S)
    step = S + 37
    for k, (name, c0, win0) in enumerate(cases):
        _, c1, win1 = cases[(k + 1) % len(cases)]
        assert win0 == int(np.argmax(c0)) and win1 == int(np.argmax(c1))
        rows = np.full(2 * step, 2 ** 31 - 1, np.int32)                      # poison: it would win wherever it is read
        rows[:S], rows[step:step + S] = c0, c1
        d_rows = t(rows, dev)
        bi = torch.full((1,), -1, dtype=torch.int64, device=dev)
        bd = torch.full((3,), 9.0, dtype=torch.float64, device=dev)
        _lib.check(L.cppf_counts_argmax_select(ptr(d_rows), S, ptr(d_sph), ptr(bi), ptr(bd), stream_ptr(dev)), "counts_argmax_select")
        assert int(bi.item()) == win0 and bd.cpu().numpy().tobytes() == sph[win0].tobytes(), (S, name)
        best_idx = torch.full((2,), -1, dtype=torch.int64, device=dev)
        best_dir = torch.full((2, 3), 9.0, dtype=torch.float64, device=dev)
        sign = torch.full((2, 3), 9.0, dtype=torch.float64, device=dev)
        ticket = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(L.cppf_pose_sums(ptr(tail["d_pc"]), ptr(tail["d_nrm"]), ptr(tail["d_idx"]), None, None, 300,
                                    tail["d_heads"].data_ptr() + 8, 8, 2, ptr(d_rows), S, step, ptr(d_sph), None, 0, ptr(best_idx),
                                    ptr(best_dir), ptr(sign), None, ptr(tail["ws"]), tail["ws"].numel(), ptr(ticket), stream_ptr(dev)),
                   "pose_sums")
        torch.cuda.synchronize()
        assert best_idx.cpu().tolist() == [win0, win1], (S, name)
        assert best_dir.cpu().numpy().tobytes() == sph[[win0, win1]].tobytes(), (S, name)
        assert int(ticket[0].item()) == 0 and (sign.cpu().numpy()[:, 2] == 300).all()


# ------------------------------------------------------------------ the record assembled on the device
S_TAIL = 64
UP_BIN, NEG_BIN, RIGHT_BIN = 31, 32, 9           # (1, 0, 0), (-1, 0, 0), (1, 1, 0) / sqrt(2) in tail_sphere()
SCALE_MEAN = (0.06, 0.05, 0.045)
# n_pairs, n_dirs, regress_right, flip of up, flip of right, r1 (dir 1's rotation head), survivors, arg-max given, object id on the device
ITEMS = [dict(n=1, n_dirs=2, rr=1, flips=(0, 0), r1=np.pi / 4, name="one pair, no flip"),
         dict(n=1023, n_dirs=2, rr=1, flips=(1, 0), r1=np.pi / 4, name="flip of up only", id_dev=True),
         dict(n=1025, n_dirs=2, rr=1, flips=(0, 1), r1=np.pi / 4, name="flip of right only"),
         dict(n=4100, n_dirs=2, rr=1, flips=(1, 1), r1=np.pi / 4, name="both flipped", id_dev=True),
         dict(n=300, n_dirs=1, rr=0, flips=(0, 0), r1=0.0, name="right derived from up = (1, 0, 0): degenerate"),
         dict(n=300, n_dirs=2, rr=0, flips=(1, 0), r1=np.pi / 4, name="right derived from up = (-1, 0, 0): degenerate", id_dev=True),
         dict(n=300, n_dirs=2, rr=1, flips=(0, 0), r1=np.pi / 4, none=True, name="no survivors: both best bins are bin 0"),
         dict(n=300, n_dirs=2, rr=1, flips=(0, 0), r1=np.pi / 4, refused=True, name="refused instance", id_dev=True)]


def tail_sphere():
    """64 unit vectors with a descending y column (the Fibonacci sphere's order) holding (0, 1, 0), (1, 1, 0) / sqrt 2, (+-1, 0, 0)"""
    y = 1.0 - 2.0 * (np.arange(S_TAIL) + 0.5) / S_TAIL
    r, phi = np.sqrt(1.0 - y * y), np.arange(S_TAIL) * np.pi * (3.0 - np.sqrt(5.0))
    sph = np.stack([r * np.cos(phi), y, r * np.sin(phi)], -1)
    sph[0], sph[RIGHT_BIN], sph[UP_BIN], sph[NEG_BIN] = (0, 1, 0), (np.sqrt(0.5), np.sqrt(0.5), 0), (1, 0, 0), (-1, 0, 0)
    assert (np.diff(sph[:, 1]) <= 0).all()
    return sph


def make_item(k, spec, sph, oracle):
    """Every pair has its own two points, a - b along +x: the rotation head 1e-4 aims all 72 candidates of direction 0 at the bin
    (1, 0, 0), and pi / 4 puts candidate 0 of direction 1 on (1, 1, 0) / sqrt 2 (the frame's x of ab = (1, 0, 0) is (0, 1, 0),
    voting.py:135).  (mu, nu) are the closed form for the centre, so the circle passes through it; a quarter of the pairs miss it by
    10 cells and must not count: their heads aim elsewhere, their logits are large."""
    rng = np.random.default_rng(100 + k)
    n, res = spec["n"], 0.004
    dims, corner = (60, 60, 60), np.array([-0.02, 0.01, 0.3], F)
    cell = np.array([30, 29, 31])
    flat = -1 if spec.get("refused") else int((cell[0] * dims[1] + cell[1]) * dims[2] + cell[2])
    T = corner.astype(D) + cell * res
    a = (T + rng.uniform(-0.06, 0.06, (n, 3))).astype(F)
    a[:, 1:] += np.where(np.abs(a[:, 1:] - T[1:]) < 0.01, 0.02, 0.0).astype(F)      # nu >= 2 cells
    b = a.copy()
    b[:, 0] -= rng.uniform(0.02, 0.05, n).astype(F)
    pts = np.stack([a, b], 1).reshape(2 * n, 3)
    nrm = rng.normal(size=(2 * n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    idx = np.arange(2 * n, dtype=np.int32).reshape(n, 2)
    w = a.astype(D) - T
    miss = (np.arange(n) % 4 == 3) & (n > 1)
    out = np.stack([w[:, 0], np.hypot(w[:, 1], w[:, 2]) + np.where(miss, 10 * res, 0.0)], -1).astype(F)
    if spec.get("none"):
        out[:, 1] = 0.0
    T32 = oracle.center_from_argmax(flat, dims, corner, res).astype(F) if flat >= 0 else None
    heads = np.zeros((n, 8), F)
    heads[:, 0], heads[:, 1] = np.where(miss, -1e-4, 1e-4), np.where(miss, -0.3, spec["r1"])
    heads[:, 4:7] = np.where(miss[:, None], 9.0, rng.normal(0.0, 0.3, (n, 3)))
    bins = (UP_BIN, RIGHT_BIN)
    for j in range(2):                                                        # +-3 with the target's sign, or against it
        tj = PC.bce_terms(pts, nrm, idx, np.zeros(n, F), sph[bins[j]])[2]
        heads[:, 2 + j] = np.where(miss, 40.0, (2 * tj - 1) * 3.0 * (-1 if spec["flips"][j] else 1))
    return dict(spec=spec, pts=pts, nrm=nrm, idx=idx, out=out, heads=heads, corner=corner, dims=dims, res=res, flat=flat, T=T, T32=T32,
                tol=float(F(3 * res)), peak=float(k) + 0.5, object_id=1000 + k)


def want_record(it, sph, oracle):
    """the record from the oracle's survivors and float64 sums (pose_tail_cases.assemble), and the 21-double rec it comes from"""
    spec, n = it["spec"], it["spec"]["n"]
    if it["flat"] >= 0:
        T, T32 = oracle.center_from_argmax(it["flat"], it["dims"], it["corner"], it["res"]), it["T32"]
    else:                                                                     # (the index is used arithmetically only)
        gy, gz = it["dims"][1], it["dims"][2]
        f = -1
        c = np.array([int(f / (gy * gz)), int(math.fmod(math.fmod(f, gy * gz), gy * gz) / gz), int(math.fmod(math.fmod(f, gy * gz), gz))])
        T = it["corner"].astype(D) + c * it["res"]
        T32 = T.astype(F)
    _, mask = oracle.backvote(it["pts"], it["out"], it["idx"], it["corner"], it["res"], 72, it["dims"], T32, F(it["tol"]))
    surv = np.nonzero(mask)[0]
    bins, sums = [], []
    for j in range(spec["n_dirs"]):
        cand = oracle.rot_voting(it["pts"], it["heads"][surv, j], it["idx"][surv], 72)
        cnt = oracle.sphere_count(cand, sph, 1.5) if surv.size else np.zeros(S_TAIL, np.int64)
        bins.append(int(np.argmax(cnt)))
        up, down, _ = PC.bce_terms(it["pts"], it["nrm"], it["idx"][surv], it["heads"][surv, 2 + j], sph[bins[j]])
        sums.append((math.fsum(up), math.fsum(down)))
    bins += [0] * (2 - len(bins))
    ssum = [math.fsum(it["heads"][surv, 4 + c].astype(D)) for c in range(3)]
    rec, info = PC.assemble(T, sph[bins], sums, ssum, surv.size, spec["n_dirs"], spec["rr"], SCALE_MEAN, it["flat"], it["peak"], it["object_id"])
    return rec, info, bins, surv, sums, ssum


def test_record_assembled_on_the_device_in_every_branch(dev, oracle):
    """cppf_pose_tail_batch, eight items in one call, second_pass = 0 on hand-made outputs and heads, against a float64 restatement
    of nocs/inference.py:299-339 (pose_tail_cases.assemble) and, for the items that have a pose, inference._assemble on the item's
    21-double rec: the four flip combinations, the random-tangent fallback from both derived rights and from equal best bins, no
    survivors, a refused instance (arg-max -1: center_from_argmax_body uses the index arithmetically only -- quotients and
    remainders, never an address --, so the tail runs on and the record's first twelve doubles are NaN), object ids from the device
    and from the host, n_pairs 1 / 1023 / 1025 / 4100, n_dirs 1 and 2.  Directions to 1e-12, scale to 1e-6 (fp32 exp on either side),
    as tests/test_gpu_resident.py; the same call twice gives the same records (launch 1 re-arms tail0 and the tickets)."""
    import ctypes as C
    from types import SimpleNamespace
    from cppf_amd import inference
    L = _lib.lib()
    sph = tail_sphere()
    # the kernel's three fallback constants are numpy's default_rng(0).standard_normal(3)
    assert [float.fromhex(h) for h in PC.FALLBACK_HEX] == list(np.random.default_rng(0).standard_normal(3))
    src = open(__import__("os").path.join(__import__("os").path.dirname(_lib.library_path()), "pose_tail.hip")).read()
    assert all(h.lstrip("-") in src for h in PC.FALLBACK_HEX)
    d_s32, d_s64 = t(sph.astype(F), dev), t(sph, dev)
    items = [make_item(k, spec, sph, oracle) for k, spec in enumerate(ITEMS)]
    arr = (_lib.PoseTailItem * 8)()
    keep, outs = [], []
    for k, it in enumerate(items):
        n = it["spec"]["n"]
        c0 = 176 + ((2 * S_TAIL * 4 + 15) & ~15)                              # record | counts i32[2][S] | ticket | chunk counts
        nbytes = c0 + 16 + ((4 * ((n + 1023) // 1024) + 15) & ~15)
        tail0 = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        d = dict(pts=t(it["pts"], dev), nrm=t(it["nrm"], dev), idx=t(it["idx"], dev), out=t(it["out"], dev), heads=t(it["heads"], dev),
                 corner=t(it["corner"], dev), argmax=t(np.array([it["flat"]], np.int64), dev), peak=t(np.array([it["peak"]], F), dev),
                 tail0=tail0, T32=torch.zeros(3, dtype=torch.float32, device=dev), mask=torch.empty(n, dtype=torch.uint8, device=dev),
                 surv=torch.full((n,), -1, dtype=torch.int32, device=dev), count=torch.full((1,), -1, dtype=torch.int32, device=dev),
                 best_idx=torch.full((2,), -1, dtype=torch.int64, device=dev),
                 sums=torch.empty(int(L.cppf_pose_sums_workspace_bytes()), dtype=torch.uint8, device=dev),
                 record=torch.full((16,), 9.0, dtype=torch.float64, device=dev), oid=t(np.array([it["object_id"]], np.int64), dev))
        keep.append(d)
        a = arr[k]
        a.pc, a.nrm, a.feat, a.idx64, a.idx32 = d["pts"].data_ptr(), d["nrm"].data_ptr(), None, None, d["idx"].data_ptr()
        a.outputs, a.u_rot, a.heads = d["out"].data_ptr(), None, d["heads"].data_ptr()
        a.corner, a.shape_dev, a.argmax_idx, a.peak = d["corner"].data_ptr(), None, d["argmax"].data_ptr(), d["peak"].data_ptr()
        a.packed, a.mlp_workspace, a.mlp_workspace_bytes, a.vote_workspace = None, None, 0, None
        a.rec, a.T32, a.tail0, a.tail0_bytes = tail0.data_ptr(), d["T32"].data_ptr(), tail0.data_ptr(), nbytes
        a.mask, a.chunk_counts, a.surv, a.count = d["mask"].data_ptr(), tail0.data_ptr() + c0 + 16, d["surv"].data_ptr(), d["count"].data_ptr()
        a.counts, a.best_idx, a.ticket = tail0.data_ptr() + 176, d["best_idx"].data_ptr(), tail0.data_ptr() + c0
        a.sums_workspace, a.sums_workspace_bytes = d["sums"].data_ptr(), d["sums"].numel()
        a.n_points, a.n_pairs, a.res64, a.res, a.tol = 2 * n, n, it["res"], it["res"], it["tol"]
        a.gx, a.gy, a.gz = it["dims"]
        a.n_dirs, a.second_pass, a.record_out = it["spec"]["n_dirs"], 0, d["record"].data_ptr()
        a.object_id_dev, a.object_id_host = (d["oid"].data_ptr(), -7) if it["spec"].get("id_dev") else (None, it["object_id"])
        a.scale_mean = (C.c_double * 3)(*SCALE_MEAN)
        a.regress_right = it["spec"]["rr"]
    runs = []
    for _ in range(2):
        _lib.check(L.cppf_pose_tail_batch(8, C.cast(arr, C.c_void_p), 32, (C.c_int * 4)(84, 32, 32, 16), 3, 141, 32, 36, 72, d_s32.data_ptr(),
                                          d_s64.data_ptr(), S_TAIL, 1, float(F(np.cos(np.radians(1.5)))), 10000, stream_ptr(dev)), "pose_tail_batch")
        torch.cuda.synchronize()
        runs.append([(d["record"].cpu().numpy().copy(), d["tail0"][:168].cpu().numpy().view(D).copy(), d["best_idx"].cpu().numpy().copy())
                     for d in keep])
    for k, it in enumerate(items):
        spec, (got, rec21, bi) = it["spec"], runs[0][k]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(runs[0][k], runs[1][k])), spec["name"]
        want, info, bins, surv, sums, ssum = want_record(it, sph, oracle)
        print(f"[{spec['name']}] survivors {surv.size} of {spec['n']}, bins {bins}, {info}, record {got}")
        # the construction is what it claims: winning bins, flips, the fallback
        if spec.get("none"):
            assert surv.size == 0 and bins == [0, 0] and info == dict(flips=[False, False], fallback=True)
        elif not spec.get("refused"):
            assert surv.size == (spec["n"] if spec["n"] == 1 else spec["n"] - spec["n"] // 4), spec["name"]
            assert bins[:spec["n_dirs"]] == [UP_BIN, RIGHT_BIN][:spec["n_dirs"]] and info["flips"] == [bool(f) for f in spec["flips"][:spec["n_dirs"]]]
            assert info["fallback"] == (spec["rr"] == 0), spec["name"]
        assert list(bi[:spec["n_dirs"]]) == bins[:spec["n_dirs"]], spec["name"]
        assert got[12] == it["flat"] and got[13] == it["peak"] and got[14] == surv.size and got[15] == it["object_id"], spec["name"]
        if spec.get("refused"):
            assert np.isnan(got[:12]).all() and got[12] == -1
            continue
        np.testing.assert_array_equal(got[0:3], want[0:3], err_msg=spec["name"])
        np.testing.assert_allclose(got[3:9], want[3:9], rtol=0, atol=1e-12, err_msg=spec["name"])
        np.testing.assert_allclose(got[9:12], want[9:12], rtol=1e-6, err_msg=spec["name"])
        if info["fallback"]:                                                  # default_rng(0).standard_normal(3), projected and normalised
            r = np.random.default_rng(0).standard_normal(3)
            r = r - r.dot(want[3:6]) * want[3:6]
            np.testing.assert_allclose(got[6:9], r / np.linalg.norm(r), rtol=0, atol=1e-12)
        if spec.get("none"):
            np.testing.assert_allclose(got[9:12], np.exp(0.0) * np.asarray(SCALE_MEAN) * 2, rtol=1e-6)
            assert got[14] == 0 and list(got[3:6]) == list(sph[0])
        # the host assembly on the item's own 21-double rec (it reads both directions: where one was asked for, the record's)
        if spec["n_dirs"] == 2 or not spec["rr"]:
            host = inference._assemble(rec21, SimpleNamespace(regress_right=bool(spec["rr"]), z_right=False, scale_mean=SCALE_MEAN))
            np.testing.assert_array_equal(got[0:3], host["T"])
            np.testing.assert_allclose(got[3:6], host["up"], rtol=0, atol=1e-12)
            np.testing.assert_allclose(got[6:9], host["right"], rtol=0, atol=1e-12)
            np.testing.assert_allclose(got[9:12], host["scale"], rtol=1e-6)
            assert host["n_surv"] == surv.size
