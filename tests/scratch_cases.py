"""The plain-scratch contract of include/cppf.h, as one table (tests/test_gpu_scratch_contract.py runs it on the device,
tests/test_scratch_contract_cpu.py checks the table and the harness without one).

The header promises that a workspace sized by its *_workspace_bytes() query is enough and that its contents are plain scratch --
except the centre vote's, whose first cppf_vote_workspace_init_bytes() bytes carry state and are zeroed once.  A ROW of the table
is one size query with the entry points that consume it, at two shapes whose workspace LAYOUTS differ (not only their lengths):

    sizes(p)         declared bytes per workspace region at shape p, through the query (most rows have one region)
    inputs(p, dev)   seeded device inputs, built once per shape and never written
    run(inp, p, regions, short)   the calls through the C ABI with regions = [(ptr, bytes), ...] -> (return codes, Outs)

No call is ever handed fewer REAL bytes than it declares: the refusal leg passes declared - 1 as the size of a full-size buffer, the
exact leg puts the declared bytes between two fences.  A violation is a failed assertion, never a fault.

Outputs are pre-filled with 0xCD bytes (or zero where the header asks for a zero-initialised output) in every leg alike, so rows the
entry point leaves untouched compare equal, and compared as raw bytes (NaNs included)."""
import ctypes as C
import functools

import numpy as np
import torch

from cppf_amd import _lib
from cppf_amd._torch_util import call

FENCE = 256 * 1024
FENCE_BYTE = 0xA5
OUT_BYTE = 0xCD
# the two poison patterns: every byte 0xFF reads as NaN (float32 / float64), -1 (int32) and the maximum (unsigned); the 32-bit word
# 0x7F7F8000 -- bytes 7F 7F 80 00 from the most significant -- reads as a large finite float32 (3.39e38) and a large positive int32
POISONS = ("ff", "big")
BIG_WORD = 0x7F7F8000
EWORKSPACE, EINVAL = -2, -1
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64


def round_up(n, m):
    return (int(n) + m - 1) // m * m


class Fenced:
    """one uint8 tensor [fence | body | fence]: FENCE bytes of 0xA5 on either side of a body of `declared` rounded up to 256; `ptr`
    (the body's address) is 256-byte aligned; the bytes from ptr + declared on count as fence"""

    def __init__(self, declared, dev):
        self.declared, self.body_bytes = int(declared), round_up(max(int(declared), 1), 256)
        self.t = torch.empty(FENCE + self.body_bytes + FENCE + 256, dtype=U8, device=dev)
        self.off = (-self.t.data_ptr()) % 256
        self.t.fill_(FENCE_BYTE)
        self.ptr = self.t.data_ptr() + self.off + FENCE
        self.body = self.t[self.off + FENCE:self.off + FENCE + self.declared]

    def fences(self):
        lo = self.t[self.off:self.off + FENCE]
        hi = self.t[self.off + FENCE + self.declared:self.off + FENCE + self.body_bytes + FENCE]
        return lo, hi

    def intact(self):
        return all(bool((f == FENCE_BYTE).all()) for f in self.fences())


class Region:
    """what a row's run() gets per workspace: unpacks to (pointer, size passed to the ABI); `mem` is a uint8 view of the declared bytes"""

    def __init__(self, ptr, nbytes, mem):
        self.ptr, self.nbytes, self.mem = int(ptr), int(nbytes), mem

    def __iter__(self):
        return iter((self.ptr, self.nbytes))

    @property
    def short(self):        # the refusal leg passes fewer bytes than `mem` really holds
        return self.nbytes < self.mem.numel()


def poison(body, pattern):
    """fill a uint8 view (4-byte aligned start) with one of POISONS"""
    if pattern == "ff":
        body.fill_(0xFF)
        return
    assert pattern == "big" and body.data_ptr() % 4 == 0
    n4 = body.numel() // 4 * 4
    if n4:
        body[:n4].view(I32).fill_(BIG_WORD)
    body[n4:].fill_(0x7F)


def poison_range(declared, state, init_bytes):
    """(zeroed, poisoned) byte ranges of a workspace of `declared` bytes: a vote workspace (`state`) keeps its first
    min(init_bytes, declared) bytes zero -- the header's contract -- and only the remainder is poisoned"""
    keep = min(int(init_bytes), int(declared)) if state else 0
    return (0, keep), (keep, int(declared))


def _init_bytes(init_bytes):
    return _lib.lib().cppf_vote_workspace_init_bytes() if init_bytes is None else init_bytes


def dirty(body, declared, state, pattern, init_bytes=None):
    """poison the plain-scratch part of a workspace body in place and write NOTHING to a vote workspace's state region: what may
    happen to a workspace in use, between two calls that share it (init_bytes: the library's, unless a test of the rule says)"""
    _, (p0, p1) = poison_range(declared, state, _init_bytes(init_bytes))
    if p1 > p0:
        poison(body[p0:p1], pattern)


def prepare(body, declared, state, pattern, init_bytes=None):
    """a workspace body before its FIRST call: the vote's state region zeroed once, as the header demands, the rest dirtied"""
    (z0, z1), _ = poison_range(declared, state, _init_bytes(init_bytes))
    if z1 > z0:
        body[z0:z1].zero_()
    dirty(body, declared, state, pattern, init_bytes)


class Outs:
    """the outputs of one run: device tensors pre-filled with OUT_BYTE (zero=True: with zeros), read back as raw bytes"""

    def __init__(self, dev):
        self.dev, self.t, self.zero = dev, {}, {}

    def new(self, name, shape, dtype, zero=False):
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        t.view(U8).fill_(0 if zero else OUT_BYTE)
        self.t[name], self.zero[name] = t, zero
        return t

    def host(self):
        torch.cuda.synchronize(self.dev)
        return {k: v.cpu().numpy().reshape(-1).view(np.uint8).copy() for k, v in self.t.items()}

    def touched(self):
        """names of the outputs that no longer hold their pre-fill"""
        h = self.host()
        return [k for k, v in h.items() if not (v == (0 if self.zero[k] else OUT_BYTE)).all()]


def same(a, b):
    """names of the outputs whose bytes differ between two host() dicts"""
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(a[k], b[k])]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def L():
    return _lib.lib()


def cints(v):
    return (C.c_int * len(v))(*v)


# ------------------------------------------------------------------------------------------------------------ rows
class Row:
    name = None
    query = None            # the size query of the header
    also = ()               # further queries the row covers (cppf_vote_workspace_init_bytes)
    entries = ()            # the entry points run
    state = False           # the vote's contract: the first init_bytes of every region stay zero
    refusal = EWORKSPACE
    shapes = {}             # "small" / "large" -> the shape's parameters
    axes = ()               # names of the size arguments of q(), for the monotonicity check

    def q(self, **a):       # the query on its size arguments alone
        raise NotImplementedError

    def qargs(self, p):     # the size arguments of shape p
        return {k: p[k] for k in self.axes}

    def valid(self, **a):   # whether the size arguments are ones the entry point accepts (the query returns 0 for others)
        return all(v >= 1 for v in a.values())

    def sizes(self, p):
        return [int(self.q(**self.qargs(p)))]

    def refusals(self, p):  # the refusal leg's cases: each a list of the regions handed one byte less than declared
        return [list(range(len(self.sizes(p))))]

    def inputs(self, p, dev):
        raise NotImplementedError

    def run(self, inp, p, regions, short=False):
        raise NotImplementedError


_inputs = {}


def inputs_of(row, shape, dev):
    key = (row.name, shape, str(dev))
    if key not in _inputs:
        _inputs[key] = row.inputs(row.shapes[shape], dev)
    return _inputs[key]


def _cloud(rng, n, ext=0.3):
    pc = rng.uniform(0, ext, (n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3))
    return pc, (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)


# --- the centre vote -------------------------------------------------------------------------------------------------
VOTE_ROTS = 72


def _vote_inputs(rng, n, P, dims, res, dev):
    ext = np.array(dims, np.float32) * np.float32(res)
    pc = (rng.uniform(0.05, 0.95, (n, 3)) * ext).astype(np.float32)
    idx = rng.integers(0, n, (P, 2)).astype(np.int32)
    out = np.stack([rng.uniform(-0.3, 0.3, P), rng.uniform(0.0, 0.3, P)], -1).astype(np.float32) * float(ext.min())
    return dict(pc=T(pc, dev), idx=T(idx, dev), outputs=T(out, dev), corner=T(np.zeros(3, np.float32), dev),
                shape=T(np.array([n, *dims], np.int32), dev))


class VoteRow(Row):
    """by-value vote: a 2-tile grid on the fused path; a grid of >= 4 tiles on the binned path, whose pair -> tile queues live in
    the workspace.  The back-vote entry points read the rotation table the vote left (vote_workspace)."""
    name, query, also = "vote", "cppf_vote_workspace_bytes", ("cppf_vote_workspace_init_bytes",)
    entries = ("cppf_vote_argmax", "cppf_ppf_voting", "cppf_vote_grid_raw", "cppf_backvote_ws", "cppf_backvote_count")
    state = True
    shapes = dict(small=dict(n_ppfs=1500, n=200, gx=40, gy=36, gz=30, res=0.01, path=2, min_tiles=2, max_tiles=2),
                  large=dict(n_ppfs=3000, n=300, gx=70, gy=64, gz=48, res=0.01, path=3, min_tiles=4, max_tiles=64))
    axes = ("n_ppfs",)      # gx, gy, gz: see test_scratch_contract_cpu.test_vote_query_in_the_grid_dims

    def q(self, n_ppfs, gx, gy, gz):
        return L().cppf_vote_workspace_bytes(int(n_ppfs), VOTE_ROTS, gx, gy, gz)

    def qargs(self, p):
        return dict(n_ppfs=p["n_ppfs"], gx=p["gx"], gy=p["gy"], gz=p["gz"])

    def inputs(self, p, dev):
        return _vote_inputs(np.random.default_rng(11), p["n"], p["n_ppfs"], (p["gx"], p["gy"], p["gz"]), p["res"], dev)

    def run(self, inp, p, regions, short=False):
        (ws, nb), = regions
        dev, P, n, d = inp["pc"].device, p["n_ppfs"], p["n"], (p["gx"], p["gy"], p["gz"])
        o = Outs(dev)
        grid, idx, val = o.new("grid", d, F32), o.new("idx", 1, I64), o.new("val", 1, F32)
        rcs = [call("cppf_vote_argmax", dev, inp["pc"], inp["outputs"], None, inp["idx"], 0, grid, inp["corner"], p["res"], n, P, VOTE_ROTS,
                    *d, 1, 0, idx, val, ws, nb, ok=(self.refusal,))]
        grid2 = o.new("grid_acc", d, F32, zero=True)
        rcs.append(call("cppf_ppf_voting", dev, inp["pc"], inp["outputs"], None, inp["idx"], grid2, inp["corner"], p["res"], n, P, VOTE_ROTS,
                        *d, 1, ws, nb, ok=(self.refusal,)))
        raw, quantum = o.new("raw", d, I64), o.new("quantum", 1, F32)
        rcs.append(call("cppf_vote_grid_raw", dev, inp["pc"], inp["outputs"], None, inp["idx"], 0, raw, quantum, inp["corner"], p["res"], n, P,
                        VOTE_ROTS, *d, 1, 0, 0, ws, nb, ok=(self.refusal,)))
        if not short:       # the back-vote takes no size: it reads the table the votes above left
            centre = T(np.array(d, np.float32) * np.float32(p["res"] * 0.5), dev)
            tol = float(np.float32(3 * p["res"]))
            off, mask = o.new("offsets", (P, 3), F32, zero=True), o.new("mask", P, U8)
            rcs.append(call("cppf_backvote_ws", dev, inp["pc"], inp["outputs"], off, inp["idx"], inp["corner"], p["res"], P, VOTE_ROTS, *d,
                            None, centre, tol, mask, ws))
            mask2, chunks = o.new("mask_count", P, U8), o.new("chunks", (P + 1023) // 1024, I32, zero=True)
            rcs.append(call("cppf_backvote_count", dev, inp["pc"], inp["outputs"], inp["idx"], inp["corner"], p["res"], P, VOTE_ROTS, *d,
                            None, centre, tol, mask2, chunks, ws))
        return rcs, o


class VoteDynRow(Row):
    """shape-polymorphic vote: tile classes 0 (fused kernel) and 16 (binning + queues); region 0 serves the single call and item 0
    of a two-item batch, region 1 item 1"""
    name, query = "vote_dyn", "cppf_vote_workspace_bytes_dyn_pairs"
    entries = ("cppf_vote_argmax_dyn", "cppf_vote_argmax_batch")
    state = True
    shapes = dict(small=dict(many_tiles=0, n_ppfs=1500, n=200, gx=40, gy=36, gz=30, res=0.01),
                  large=dict(many_tiles=16, n_ppfs=3000, n=300, gx=70, gy=64, gz=48, res=0.01))
    axes = ("n_ppfs",)      # many_tiles is a class, not a size: see test_scratch_contract_cpu.test_vote_dyn_query_in_the_tile_class

    def q(self, n_ppfs, many_tiles=0):
        return L().cppf_vote_workspace_bytes_dyn_pairs(int(many_tiles), int(n_ppfs))

    def valid(self, n_ppfs, many_tiles=0):
        return n_ppfs >= 1

    def qargs(self, p):
        return dict(n_ppfs=p["n_ppfs"], many_tiles=p["many_tiles"])

    def sizes(self, p):
        return [int(self.q(**self.qargs(p)))] * 2

    def refusals(self, p):  # both items short; and a valid item 0 in front of a short item 1: nothing of item 0 may have run
        return [[0, 1], [1]]

    def inputs(self, p, dev):
        d = (p["gx"], p["gy"], p["gz"])
        a = _vote_inputs(np.random.default_rng(12), p["n"], p["n_ppfs"], d, p["res"], dev)
        b = _vote_inputs(np.random.default_rng(13), p["n"], p["n_ppfs"], d, p["res"], dev)
        return dict(a=a, b=b)

    def run(self, inp, p, regions, short=False):
        dev, P, n = inp["a"]["pc"].device, p["n_ppfs"], p["n"]
        cells = p["gx"] * p["gy"] * p["gz"]
        o = Outs(dev)
        a = inp["a"]
        rcs = []
        if not short or regions[0].short:       # (a refusal case that shortens item 1 alone is about the batch)
            grid, idx, val = o.new("grid", cells, F32), o.new("idx", 1, I64), o.new("val", 1, F32)
            rcs.append(call("cppf_vote_argmax_dyn", dev, a["pc"], a["outputs"], None, a["idx"], 0, grid, cells, a["corner"], p["res"], n, P,
                            VOTE_ROTS, a["shape"], p["many_tiles"], 1, 0, idx, val, *regions[0], ok=(self.refusal,)))
        arr = (_lib.VoteItem * 2)()
        for i, k in enumerate("ab"):
            m = inp[k]
            g, ix, v = o.new(f"grid_{k}", cells, F32), o.new(f"idx_{k}", 1, I64), o.new(f"val_{k}", 1, F32)
            it = arr[i]
            it.points, it.outputs, it.probs, it.point_idxs = m["pc"].data_ptr(), m["outputs"].data_ptr(), None, m["idx"].data_ptr()
            it.grid, it.corner, it.out_idx, it.out_val = g.data_ptr(), m["corner"].data_ptr(), ix.data_ptr(), v.data_ptr()
            it.workspace, it.workspace_bytes = regions[i]
            it.shape_dev, it.grid_capacity, it.n_points, it.n_ppfs, it.res = m["shape"].data_ptr(), cells, n, P, p["res"]
            it.gx = it.gy = it.gz = 1
            it.idx_is_i64, it.many_tiles = 0, p["many_tiles"]
        rcs.append(call("cppf_vote_argmax_batch", dev, 2, arr, VOTE_ROTS, 1, 0, ok=(self.refusal,)))
        if short:           # a refused call launched nothing: the state blocks are as zero as they were handed over (a binning launch
            init = int(L().cppf_vote_workspace_init_bytes())            # without its consumer would leave its queue counters there)
            for k, r in zip("ab", regions):
                o.new(f"state_{k}", init, U8, zero=True).copy_(r.mem[:init])
        return rcs, o


# --- the encoders ----------------------------------------------------------------------------------------------------
PPFFCS, OUT_DIM, FEAT = [84, 32, 32, 16], 141, 40


@functools.lru_cache(maxsize=None)
def _ppf_encoder(dev, precision="fp32"):
    from cppf_amd.models.model import PPFEncoder
    torch.manual_seed(5)
    enc = PPFEncoder(PPFFCS, OUT_DIM).eval().to(dev)
    return enc.set_precision(precision)


@functools.lru_cache(maxsize=None)
def _point_encoder(dev, num_layers, k):
    from cppf_amd.models.model import PointEncoder
    torch.manual_seed(6)
    return PointEncoder(k=k, spfcs=[32, 64, 32, 32], num_layers=num_layers, out_dim=32).eval().to(dev)


def _pair_inputs(rng, N, P, dev):
    pc, nrm = _cloud(rng, N)
    sel = np.sort(rng.choice(P, P // 3, replace=False)).astype(np.int32)
    return dict(pc=T(pc, dev), nrm=T(nrm, dev), feat=T(rng.standard_normal((N, FEAT)).astype(np.float32), dev),
                idx=T(rng.integers(0, N, (P, 2)).astype(np.int32), dev), u_tr=T(rng.random((P, 2)).astype(np.float32), dev),
                u_rot=T(rng.random((P, 2)).astype(np.float32), dev), sel=T(sel, dev), n_sel=T(np.array([len(sel)], np.int32), dev),
                grad=T(rng.standard_normal((P, OUT_DIM)).astype(np.float32), dev))


class PairMlpRow(Row):
    """the per-point table: forward, the fused decode, the selected second pass ON THE TABLE THE FIRST PASS LEFT (documented: the
    workspace of the preceding decode is reused, not rebuilt), and the bf16 forward in the same workspace"""
    name, query = "pair_mlp", "cppf_pair_mlp_workspace_bytes"
    entries = ("cppf_pair_mlp_forward", "cppf_pair_mlp_decode", "cppf_pair_mlp_decode_sel", "cppf_pair_mlp_bf16_forward")
    shapes = dict(small=dict(N=64, P=65), large=dict(N=300, P=1000))
    axes = ("N",)

    def q(self, N):
        return L().cppf_pair_mlp_workspace_bytes(int(N), FEAT, cints(PPFFCS), 3, OUT_DIM)

    def inputs(self, p, dev):
        return _pair_inputs(np.random.default_rng(21), p["N"], p["P"], dev)

    def decode(self, inp, p, region, o, tag="", feat=None):
        dev, N, P = inp["pc"].device, p["N"], p["P"]
        feat = inp["feat"] if feat is None else feat
        outputs = o.new("outputs" + tag, (P, 2), F32)
        return call("cppf_pair_mlp_decode", dev, inp["pc"], inp["nrm"], feat, inp["idx"], 0, _ppf_encoder(dev)._packed_weights(dev), N, FEAT,
                    cints(PPFFCS), 3, P, OUT_DIM, 32, 36, -0.5, 0.5, inp["u_tr"], None, outputs, None, *region, ok=(self.refusal,))

    def decode_sel(self, inp, p, region, o, tag=""):
        dev, N, P = inp["pc"].device, p["N"], p["P"]
        heads = o.new("heads" + tag, (P, 8), F32)
        return call("cppf_pair_mlp_decode_sel", dev, inp["pc"], inp["nrm"], inp["feat"], inp["idx"], 0, _ppf_encoder(dev)._packed_weights(dev),
                    N, FEAT, cints(PPFFCS), 3, P, OUT_DIM, 32, 36, inp["u_rot"], inp["sel"], inp["n_sel"], P, heads, *region,
                    ok=(self.refusal,))

    def run(self, inp, p, regions, short=False):
        dev, N, P = inp["pc"].device, p["N"], p["P"]
        o = Outs(dev)
        logits = o.new("logits", (P, OUT_DIM), F32)
        rcs = [call("cppf_pair_mlp_forward", dev, inp["pc"], inp["nrm"], inp["feat"], inp["idx"], 0, _ppf_encoder(dev)._packed_weights(dev), N,
                    FEAT, cints(PPFFCS), 3, P, OUT_DIM, logits, *regions[0], ok=(self.refusal,))]
        rcs.append(self.decode(inp, p, regions[0], o))
        rcs.append(self.decode_sel(inp, p, regions[0], o))
        lb = o.new("logits_bf16", (P, OUT_DIM), F32)
        rcs.append(call("cppf_pair_mlp_bf16_forward", dev, inp["pc"], inp["nrm"], inp["feat"], inp["idx"], 0,
                        _ppf_encoder(dev, "bf16")._packed_weights(dev), N, FEAT, cints(PPFFCS), 3, P, OUT_DIM, lb, *regions[0],
                        ok=(self.refusal,)))
        return rcs, o


class PairMlpBackwardRow(Row):
    name, query = "pair_mlp_backward", "cppf_pair_mlp_backward_workspace_bytes"
    entries = ("cppf_pair_mlp_backward",)
    shapes = dict(small=dict(N=64, P=65), large=dict(N=300, P=1000))
    axes = ("P", "N")

    def q(self, P, N):
        return L().cppf_pair_mlp_backward_workspace_bytes(int(P), int(N), FEAT, cints(PPFFCS), 3, OUT_DIM)

    def inputs(self, p, dev):
        return _pair_inputs(np.random.default_rng(22), p["N"], p["P"], dev)

    def run(self, inp, p, regions, short=False):
        dev, N, P = inp["pc"].device, p["N"], p["P"]
        flat, offs = _ppf_encoder(dev)._flat_params(dev)
        o = Outs(dev)
        gp, gf = o.new("grad_params", flat.numel(), F32), o.new("grad_feat", (N, FEAT), F32, zero=True)
        return [call("cppf_pair_mlp_backward", dev, inp["pc"], inp["nrm"], inp["feat"], inp["idx"], 0, flat, offs, N, FEAT, cints(PPFFCS), 3, P,
                     OUT_DIM, inp["grad"], gp, gf, *regions[0], ok=(self.refusal,))], o


def _point_inputs(rng, N, k, layers, dev):
    pc, nrm = _cloud(rng, N)
    d = dict(pc=T(pc, dev), nrm=T(nrm, dev), nbrs=torch.empty((N, k), dtype=I32, device=dev),
             grad=T(rng.standard_normal((N, 40)).astype(np.float32), dev))
    call("cppf_knn", dev, d["pc"], None, N, k, d["nbrs"])
    if layers == 1:          # the forward output the backward reads (pooled maxima), computed once in scratch of its own
        d["out_fwd"] = _point_encoder(dev, 1, k).forward_nbrs(d["pc"], d["nrm"], d["nbrs"]).detach().clone()
    return d


def _penc_args(enc, dev):
    packed, desc = enc._packed_weights(dev)
    return packed, (cints(desc["hidden"]), len(desc["hidden"]), desc["rank"], desc["n_nbr_feats"], desc["n_out"], desc["n_glob"])


class PointEncoderRow(Row):
    """one layer (no inter-layer buffer) and two (the first layer's features live in the workspace)"""
    name, query = "point_encoder", "cppf_point_encoder_workspace_bytes"
    entries = ("cppf_point_encoder_forward",)
    shapes = dict(small=dict(N=70, k=8, layers=1), large=dict(N=300, k=16, layers=2))
    axes = ("N", "layers")

    def q(self, N, layers):
        return L().cppf_point_encoder_workspace_bytes(int(N), 32, 8, int(layers))

    def inputs(self, p, dev):
        return _point_inputs(np.random.default_rng(31), p["N"], p["k"], 0, dev)

    def run(self, inp, p, regions, short=False):
        dev, N, k = inp["pc"].device, p["N"], p["k"]
        with torch.no_grad():
            packed, shape = _penc_args(_point_encoder(dev, p["layers"], k), dev)
        o = Outs(dev)
        out = o.new("out", (N, 40), F32)
        return [call("cppf_point_encoder_forward", dev, inp["pc"], inp["nrm"], inp["nbrs"], N, k, packed, *shape, p["layers"], out, *regions[0],
                     ok=(self.refusal,))], o


class PointEncoderBackwardRow(Row):
    """fewer points than partial gradients, and more than CPPF_SPRIN_BWD_MAX_PARTS = 1024 (the two-level sum)"""
    name, query = "point_encoder_backward", "cppf_point_encoder_backward_workspace_bytes"
    entries = ("cppf_point_encoder_backward",)
    shapes = dict(small=dict(N=70, k=8), large=dict(N=1100, k=16))
    axes = ("N",)

    def q(self, N):
        return L().cppf_point_encoder_backward_workspace_bytes(int(N))

    def inputs(self, p, dev):
        with torch.no_grad():
            return _point_inputs(np.random.default_rng(32), p["N"], p["k"], 1, dev)

    def run(self, inp, p, regions, short=False):
        dev, N, k = inp["pc"].device, p["N"], p["k"]
        with torch.no_grad():
            packed, shape = _penc_args(_point_encoder(dev, 1, k), dev)
        o = Outs(dev)
        gp = o.new("grad_packed", 9256, F32)
        return [call("cppf_point_encoder_backward", dev, inp["pc"], inp["nrm"], inp["nbrs"], N, k, packed, *shape, 1, inp["out_fwd"], None,
                     inp["grad"], gp, *regions[0], ok=(self.refusal,))], o


# --- the pose tail ---------------------------------------------------------------------------------------------------
class CompactRow(Row):
    """one block of 1024 and three (block counts, the scan over them)"""
    name, query = "compact", "cppf_compact_workspace_bytes"
    entries = ("cppf_compact_mask",)
    shapes = dict(small=dict(n=1000), large=dict(n=2 * 1024 + 5))
    axes = ("n",)

    def q(self, n):
        return L().cppf_compact_workspace_bytes(int(n))

    def inputs(self, p, dev):
        return dict(mask=T((np.random.default_rng(41).random(p["n"]) < 0.3).astype(np.uint8), dev))

    def run(self, inp, p, regions, short=False):
        dev = inp["mask"].device
        o = Outs(dev)
        surv, count = o.new("surv", p["n"], I32), o.new("count", 1, I32)
        return [call("cppf_compact_mask", dev, inp["mask"], p["n"], surv, count, *regions[0], ok=(self.refusal,))], o


def _tail_inputs(rng, N, P, n_sel, S, dev):
    pc, nrm = _cloud(rng, N)
    sph = rng.standard_normal((S, 3))
    sph /= np.linalg.norm(sph, axis=-1, keepdims=True)
    return dict(pc=T(pc, dev), nrm=T(nrm, dev), idx=T(rng.integers(0, N, (P, 2)).astype(np.int32), dev),
                sel=T(np.sort(rng.choice(P, n_sel, replace=False)).astype(np.int32), dev), n_sel=T(np.array([n_sel], np.int32), dev),
                heads=T(rng.standard_normal((P, 8)).astype(np.float32), dev), sphere=T(sph, dev),
                counts=T(rng.integers(0, 50, 2 * S).astype(np.int32), dev), best_dir=T(sph[3].copy(), dev))


class ReduceRow(Row):
    """the two-kernel reductions: one block's worth of survivors, and many blocks of partials"""
    name, query = "reduce", "cppf_reduce_workspace_bytes"
    entries = ("cppf_axis_sign", "cppf_scale_sum", "cppf_scale_exp_sum")
    shapes = dict(small=dict(N=100, P=300, n_sel=200), large=dict(N=500, P=70000, n_sel=66000))

    def q(self):
        return L().cppf_reduce_workspace_bytes()

    def inputs(self, p, dev):
        return _tail_inputs(np.random.default_rng(42), p["N"], p["P"], p["n_sel"], 16, dev)

    def run(self, inp, p, regions, short=False):
        dev, h = inp["pc"].device, inp["heads"]
        o = Outs(dev)
        sign, ssum, esum = o.new("sign", 3, F64), o.new("scale", 4, F64), o.new("scale_exp", 4, F64)
        return [call("cppf_axis_sign", dev, inp["pc"], inp["nrm"], inp["idx"], inp["sel"], inp["n_sel"], p["P"], h.data_ptr() + 8, 8,
                     inp["best_dir"], sign, *regions[0], ok=(self.refusal,)),
                call("cppf_scale_sum", dev, h.data_ptr() + 16, 8, inp["sel"], inp["n_sel"], p["P"], ssum, *regions[0], ok=(self.refusal,)),
                call("cppf_scale_exp_sum", dev, h.data_ptr() + 16, 8, inp["sel"], inp["n_sel"], p["P"], esum, *regions[0],
                     ok=(self.refusal,))], o


class PoseSumsRow(Row):
    """fewer than 256 survivors (one workgroup), and more than 65 536 (the stride loop runs; the ticket elects the last block)"""
    name, query = "pose_sums", "cppf_pose_sums_workspace_bytes"
    entries = ("cppf_pose_sums",)
    shapes = dict(small=dict(N=100, P=300, n_sel=200), large=dict(N=500, P=70000, n_sel=66000))

    def q(self):
        return L().cppf_pose_sums_workspace_bytes()

    def inputs(self, p, dev):
        return _tail_inputs(np.random.default_rng(43), p["N"], p["P"], p["n_sel"], 16, dev)

    def run(self, inp, p, regions, short=False):
        dev, h, S = inp["pc"].device, inp["heads"], 16
        o = Outs(dev)
        best_idx, best_dir, sign, scale = o.new("best_idx", 2, I64), o.new("best_dir", 6, F64), o.new("sign", 6, F64), o.new("scale", 4, F64)
        ticket = o.new("ticket", 1, I32, zero=True)             # zero before the first call and left at zero
        return [call("cppf_pose_sums", dev, inp["pc"], inp["nrm"], inp["idx"], inp["sel"], inp["n_sel"], p["P"], h.data_ptr() + 8, 8, 2,
                     inp["counts"], S, S, inp["sphere"], h.data_ptr() + 16, 8, best_idx, best_dir, sign, scale, *regions[0], ticket,
                     ok=(self.refusal,))], o


TAIL_SPHERE = 64


def _sorted_sphere(S):
    """S unit vectors with a descending y column (the Fibonacci sphere's order)"""
    y = 1.0 - 2.0 * (np.arange(S) + 0.5) / S
    r, phi = np.sqrt(1.0 - y * y), np.arange(S) * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], -1)


def tail0_layout(P, S=TAIL_SPHERE):
    """the region launch 1 zeroes, as cppf_amd.inference.PoseWorkspace lays it out: record 176 B | counts i32[2][S] | ticket 16 B |
    survivors per chunk of 1024 pairs -> (bytes, offset of the ticket)"""
    c0 = 176 + ((2 * S * 4 + 15) & ~15)
    return c0 + 16 + ((4 * ((P + 1023) // 1024) + 15) & ~15), c0


class PoseTailRow(Row):
    """cppf_pose_tail_batch takes its scratch through CppfPoseTailItem: per item the region launch 1 zeroes (tail0: the record, the
    sphere-bin counts, the ticket, the chunk counts), the pose-sums partials and the per-point table the first pass left.  Two
    items; regions [tail0, sums, table] of item 0, then of item 1.  tail0 is poisoned like any scratch: launch 1 must zero it.
    tail0 has no size query (the caller lays it out), so the refusal leg shortens the sums and the table regions, one at a time."""
    name, query = "pose_tail", None
    entries = ("cppf_pose_tail_batch",)
    shapes = dict(small=dict(N=64, P=700, dims=(12, 10, 9)), large=dict(N=300, P=2 * 1024 + 300, dims=(20, 18, 17)))

    def sizes(self, p):
        one = [tail0_layout(p["P"])[0], int(L().cppf_pose_sums_workspace_bytes()), int(PairMlpRow().q(N=p["N"]))]
        return one + one

    def refusals(self, p):
        return [[1], [2], [4], [5]]

    def inputs(self, p, dev):
        members = []
        for seed in (44, 45):
            rng = np.random.default_rng(seed)
            m = _pair_inputs(rng, p["N"], p["P"], dev)
            m["outputs"] = T(np.stack([rng.uniform(-0.1, 0.1, p["P"]), rng.uniform(0, 0.1, p["P"])], -1).astype(np.float32), dev)
            m["corner"] = T(np.zeros(3, np.float32), dev)
            d = p["dims"]
            m["argmax"] = T(np.array([(d[0] // 2 * d[1] + d[1] // 2) * d[2] + d[2] // 2], np.int64), dev)
            m["peak"] = T(np.array([17.5], np.float32), dev)
            members.append(m)
        sph = _sorted_sphere(TAIL_SPHERE)
        return dict(members=members, sph32=T(sph.astype(np.float32), dev), sph64=T(sph, dev))

    def run(self, inp, p, regions, short=False):
        dev, N, P = inp["sph32"].device, p["N"], p["P"]
        packed = _ppf_encoder(dev)._packed_weights(dev)
        o = Outs(dev)
        arr = (_lib.PoseTailItem * 2)()
        rcs, res = [], 0.3 / p["dims"][0]
        nbytes, c0 = tail0_layout(P)
        for i, m in enumerate(inp["members"]):
            tail0, sums, table = regions[3 * i:3 * i + 3]
            # the first pass leaves the per-point table (full size here: only the tail's own checks are under test)
            first = Outs(dev)
            call("cppf_pair_mlp_decode", dev, m["pc"], m["nrm"], m["feat"], m["idx"], 0, packed, N, FEAT, cints(PPFFCS), 3, P, OUT_DIM, 32, 36,
                 -0.5, 0.5, m["u_tr"], None, first.new("outputs", (P, 2), F32), None, table.ptr, table.mem.numel())
            it = arr[i]
            it.pc, it.nrm, it.feat, it.idx64, it.idx32 = m["pc"].data_ptr(), m["nrm"].data_ptr(), m["feat"].data_ptr(), None, m["idx"].data_ptr()
            it.outputs, it.u_rot = m["outputs"].data_ptr(), m["u_rot"].data_ptr()
            it.heads = o.new(f"heads{i}", (P, 8), F32, zero=True).data_ptr()
            it.corner, it.shape_dev, it.argmax_idx, it.peak = m["corner"].data_ptr(), None, m["argmax"].data_ptr(), m["peak"].data_ptr()
            it.packed, it.mlp_workspace, it.mlp_workspace_bytes, it.vote_workspace = packed.data_ptr(), table.ptr, table.nbytes, None
            it.rec, it.T32 = tail0.ptr, o.new(f"T32_{i}", 3, F32).data_ptr()
            it.tail0, it.tail0_bytes = tail0.ptr, nbytes
            it.mask, it.chunk_counts = o.new(f"mask{i}", P, U8).data_ptr(), tail0.ptr + c0 + 16
            it.surv, it.count = o.new(f"surv{i}", P, I32).data_ptr(), o.new(f"count{i}", 1, I32).data_ptr()
            it.counts, it.best_idx, it.ticket = tail0.ptr + 176, o.new(f"best_idx{i}", 2, I64).data_ptr(), tail0.ptr + c0
            it.sums_workspace, it.sums_workspace_bytes = sums.ptr, sums.nbytes
            it.n_points, it.n_pairs, it.res64, it.res, it.tol = N, P, res, res, 0.05
            it.gx, it.gy, it.gz = p["dims"]
            it.n_dirs, it.second_pass, it.record_out = 2, 1, None
        rcs.append(call("cppf_pose_tail_batch", dev, 2, arr, FEAT, cints(PPFFCS), 3, OUT_DIM, 32, 36, VOTE_ROTS, inp["sph32"], inp["sph64"],
                        TAIL_SPHERE, 1, float(np.float32(np.cos(np.radians(1.5)))), 10000, ok=(self.refusal,)))
        if not short:       # the record, the bin counts, the ticket (zero again) and the chunk counts live in tail0
            for i in range(2):
                o.new(f"tail0_{i}", nbytes, U8).copy_(regions[3 * i].mem[:nbytes])
        return rcs, o


# --- pre-processing --------------------------------------------------------------------------------------------------
def _kinv(fx, fy, cx, cy):
    return np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])).reshape(-1).copy()


def _depth_image(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    d = 900.0 + 3.0 * xx + 2.0 * yy + rng.uniform(0, 40, (H, W))
    d[rng.random((H, W)) < 0.1] = 0.0
    return d.astype(np.float32)


class BackprojectRow(Row):
    """one compaction chunk of 1024 pixels, and three"""
    name, query = "backproject", "cppf_backproject_workspace_bytes"
    entries = ("cppf_backproject",)
    shapes = dict(small=dict(H=30, W=30), large=dict(H=41, W=60))
    axes = ("H", "W")

    def q(self, H, W):
        return L().cppf_backproject_workspace_bytes(int(H), int(W))

    def inputs(self, p, dev):
        rng = np.random.default_rng(51)
        return dict(depth=T(_depth_image(rng, p["H"], p["W"]), dev), mask=T((rng.random((p["H"], p["W"])) < 0.6).astype(np.uint8), dev),
                    kinv=_kinv(50.0, 50.0, p["W"] / 2, p["H"] / 2))

    def run(self, inp, p, regions, short=False):
        dev, H, W = inp["depth"].device, p["H"], p["W"]
        o = Outs(dev)
        pts, pix, count = o.new("pts", (H * W, 3), F64), o.new("pix", H * W, I32), o.new("count", 1, I32)
        return [call("cppf_backproject", dev, inp["depth"], 0, inp["mask"], H, W, inp["kinv"], pts, pix, count, *regions[0],
                     ok=(self.refusal,))], o


class DepthPointsRow(BackprojectRow):
    name, query = "depth_points", "cppf_depth_points_workspace_bytes"
    entries = ("cppf_depth_points",)

    def q(self, H, W):
        return L().cppf_depth_points_workspace_bytes(int(H), int(W))

    def run(self, inp, p, regions, short=False):
        dev, H, W = inp["depth"].device, p["H"], p["W"]
        o = Outs(dev)
        pts, pix, count = o.new("pts", (H * W, 3), F64), o.new("pix", H * W, I32), o.new("count", 1, I32)
        return [call("cppf_depth_points", dev, inp["depth"], H, W, inp["kinv"], pts, pix, count, *regions[0], ok=(self.refusal,))], o


class VoxelDedupeRow(Row):
    """one chunk of 1024 points, and three; about half of the points share a voxel with an earlier one"""
    name, query = "voxel_dedupe", "cppf_voxel_dedupe_workspace_bytes"
    entries = ("cppf_voxel_dedupe",)
    shapes = dict(small=dict(n=500), large=dict(n=2 * 1024 + 77))
    axes = ("n",)

    def q(self, n):
        return L().cppf_voxel_dedupe_workspace_bytes(int(n))

    def inputs(self, p, dev):
        return dict(pc=T(np.random.default_rng(52).uniform(-0.1, 0.1, (p["n"], 3)).astype(np.float32), dev))

    def run(self, inp, p, regions, short=False):
        dev = inp["pc"].device
        o = Outs(dev)
        keep, count = o.new("keep", p["n"], I32), o.new("count", 1, I32)
        return [call("cppf_voxel_dedupe", dev, inp["pc"], p["n"], 0.02, keep, count, *regions[0], ok=(self.refusal,))], o


class FrameCloudRow(Row):
    """the frame stage of one instance: a frame of one pixel chunk, and one of three with a larger capacity"""
    name, query = "frame_cloud", "cppf_frame_cloud_workspace_bytes"
    entries = ("cppf_frame_cloud_dyn",)
    shapes = dict(small=dict(H=24, W=32, n_cap=256, k=8), large=dict(H=48, W=64, n_cap=1536, k=12))
    axes = ("H", "W", "n_cap", "k")

    def q(self, H, W, n_cap, k):
        return L().cppf_frame_cloud_workspace_bytes(int(H), int(W), int(n_cap), int(k))

    def inputs(self, p, dev):
        rng, H, W = np.random.default_rng(53), p["H"], p["W"]
        labels = np.zeros((H, W), np.uint8)
        labels[H // 4:3 * H // 4, W // 4:3 * W // 4] = 1 << 2          # H W / 4 pixels of the instance on bit 2
        labels[:H // 8] = 1 << 1                                        # another instance
        assert int((labels & 4 != 0).sum()) <= p["n_cap"]
        return dict(depth=T(_depth_image(rng, H, W), dev), labels=T(labels, dev), kinv=_kinv(60.0, 60.0, W / 2, H / 2))

    def run(self, inp, p, regions, short=False):
        dev, H, W, cap, k = inp["depth"].device, p["H"], p["W"], p["n_cap"], p["k"]
        o = Outs(dev)
        pc, nrm, corner = o.new("pc", (cap, 3), F32), o.new("nrm", (cap, 3), F32), o.new("corner", 3, F32)
        shape, nbrs = o.new("shape", 4, I32), o.new("nbrs", (cap, k), I32)
        return [call("cppf_frame_cloud_dyn", dev, inp["depth"], 0, inp["labels"], 1, 2, H, W, inp["kinv"], 1000.0, 0.004, k, k, cap, pc, nrm,
                     corner, shape, nbrs, *regions[0], ok=(self.refusal,))], o


# --- the scene paths -------------------------------------------------------------------------------------------------
def _weights(radius, sigma):
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 * (x / sigma) ** 2)
    return (w / w.sum()).copy()


def _scene_grid(rng, dims, peaks):
    g = rng.random(dims).astype(np.float32)
    for j in range(peaks):
        g[tuple(int(rng.integers(0, d)) for d in dims)] = 400.0 + 100.0 * j
    return g


class GaussianRow(Row):
    """lines shorter than the radius (reflect repeats) in a grid of a few cells, and a grid of several workgroups"""
    name, query = "gaussian_filter3d", "cppf_gaussian_filter3d_workspace_bytes"
    entries = ("cppf_gaussian_filter3d",)
    shapes = dict(small=dict(gx=5, gy=4, gz=3, radius=4), large=dict(gx=33, gy=20, gz=17, radius=4))
    axes = ("gx", "gy", "gz")

    def q(self, gx, gy, gz):
        return L().cppf_gaussian_filter3d_workspace_bytes(int(gx), int(gy), int(gz))

    def inputs(self, p, dev):
        return dict(grid=T(_scene_grid(np.random.default_rng(61), (p["gx"], p["gy"], p["gz"]), 3), dev), w=_weights(p["radius"], 1.0))

    def run(self, inp, p, regions, short=False):
        dev, d = inp["grid"].device, (p["gx"], p["gy"], p["gz"])
        o = Outs(dev)
        out = o.new("out", d, F32)
        return [call("cppf_gaussian_filter3d", dev, inp["grid"], out, *d, inp["w"], p["radius"], *regions[0], ok=(self.refusal,))], o


class SceneProposalsRow(Row):
    """the two grid copies and the table of one (max, first index) per 8^3 cells: one tile, and 3 x 3 x 3 ragged tiles"""
    name, query = "scene_proposals", "cppf_scene_proposals_workspace_bytes"
    entries = ("cppf_scene_proposals",)
    shapes = dict(small=dict(gx=8, gy=8, gz=8, peaks=1), large=dict(gx=20, gy=18, gz=17, peaks=4))
    axes = ("gx", "gy", "gz")

    def q(self, gx, gy, gz):
        return L().cppf_scene_proposals_workspace_bytes(int(gx), int(gy), int(gz))

    def inputs(self, p, dev):
        return dict(grid=T(_scene_grid(np.random.default_rng(62), (p["gx"], p["gy"], p["gz"]), p["peaks"]), dev), w=_weights(4, 1.0))

    def run(self, inp, p, regions, short=False):
        dev, d, K = inp["grid"].device, (p["gx"], p["gy"], p["gz"]), 8
        o = Outs(dev)
        loc, value, diff, count = o.new("loc", (K, 3), I32), o.new("value", K, F32), o.new("diff", K, F32), o.new("count", 1, I32)
        smoothed = o.new("smoothed", d, F32)
        return [call("cppf_scene_proposals", dev, inp["grid"], *d, inp["w"], 4, 2.0, 3, K, 32, loc, value, diff, count, smoothed, *regions[0],
                     ok=(self.refusal,))], o


def _segment_inputs(rng, N, P, K, dev):
    idx = rng.integers(0, N, (P, 2)).astype(np.int32)
    idx[rng.random(P) < 0.5] //= 8                      # a dense core: points that pass min_contrib
    bits = np.zeros(P, np.uint32)
    for k in range(K):
        bits |= (rng.random(P) < 0.4).astype(np.uint32) << np.uint32(k)
    masks = (rng.random((K, N)) < 0.4).astype(np.uint8)
    return dict(idx=T(idx, dev), bits=T(bits.view(np.int32), dev), surv=T((bits & 1).astype(np.uint8), dev), masks=T(masks, dev))


class SegmentInstanceRow(Row):
    """contrib / keep / counts: one chunk of 1024 pairs over one block of 256 points, and three ragged chunks over two blocks"""
    name, query = "segment_instance", "cppf_segment_instance_workspace_bytes"
    entries = ("cppf_segment_instance",)
    shapes = dict(small=dict(N=100, P=1000, K=1), large=dict(N=300, P=2 * 1024 + 5, K=1))
    axes = ("N", "P")

    def q(self, N, P):
        return L().cppf_segment_instance_workspace_bytes(int(N), int(P))

    def inputs(self, p, dev):
        return _segment_inputs(np.random.default_rng(63), p["N"], p["P"], p["K"], dev)

    def run(self, inp, p, regions, short=False):
        dev, N, P = inp["idx"].device, p["N"], p["P"]
        o = Outs(dev)
        pm, pairs, count = o.new("point_mask", N, U8), o.new("pairs", P, I32), o.new("count", 1, I32)
        return [call("cppf_segment_instance", dev, inp["idx"], inp["surv"], P, N, 3, pm, pairs, count, *regions[0], ok=(self.refusal,))], o


class SegmentInstancesRow(Row):
    """the [n_centers, n_points] table, the keep bits and the per-chunk counts: 2 proposals on one chunk of 1024 pairs, 5 on three"""
    name, query = "segment_instances", "cppf_segment_instances_workspace_bytes"
    entries = ("cppf_segment_instances",)
    shapes = dict(small=dict(N=100, P=1000, K=2), large=dict(N=300, P=2 * 1024 + 5, K=5))
    axes = ("N", "P", "K")

    def q(self, N, P, K):
        return L().cppf_segment_instances_workspace_bytes(int(N), int(P), int(K))

    def inputs(self, p, dev):
        return _segment_inputs(np.random.default_rng(64), p["N"], p["P"], p["K"], dev)

    def run(self, inp, p, regions, short=False):
        dev, N, P, K = inp["idx"].device, p["N"], p["P"], p["K"]
        o = Outs(dev)
        pm, pairs, offsets = o.new("point_masks", (K, N), U8), o.new("pairs", P * K, I32), o.new("offsets", K + 1, I32)
        return [call("cppf_segment_instances", dev, inp["idx"], inp["bits"], P, N, K, 3, pm, pairs, P * K, offsets, *regions[0],
                     ok=(self.refusal,))], o


class ProposalSupportRow(Row):
    """one membership word per point; a short workspace is CPPF_EINVAL (the header lists it with the argument errors)"""
    name, query = "proposal_support", "cppf_proposal_support_workspace_bytes"
    entries = ("cppf_proposal_support",)
    refusal = EINVAL
    shapes = dict(small=dict(N=100, P=1000, K=2), large=dict(N=300, P=2 * 1024 + 5, K=5))
    axes = ("N",)

    def q(self, N):
        return L().cppf_proposal_support_workspace_bytes(int(N))

    def inputs(self, p, dev):
        return _segment_inputs(np.random.default_rng(65), p["N"], p["P"], p["K"], dev)

    def run(self, inp, p, regions, short=False):
        dev, N, P, K = inp["idx"].device, p["N"], p["P"], p["K"]
        o = Outs(dev)
        counts = o.new("counts", (K, 4), I32)
        return [call("cppf_proposal_support", dev, inp["idx"], inp["bits"], inp["masks"], P, N, K, counts, *regions[0], ok=(self.refusal,))], o


# --- meshes ----------------------------------------------------------------------------------------------------------
RW, RH, RF = 40, 24, 40.0        # a 40 x 24 image: 3 x 2 tiles of 16 x 16, the right column and the bottom row ragged


def _px(c, r, d=1.0):
    """camera-frame vertex (the camera looks down -z) that projects to column c, row r (from the top)"""
    return [(c - RW / 2) / RF * d, (RH / 2 - r) / RF * d, -d]


def _tri_mesh():
    return np.array([_px(3, 3), _px(3, 9), _px(10, 6)]), np.array([[0, 1, 2]], np.int32)          # inside tile (0, 0)


def _cover_mesh():
    """a quad over the whole image at depth 2 and three triangles in front of it"""
    v = [_px(-2, -2, 2.0), _px(-2, RH + 2, 2.0), _px(RW + 2, RH + 2, 2.0), _px(RW + 2, -2, 2.0),
         _px(14, 2), _px(14, 20), _px(34, 12), _px(20, 14, 1.5), _px(20, 23, 1.5), _px(39, 22, 1.5), _px(1, 15, 0.7), _px(1, 23, 0.7),
         _px(18, 19, 0.7)]
    return np.array(v), np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], np.int32)


class RasterRow(Row):
    """a mesh that touches one tile, and one that touches every tile of the image (tile counts, cursors, the bin list)"""
    name, query = "raster", "cppf_raster_workspace_bytes"
    entries = ("cppf_raster_depth",)
    shapes = dict(small=dict(mesh="tri", F=1, bins=16), large=dict(mesh="cover", F=5, bins=64))
    axes = ("F", "W", "H", "bins")

    def q(self, F, W=RW, H=RH, bins=16):
        return L().cppf_raster_workspace_bytes(int(F), int(W), int(H), int(bins))

    def qargs(self, p):
        return dict(F=p["F"], W=RW, H=RH, bins=p["bins"])

    def inputs(self, p, dev):
        v, f = _tri_mesh() if p["mesh"] == "tri" else _cover_mesh()
        assert f.shape[0] == p["F"]
        return dict(v=T(v, dev), f=T(f, dev))

    def run(self, inp, p, regions, short=False):
        dev = inp["v"].device
        o = Outs(dev)
        depth = o.new("depth", (RH, RW), F32)
        return [call("cppf_raster_depth", dev, inp["v"], inp["v"].shape[0], inp["f"], p["F"], None, RF, RF, RW, RH, 0.05, 0, depth, p["bins"],
                     1, *regions[0], ok=(self.refusal,))], o


class RasterInstancesRow(Row):
    """one instance of one mesh in one tile; five instances of two meshes over every tile (the instance scan, the host tables
    copied into the workspace)"""
    name, query = "raster_instances", "cppf_raster_instances_workspace_bytes"
    entries = ("cppf_raster_instances",)
    shapes = dict(small=dict(K=1, Q=1, M=1, bins=16), large=dict(K=5, Q=17, M=2, bins=128))
    axes = ("K", "Q", "M", "W", "H", "bins")

    def q(self, K, Q, M, W=RW, H=RH, bins=16):
        return L().cppf_raster_instances_workspace_bytes(int(K), int(Q), int(M), int(W), int(H), int(bins))

    def qargs(self, p):
        return dict(K=p["K"], Q=p["Q"], M=p["M"], W=RW, H=RH, bins=p["bins"])

    def inputs(self, p, dev):
        (tv, tf), (cv, cf) = _tri_mesh(), _cover_mesh()
        if p["M"] == 1:
            v, f, vo, fo, inst = tv, tf, [0, 3], [0, 1], [0]
        else:
            v, f, vo, fo, inst = np.concatenate([tv, cv]), np.concatenate([tf, cf]), [0, 3, 3 + len(cv)], [0, 1, 1 + len(cf)], [1, 0, 1, 0, 1]
        mvs = np.tile(np.eye(4)[:3].reshape(-1), (p["K"], 1))
        mvs[:, 3] += 0.05 * np.arange(p["K"])                          # x shifts
        mvs[:, 11] -= 0.1 * np.arange(p["K"])                          # and further away
        assert sum(fo[m + 1] - fo[m] for m in inst) == p["Q"]
        return dict(v=T(v, dev), f=T(f, dev), vo=np.array(vo, np.int64), fo=np.array(fo, np.int64), inst=np.array(inst, np.int32), mvs=mvs.copy())

    def run(self, inp, p, regions, short=False):
        dev = inp["v"].device
        o = Outs(dev)
        depth, labels = o.new("depth", (RH, RW), F32), o.new("labels", (RH, RW), I32)
        return [call("cppf_raster_instances", dev, inp["v"], inp["f"], inp["vo"], inp["fo"], p["M"], inp["inst"], inp["mvs"], p["K"], RF, RF, RW,
                     RH, 0.05, 0, depth, labels, p["bins"], 1, *regions[0], ok=(self.refusal,))], o


def _grid_mesh(rng, nx, ny):
    xs, ys = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing="ij")
    v = np.stack([xs, ys, 0.1 * rng.random(xs.shape)], -1).reshape(-1, 3)
    i = (np.arange(nx)[:, None] * (ny + 1) + np.arange(ny)[None]).reshape(-1)
    f = np.concatenate([np.stack([i, i + ny + 1, i + 1], -1), np.stack([i + 1, i + ny + 1, i + ny + 2], -1)])
    return v, f.astype(np.int32)


class SurfaceSampleRow(Row):
    """one mesh of 8 faces (the serial chain), and three meshes one of which has more than 1024 faces (two faces per block)"""
    name, query = "surface_sample", "cppf_surface_sample_workspace_bytes"
    entries = ("cppf_surface_sample_batch",)
    shapes = dict(small=dict(M=1, F=8, n=100), large=dict(M=3, F=8 + 1152 + 18, n=700))
    axes = ("M", "F")

    def q(self, M, F):
        return L().cppf_surface_sample_workspace_bytes(int(M), int(F))

    def valid(self, M, F):  # every mesh has at least one face
        return 1 <= M <= F

    def inputs(self, p, dev):
        rng = np.random.default_rng(71)
        meshes = [_grid_mesh(rng, 2, 2)] + ([_grid_mesh(rng, 24, 24), _grid_mesh(rng, 3, 3)] if p["M"] == 3 else [])
        vo = np.concatenate([[0], np.cumsum([m[0].shape[0] for m in meshes])]).astype(np.int64)
        fo = np.concatenate([[0], np.cumsum([m[1].shape[0] for m in meshes])]).astype(np.int64)
        assert fo[-1] == p["F"]
        return dict(v=T(np.concatenate([m[0] for m in meshes]), dev), f=T(np.concatenate([m[1] for m in meshes]), dev), vo=vo, fo=fo)

    def run(self, inp, p, regions, short=False):
        dev, M, n = inp["v"].device, p["M"], p["n"]
        o = Outs(dev)
        pts, fid, status = o.new("points", (M, n, 3), F64), o.new("face_ids", (M, n), I32), o.new("status", M, I32)
        return [call("cppf_surface_sample_batch", dev, inp["v"], inp["f"], inp["vo"], inp["fo"], M, n, 77, 0, pts, fid, status, *regions[0],
                     ok=(self.refusal,))], o


class MeshVoteStatsRow(Row):
    """partial maxima per (mesh, block of 256 pairs): one mesh whose two blocks take their pairs in one trip, and 32 meshes at the
    cap of ceil(4096 / 32) = 128 blocks each, one pair block more than that, so that the stride loop runs a second trip"""
    name, query = "mesh_vote_stats", "cppf_mesh_vote_stats_workspace_bytes"
    entries = ("cppf_mesh_vote_stats_batch",)
    shapes = dict(small=dict(M=1, n=100, pairs=500), large=dict(M=32, n=300, pairs=128 * 256 + 5))
    axes = ("n", "pairs")   # M: see test_scratch_contract_cpu.test_mesh_vote_stats_query_in_the_mesh_count

    def q(self, n, pairs, M):
        return L().cppf_mesh_vote_stats_workspace_bytes(int(M), int(n), int(pairs))

    def qargs(self, p):
        return dict(M=p["M"], n=p["n"], pairs=p["pairs"])

    def inputs(self, p, dev):
        return dict(points=T(np.random.default_rng(72).standard_normal((p["M"], p["n"], 3)), dev))

    def run(self, inp, p, regions, short=False):
        dev, M = inp["points"].device, p["M"]
        o = Outs(dev)
        stats, status = o.new("stats", (M, 6), F64), o.new("status", M, I32)
        return [call("cppf_mesh_vote_stats_batch", dev, inp["points"], M, p["n"], p["pairs"], 78, 0, stats, status, *regions[0],
                     ok=(self.refusal,))], o


# --- evaluation ------------------------------------------------------------------------------------------------------
def _boxes(rng, m, side):
    RT = np.tile(np.eye(4), (m, 1, 1))
    a = rng.uniform(0, 2 * np.pi, m)
    RT[:, 0, 0], RT[:, 0, 2], RT[:, 2, 0], RT[:, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    RT[:, :3, 3] = rng.uniform(-0.5 * side, 0.5 * side, (m, 3))
    return RT, rng.uniform(0.5, 1.5, (m, 3))


class PoseEvalPairsRow(Row):
    """the work-item offsets: plain pairs only, and a list with swept pairs (20 items each)"""
    name, query = "pose_eval_pairs", "cppf_pose_eval_pairs_workspace_bytes"
    entries = ("cppf_pose_eval_pairs",)
    shapes = dict(small=dict(M=50, swept=0), large=dict(M=3000, swept=700))
    axes = ("M",)

    def q(self, M):
        return L().cppf_pose_eval_pairs_workspace_bytes(int(M))

    def inputs(self, p, dev):
        rng, M, nb = np.random.default_rng(81), p["M"], 40
        (a, sa), (b, sb) = _boxes(rng, nb, 2.0), _boxes(rng, nb, 2.0)
        sweep = np.zeros(M, np.int32)
        sweep[rng.permutation(M)[:p["swept"]]] = 1
        return dict(a=T(a, dev), sa=T(sa, dev), b=T(b, dev), sb=T(sb, dev), up=T((rng.random(nb) < 0.5).astype(np.int32), dev),
                    pairs=T(rng.integers(0, nb, (M, 2)).astype(np.int32), dev), sweep=T(sweep, dev), nb=nb)

    def run(self, inp, p, regions, short=False):
        dev, M, nb = inp["a"].device, p["M"], inp["nb"]
        o = Outs(dev)
        iou, err = o.new("iou", M, F64), o.new("err", (M, 2), F64)
        return [call("cppf_pose_eval_pairs", dev, inp["a"], inp["sa"], nb, inp["b"], inp["sb"], inp["up"], nb, inp["pairs"], inp["sweep"], M, iou,
                     err, *regions[0], ok=(self.refusal,))], o


class BoxNmsRow(Row):
    """one group of 10 boxes (one word per bit-matrix row), and three groups -- one empty, one of 130 boxes (three words per row)"""
    name, query = "box_nms", "cppf_box_nms_workspace_bytes"
    entries = ("cppf_box_nms_batch",)
    shapes = dict(small=dict(n=10, G=1, sizes=(10,)), large=dict(n=200, G=3, sizes=(70, 0, 130)))
    axes = ("n", "G")

    def q(self, n, G):
        return L().cppf_box_nms_workspace_bytes(int(n), int(G))

    def inputs(self, p, dev):
        rng = np.random.default_rng(82)
        RT, scales = _boxes(rng, p["n"], 3.0)
        return dict(RT=T(RT, dev), scales=T(scales, dev), scores=T(rng.integers(0, 7, p["n"]).astype(np.float64), dev),
                    off=np.concatenate([[0], np.cumsum(p["sizes"])]).astype(np.int32))

    def run(self, inp, p, regions, short=False):
        dev, n, G = inp["RT"].device, p["n"], p["G"]
        o = Outs(dev)
        pick, n_pick = o.new("pick", n, I32), o.new("n_pick", G, I32)
        iou = o.new("iou", sum(m * (m - 1) // 2 for m in p["sizes"]), F64)
        return [call("cppf_box_nms_batch", dev, inp["RT"], inp["scales"], inp["scores"], n, inp["off"], G, 0.25, pick, n_pick, iou, *regions[0],
                     ok=(self.refusal,))], o


ROWS = [VoteRow(), VoteDynRow(), PairMlpRow(), PairMlpBackwardRow(), PointEncoderRow(), PointEncoderBackwardRow(), CompactRow(),
        ReduceRow(), PoseSumsRow(), PoseTailRow(), FrameCloudRow(), BackprojectRow(), VoxelDedupeRow(), GaussianRow(), SceneProposalsRow(),
        SegmentInstanceRow(), SegmentInstancesRow(), RasterRow(), RasterInstancesRow(), DepthPointsRow(), SurfaceSampleRow(),
        MeshVoteStatsRow(), PoseEvalPairsRow(), BoxNmsRow(), ProposalSupportRow()]
BY_NAME = {r.name: r for r in ROWS}

# size queries of the header without a row, each with its reason (at most three; none of MUST_COVER)
EXCLUDED = {}

MUST_COVER = (
    "cppf_vote_workspace_bytes", "cppf_vote_workspace_bytes_dyn_pairs", "cppf_pair_mlp_workspace_bytes",
    "cppf_pair_mlp_backward_workspace_bytes", "cppf_point_encoder_workspace_bytes", "cppf_point_encoder_backward_workspace_bytes",
    "cppf_compact_workspace_bytes", "cppf_reduce_workspace_bytes", "cppf_pose_sums_workspace_bytes", "cppf_frame_cloud_workspace_bytes",
    "cppf_backproject_workspace_bytes", "cppf_voxel_dedupe_workspace_bytes", "cppf_gaussian_filter3d_workspace_bytes",
    "cppf_scene_proposals_workspace_bytes", "cppf_segment_instance_workspace_bytes", "cppf_segment_instances_workspace_bytes",
    "cppf_raster_workspace_bytes", "cppf_raster_instances_workspace_bytes", "cppf_depth_points_workspace_bytes",
    "cppf_surface_sample_workspace_bytes", "cppf_mesh_vote_stats_workspace_bytes", "cppf_pose_eval_pairs_workspace_bytes",
    "cppf_box_nms_workspace_bytes", "cppf_proposal_support_workspace_bytes")
