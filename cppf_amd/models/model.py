"""Drop-in for the pair-encoder half of the reference's models/model.py.

`ResLayer` and `PPFEncoder` keep the reference's constructor signatures, parameter names and shapes
(models/model.py:8-31, 80-87), so reference checkpoints load with `load_state_dict`
(nocs/inference.py:88), and the same call signatures (models/model.py:89-91, 117):

    PPFEncoder(ppffcs, out_dim)
    .forward(pc[1,N,3], pc_normal[1,N,3], feat[1,N,F], dist=None, idxs=None) -> f32[1,P,out_dim]
    .forward_with_idx(pc[N,3], pc_normal[N,3], feat[N,F], idxs[P,2])        -> f32[P,out_dim]

Under `torch.no_grad()` (inference, nocs/inference.py:179-182) the whole of forward_with_idx -- PPF
construction, gather/concat, three ResLayers and the final linear -- is one HIP kernel
(csrc/pair_mlp.hip).  When autograd needs the graph (train.py:66,91) and the shape is the standard one
(ppffcs [84,32,32,16]) the forward is the same HIP kernel wrapped in an autograd.Function whose backward is
csrc/pair_mlp_bwd.hip (gradients of every parameter and of `feat`); other
shapes evaluate the composite of torch ops.

`PointEncoder` (SPRIN, models/model.py:36-78) produces the per-point `feat` the pair encoder gathers:
    PointEncoder(k, spfcs, out_dim, num_layers=2, num_nbr_feats=2)
    .forward(pc[1,N,3], pc_normal[1,N,3], dist[1,N,N])      -> f32[1,N,out_dim + out_dim//4]
    .forward_nbrs(pc, pc_normal, nbrs_idx[1,N,k])           -> same
Under `no_grad` it is kNN selection + one fused HIP kernel per layer (csrc/sprin.hip); `dist=None` is
accepted as an extension and selects neighbours from exact squared distances without an N x N matrix.
"""
import ctypes as C
import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._torch_util import call, canon, dev_tensor, fill, require_cuda, scratch, workspace
from .sprin import GlobalInfoProp, SparseSO3Conv, pack_point_encoder

__all__ = ["ResLayer", "PPFEncoder", "PointEncoder"]


class ResLayer(nn.Module):
    """models/model.py:8-31: fc1 -> relu -> fc2, plus fc0(x) (or x when dim_in == dim_out)."""

    def __init__(self, dim_in, dim_out, bn=False):
        super().__init__()
        assert bn is False
        self.fc1 = nn.Linear(dim_in, dim_out)
        self.fc2 = nn.Linear(dim_out, dim_out)
        self.fc0 = nn.Linear(dim_in, dim_out) if dim_in != dim_out else None

    def forward(self, x):
        x_res = x if self.fc0 is None else self.fc0(x)
        return self.fc2(F.relu(self.fc1(x))) + x_res


def _params_of(module):
    """The module's parameters as a cached list.  nn.Module.parameters() walks the module tree on every call (~100 us for
    these encoders, several times per training step); the Parameter objects themselves are stable: .to() / .cuda() /
    load_state_dict() swap or fill their data in place, and the encoders' structure is fixed by their constructors.
    Code that REPLACES a Parameter object or a submodule afterwards must call the encoder's invalidate()."""
    plist = module.__dict__.get("_cppf_plist")
    if plist is None:
        plist = list(module.parameters())
        module.__dict__["_cppf_plist"] = plist
    return plist


_STREAM_STATE = weakref.WeakKeyDictionary()   # encoder -> {"readers": {stream: event}, "image_ev": (event, stream, generation)}


class _DeviceWeights:
    """What both encoders share about their device-side weight images.

    The HIP kernels read a lane-ordered IMAGE of the parameters, rebuilt when a parameter changes.  A change is detected
    through (data_ptr, _version) of every Parameter -- what optimizers, load_state_dict(), .to() and any in-place torch
    op on the Parameter update.  Writes that bypass the version counter (`p.data.copy_()`, `p.data.mul_()`, EMA / weight
    surgery through `.data`) are invisible to it: call `invalidate()` after them.  The image is rebuilt IN PLACE (same
    device buffer) whenever size and device allow, so captured hipGraphs that baked its address in stay valid and pick
    the new weights up at their next replay (inference.CenterPipeline re-checks before every replay)."""

    def invalidate(self):
        """Forget every cached view of the parameters (weight images, flat copies, parameter lists)."""
        self.__dict__["_cppf_epoch"] = self.__dict__.get("_cppf_epoch", 0) + 1
        for k in ("_cppf_plist", "_cppf_ordered", "_cppf_transposed"):
            self.__dict__.pop(k, None)

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() / .float(): parameters may move or be re-created
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate()
        return out

    def _param_key(self, device):
        return (str(device), self.__dict__.get("_cppf_epoch", 0)) + tuple((p.data_ptr(), p._version) for p in _params_of(self))

    # ------------------------------------------------------------------ precision and the image of each
    # An encoder supplies: _ENTRY (the prefix of its C entry points), _image_words(precision) (the image's size in 4-byte words, 0:
    # no kernel serves this encoder in that precision), _no_kernel(precision) (the refusal's text) and _pack_image(dev, buf) (pack
    # the image of the current precision into `buf`, on the device where it can, and return what _packed_weights() hands out).
    @property
    def precision(self):
        """"fp32" (the default: bit for bit the oracle's arithmetic) or "bf16" (set_precision)"""
        return self.__dict__.get("_cppf_precision", "fp32")

    def set_precision(self, precision):
        """Choose the arithmetic of the inference kernels: "fp32" (exact fp32 MFMAs) or "bf16" (the hidden layers as bf16 x bf16
        products accumulated in fp32; which layers stay fp32 is the encoder's, see its class).  bf16 is inference only (the backward
        stays fp32: a bf16 encoder asked for gradients raises CppfError) and serves the architecture the fp32 MFMA kernel serves
        (no fall-back to fp32).  Each precision keeps its own weight image; captured pipelines capture again after a switch.
        Returns self."""
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        if precision == "bf16" and self._image_words(precision) == 0:
            raise _lib.CppfError(self._no_kernel(precision))
        self.__dict__["_cppf_precision"] = precision
        return self

    def _entry(self, name):
        """the C entry point of the current precision: <_ENTRY>_<name> or <_ENTRY>_bf16_<name>"""
        return f"{self._ENTRY}_bf16_{name}" if self.precision == "bf16" else f"{self._ENTRY}_{name}"

    def _current_image(self):
        """what _packed_weights() last returned for the current precision, as it is now (None before its first pack)"""
        hit = self.__dict__.get("_cppf_images", {}).get(self.precision)
        return None if hit is None else hit[2]

    def _packed_weights(self, device):
        """The weight image for the HIP kernels of the current precision (fp32: a float32 tensor, bf16: an int32 tensor of words),
        rebuilt when a parameter changes.  Each precision has its own buffer and key; a rebuild rewrites the buffer in place when
        device, size and type allow, ordered against readers on other streams."""
        prec = self.precision
        key = self._param_key(device)
        images = self.__dict__.setdefault("_cppf_images", {})       # precision -> (key, buffer, what the encoder hands out)
        hit = images.get(prec)
        if hit is not None and hit[0] == key:
            return hit[2]
        n = self._image_words(prec)
        if n == 0:
            raise _lib.CppfError(self._no_kernel(prec))
        dev, dtype = torch.device(device), torch.int32 if prec == "bf16" else torch.float32
        buf = None if hit is None else hit[1]
        if buf is not None and buf.device == dev and buf.numel() == n and buf.dtype == dtype:
            if dev.type == "cuda":
                self._image_rebuild_begins(dev)
        else:
            buf = torch.empty(n, dtype=dtype, device=dev)
        images[prec] = (key, buf, self._pack_image(dev, buf))
        if dev.type == "cuda":
            self._image_rebuilt(dev)
        return images[prec][2]

    # Several HIP streams may share one encoder (inference.CenterPipeline lanes, batch.BatchPoseRunner).  The image is rebuilt
    # in place on whichever stream notices the parameter change, so both directions are ordered with events: a rebuild waits for
    # every replay that was still reading the old image (`_note_image_read`), and a reader on another stream waits for the
    # rebuild before its next replay (`_await_image`).  A training loop on one stream pays one event record per re-pack.
    # (the events live outside the module: copy.deepcopy / pickling of an encoder must not meet a HIP event)
    def _stream_state(self):
        st = _STREAM_STATE.get(self)
        if st is None:
            st = _STREAM_STATE[self] = {"readers": {}, "image_ev": (None, None, 0)}
        return st

    def _image_rebuild_begins(self, dev):
        """called right before the weight image is rewritten in place on the current stream of `dev`"""
        readers = self._stream_state()["readers"]
        if readers:
            cur = torch.cuda.current_stream(dev)
            for sid, ev in readers.items():
                if sid != cur.cuda_stream:
                    cur.wait_event(ev)

    def _image_rebuilt(self, dev):
        """called right after the rebuild was enqueued: later readers on other streams wait for this event"""
        st = self._stream_state()
        # recorded after EVERY pack, also the very first one (no reader registered yet): a pipeline that is captured or replayed on
        # another stream right afterwards finds the key unchanged and would otherwise never learn that it has to wait
        if torch.cuda.is_current_stream_capturing():
            return                                   # (packs happen before a capture begins; an event record would become a graph node)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        st["image_ev"] = (ev, torch.cuda.current_stream(dev).cuda_stream, st["image_ev"][2] + 1)

    def _await_image(self, dev, seen_gen):
        """reader side, before a replay on the current stream: wait for the newest rebuild if this reader has not yet;
        returns the rebuild generation to remember"""
        ev, sid, gen = self._stream_state()["image_ev"]
        if ev is not None and gen != seen_gen:
            cur = torch.cuda.current_stream(dev)
            if cur.cuda_stream != sid:
                cur.wait_event(ev)
        return gen

    def _note_image_read(self, dev):
        """reader side, after a replay was enqueued on the current stream"""
        readers = self._stream_state()["readers"]
        cur = torch.cuda.current_stream(dev)
        ev = readers.get(cur.cuda_stream)
        if ev is None:
            ev = readers[cur.cuda_stream] = torch.cuda.Event()
        ev.record(cur)


class _PairMlpFunction(torch.autograd.Function):
    """forward_with_idx with a HIP backward (train.py:66,91).  Saves only the inputs; the backward kernel
    recomputes the forward.  Gradients: feat, then the parameters in `flatten_state_dict` order."""

    @staticmethod
    def forward(ctx, enc, pc, pc_normal, feat, idxs, *params):
        with torch.no_grad():
            out = enc._forward_device(pc, pc_normal, feat, idxs)
        ctx.enc = enc
        ctx.save_for_backward(pc, pc_normal, feat, idxs, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        enc = ctx.enc
        pc, nrm, feat, idxs, *params = ctx.saved_tensors
        dev = pc.device
        flat, offs_c = enc._flat_params(dev)                   # the forward's flat copy unless a parameter changed since
        dims = (C.c_int * len(enc.ppffcs))(*enc.ppffcs)
        L = _lib.lib()
        P, F_ = idxs.shape[0], feat.shape[1]
        grad_out = grad_out.detach().float().contiguous()
        gp = torch.empty_like(flat)
        gf = torch.zeros((feat.shape[0], F_), dtype=torch.float32, device=dev)
        need = L.cppf_pair_mlp_backward_workspace_bytes(P, feat.shape[0], F_, dims, len(enc.ppffcs) - 1, enc.out_dim)
        ws = workspace(max(int(need), 256), dev, "pair_mlp_bwd")
        pcc, nrmc, featc = (pc.detach().float().contiguous(), nrm.detach().float().contiguous(),
                            feat.detach().float().contiguous())
        call("cppf_pair_mlp_backward", dev, pcc, nrmc, featc, idxs, idxs.dtype == torch.int64, flat, offs_c, pc.shape[0], F_, dims,
             len(enc.ppffcs) - 1, P, enc.out_dim, grad_out, gp, gf, scratch(ws))
        grads, pos = [], 0
        for p in params:
            grads.append(gp[pos:pos + p.numel()].reshape(p.shape))
            pos += p.numel()
        return (None, None, None, gf if ctx.needs_input_grad[3] else None, None, *grads)


class _PointEncoderFunction(torch.autograd.Function):
    """PointEncoder.forward under autograd with a HIP backward (train.py:62-64,91): forward = the inference kernels
    (kNN from `dist` + SPRIN), backward = cppf_point_encoder_backward, which recomputes the forward per point.  Points
    and normals carry no gradient (train.py:58-60); gradients flow to the parameters, in `_ordered_params` order."""

    @staticmethod
    def forward(ctx, enc, pc, nrm, nbrs, *params):
        with torch.no_grad():
            # the per-point contraction [rank 32 x n_nbr_feats], kept for the backward
            mixed = torch.empty((pc.shape[0], 32 * enc.num_nbr_feats), dtype=torch.float32, device=pc.device)
            out = enc._forward_device(pc, nrm, nbrs, keep_contraction=mixed)
        ctx.enc = enc
        # the parameters are saved too: the backward recomputes the forward from the weight image of the CURRENT parameters,
        # so an in-place update between forward and backward must fail autograd's version check instead of giving
        # silently wrong gradients
        ctx.save_for_backward(pc, nrm, nbrs, out, mixed, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        enc = ctx.enc
        pc, nrm, nbrs, out, mixed = ctx.saved_tensors[:5]
        dev = pc.device
        packed, desc = enc._packed_weights(dev)
        hid = (C.c_int * len(desc["hidden"]))(*desc["hidden"])
        L = _lib.lib()
        N, k = nbrs.shape
        g = grad_out.detach().float().contiguous()
        n_nat = sum(p.numel() for p in enc._ordered_params())
        gp = torch.empty(n_nat, dtype=torch.float32, device=dev)
        ws = workspace(max(int(L.cppf_point_encoder_backward_workspace_bytes(N)), 256), dev, "point_encoder_bwd")
        call("cppf_point_encoder_backward", dev, pc, nrm, nbrs, N, k, packed, hid, len(desc["hidden"]), desc["rank"], desc["n_nbr_feats"],
             desc["n_out"], desc["n_glob"], enc.num_layers, out, mixed, g, gp, scratch(ws))
        grads, pos = [], 0
        for p, transposed in zip(enc._ordered_params(), enc._ordered_transposed()):
            v = gp[pos:pos + p.numel()]
            grads.append(v.reshape(p.shape[1], p.shape[0]).t() if transposed else v.reshape(p.shape))
            pos += p.numel()
        return (None, None, None, None, *grads)


class PointEncoder(_DeviceWeights, nn.Module):
    """models/model.py:36-78.  Same constructor, parameter names and call signatures as the reference."""

    def __init__(self, k, spfcs, out_dim, num_layers=2, num_nbr_feats=2):
        super().__init__()
        self.k = int(k)
        self.spfcs = [int(h) for h in spfcs]
        self.out_dim = int(out_dim)
        self.num_layers = int(num_layers)
        self.num_nbr_feats = int(num_nbr_feats)
        self.spconvs = nn.ModuleList([SparseSO3Conv(32, num_nbr_feats, out_dim, *spfcs)])
        self.aggrs = nn.ModuleList([GlobalInfoProp(out_dim, out_dim // 4)])
        for _ in range(num_layers - 1):
            self.spconvs.append(SparseSO3Conv(32, out_dim + out_dim // 4, out_dim, *spfcs))
            self.aggrs.append(GlobalInfoProp(out_dim, out_dim // 4))

    # ------------------------------------------------------------------ precision (this package: _DeviceWeights.set_precision)
    # "fp32": csrc/sprin.hip.  "bf16": csrc/sprin_bf16.hip -- gather, rifeat, layer 1 of the kernel-MLP and every LayerNorm in fp32
    # as before, layers 2..5 in bf16; the contraction, the outnet and GlobalInfoProp are the fp32 code.
    _ENTRY = "cppf_point_encoder"

    def _std_layers(self):
        return (self.spfcs == [32, 64, 32, 32] and self.out_dim == 32 and self.num_nbr_feats == 2
                and all(sc.layer_norm is not None for sc in self.spconvs))

    def _std_shape(self):
        return self._std_layers() and self.k <= 64

    def _desc(self):
        return dict(hidden=list(self.spfcs), rank=32, n_nbr_feats=self.num_nbr_feats, n_out=self.out_dim, n_glob=self.out_dim // 4,
                    num_layers=self.num_layers)

    def _shape_args(self):
        return ((C.c_int * len(self.spfcs))(*self.spfcs), len(self.spfcs), 32, self.num_nbr_feats, self.out_dim, self.out_dim // 4,
                self.num_layers)

    def _image_words(self, precision):
        L = _lib.lib()
        if precision == "bf16":
            return int(L.cppf_point_encoder_bf16_packed_bytes(*self._shape_args())) // 4 if self._std_shape() else 0
        # (a shape without an MFMA image keeps the natural block, and the forward says that no kernel serves it)
        return max(int(L.cppf_point_encoder_packed_floats(*self._shape_args())), sum(p.numel() for p in _params_of(self)))

    def _no_kernel(self, precision):
        return (f"no {precision} kernel for PointEncoder(k={self.k}, spfcs={self.spfcs}, out_dim={self.out_dim}, "
                f"num_nbr_feats={self.num_nbr_feats}): csrc/sprin_bf16.hip covers spfcs=[32,64,32,32], out_dim=32, "
                "num_nbr_feats=2, k<=64 (train.py:34); there is no fall-back to fp32")

    def _pack_image(self, dev, buf):
        """-> (image, desc).  fp32: the natural block, then the MFMA image; bf16: the natural block verbatim, then per layer the
        fp32 layer 1, the bf16 layers 2..5 and the fp32 vectors"""
        pack = self._entry("pack")
        if dev.type == "cuda" and self.num_layers == 1 and self._std_layers():
            # standard encoder: natural block by one torch.cat, image by a device kernel -- no host round trip, so a training
            # loop (weights change every step) stays on the stream
            nat = torch.cat([(p.detach().t() if tr else p.detach()).reshape(-1).float()
                             for p, tr in zip(self._ordered_params(), self._ordered_transposed())]).to(dev).contiguous()
            call(pack + "_device", dev, nat, *self._shape_args(), buf)
        else:
            sd = {k: v.detach().float().cpu().numpy() for k, v in self.state_dict().items()}
            image = torch.zeros(buf.numel(), dtype=buf.dtype)
            call(pack, None, pack_point_encoder(sd, self.num_layers)[0], *self._shape_args(), image)
            buf.copy_(image)
        return buf, self._desc()

    def _refuse_gradients(self, *inputs):
        if torch.is_grad_enabled() and (self.training or any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs)
                                        or any(p.requires_grad for p in _params_of(self))):
            raise _lib.CppfError("PointEncoder with precision 'bf16' is inference only (the backward kernels are fp32): call it in "
                                 "eval mode under torch.no_grad() (or with parameters and inputs that need no gradient), or "
                                 "set_precision('fp32') to train")

    # ------------------------------------------------------------------ reference signatures
    def forward(self, pc, pc_normal, dist=None):
        if self.precision == "bf16":
            self._refuse_gradients(pc, pc_normal)
            with torch.no_grad():
                pc2, nrm2 = self._check_inputs(pc, pc_normal)
                d2 = None if dist is None else self._check_dist(dist, pc2)
                return self._forward_device(pc2, nrm2, self.neighbours(pc2, d2)).reshape(*pc.shape[:-1], -1)
        if self._needs_graph(pc):
            if self._has_device_backward(pc, pc_normal):
                pc2, nrm2 = self._check_inputs(pc, pc_normal)
                d2 = None if dist is None else self._check_dist(dist, pc2)
                out = _PointEncoderFunction.apply(self, pc2, nrm2, self.neighbours(pc2, d2), *self._ordered_params())
                return out.reshape(*pc.shape[:-1], -1)
            if dist is None:
                dist = torch.cdist(pc, pc)
            nbrs = torch.topk(dist, self.k, largest=False, sorted=False)[1]          # models/model.py:47
            return self._composite(pc, pc_normal, nbrs)
        pc2, nrm2 = self._check_inputs(pc, pc_normal)
        if dist is not None:
            dist = self._check_dist(dist, pc2)
        return self._forward_device(pc2, nrm2, self.neighbours(pc2, dist)).reshape(*pc.shape[:-1], -1)

    def forward_nbrs(self, pc, pc_normal, nbrs_idx):
        if self.precision == "bf16":
            self._refuse_gradients(pc, pc_normal)
            with torch.no_grad():
                pc2, nrm2 = self._check_inputs(pc, pc_normal)
                return self._forward_device(pc2, nrm2, self._check_nbrs(nbrs_idx, pc2)).reshape(*pc.shape[:-1], -1)
        if self._needs_graph(pc):
            if self._has_device_backward(pc, pc_normal):
                pc2, nrm2 = self._check_inputs(pc, pc_normal)
                nbrs = self._check_nbrs(nbrs_idx, pc2)
                out = _PointEncoderFunction.apply(self, pc2, nrm2, nbrs, *self._ordered_params())
                return out.reshape(*pc.shape[:-1], -1)
            return self._composite(pc, pc_normal, nbrs_idx)
        pc2, nrm2 = self._check_inputs(pc, pc_normal)
        nbrs = self._check_nbrs(nbrs_idx, pc2)
        return self._forward_device(pc2, nrm2, nbrs).reshape(*pc.shape[:-1], -1)

    # ------------------------------------------------------------------ device path
    def neighbours(self, pc, dist=None):
        """i32[N,k]: rows of torch.topk(dist, k, largest=False) in ascending index order; without `dist`
        the keys are exact squared distances computed from pc."""
        N = pc.shape[0]
        if self.k > N:
            raise ValueError(f"k={self.k} neighbours requested from {N} points")
        nbrs = torch.empty((N, self.k), dtype=torch.int32, device=pc.device)
        call("cppf_knn", pc.device, pc, dist, N, self.k, nbrs)
        return nbrs

    def _forward_device(self, pc, nrm, nbrs, keep_contraction=None):
        N, k = nbrs.shape
        packed, desc = self._packed_weights(pc.device)
        hid = (C.c_int * len(desc["hidden"]))(*desc["hidden"])
        L = _lib.lib()
        W = desc["n_out"] + desc["n_glob"]
        out = torch.empty((N, W), dtype=torch.float32, device=pc.device)
        ws = workspace(L.cppf_point_encoder_workspace_bytes(N, desc["n_out"], desc["n_glob"], self.num_layers), pc.device,
                       "point_encoder")
        args = (pc, nrm, nbrs, N, k, packed, hid, len(desc["hidden"]), desc["rank"], desc["n_nbr_feats"], desc["n_out"], desc["n_glob"],
                self.num_layers, out)
        if keep_contraction is not None:   # training (fp32 only): the backward reuses the per-point contraction
            rc = call("cppf_point_encoder_forward_train", pc.device, *args, keep_contraction, scratch(ws), ok=(_lib.EUNSUPPORTED,))
        else:
            rc = call(self._entry("forward"), pc.device, *args, scratch(ws), ok=(_lib.EUNSUPPORTED,))
        if rc == _lib.EUNSUPPORTED:
            raise _lib.CppfError(f"no device kernel ({self.precision}) for PointEncoder(k={self.k}, spfcs={self.spfcs}, "
                                 f"out_dim={self.out_dim}): csrc/sprin.hip and csrc/sprin_bf16.hip cover spfcs=[32,64,32,32], "
                                 "out_dim=32, k<=64 (train.py:34)")
        return out

    # ------------------------------------------------------------------ internals
    def _needs_graph(self, pc):
        if not torch.is_grad_enabled():
            return False
        return pc.requires_grad or any(p.requires_grad for p in _params_of(self))

    def _has_device_backward(self, pc, pc_normal):
        """csrc/sprin_bwd.hip covers the one-layer standard encoder (train.py:34) when only the parameters need gradients"""
        return pc.is_cuda and self.num_layers == 1 and self._std_shape() and not pc.requires_grad and not pc_normal.requires_grad

    def _ordered_params(self):
        """parameters in the packed natural order of `pack_point_encoder` (one layer); cached like `_params_of`"""
        cached = self.__dict__.get("_cppf_ordered")
        if cached is not None:
            return cached
        ker = self.spconvs[0].kernel
        ps = []
        for i in range(0, len(ker) - 1, 3):
            ps += [ker[i].weight, ker[i].bias, ker[i + 1].weight, ker[i + 1].bias]
        ps += [ker[len(ker) - 1].weight, ker[len(ker) - 1].bias]
        sc = self.spconvs[0]
        ps += [sc.outnet.weight, sc.outnet.bias, sc.layer_norm.weight, sc.layer_norm.bias,
               self.aggrs[0].linear.weight, self.aggrs[0].linear.bias]
        self.__dict__["_cppf_ordered"] = ps
        return ps

    def _ordered_transposed(self):
        """which of `_ordered_params` are stored transposed in the packed layout (outnet.weight: [C][n_out])"""
        cached = self.__dict__.get("_cppf_transposed")
        if cached is None:
            cached = [p is self.spconvs[0].outnet.weight for p in self._ordered_params()]
            self.__dict__["_cppf_transposed"] = cached
        return cached

    def _composite(self, pc, pc_normal, nbrs_idx):
        """models/model.py:63-78 as torch ops (autograd path)."""
        gather = lambda t: torch.gather(t.unsqueeze(-3).expand(*t.shape[:-1], *t.shape[-2:]), -2,
                                        nbrs_idx[..., None].expand(*nbrs_idx.shape, t.shape[-1]))
        pc_nbrs = gather(pc)
        norm = torch.norm(pc_nbrs - pc.unsqueeze(-2), dim=-1, keepdim=True)
        cos = torch.sum(gather(pc_normal) * pc_normal.unsqueeze(-2), -1, keepdim=True)
        feat = self.aggrs[0](self.spconvs[0](pc_nbrs, torch.cat([norm, cos], -1), pc))
        for spconv, aggr in zip(self.spconvs[1:], self.aggrs[1:]):
            feat = aggr(spconv(pc_nbrs, gather(feat), pc))
        return feat

    def _check_inputs(self, pc, pc_normal):
        require_cuda()
        if not pc.is_cuda:
            raise _lib.CppfError("PointEncoder inference runs on a HIP device only (no CPU fallback); "
                                 "move the module and its inputs to cuda")
        if pc.shape[-1] != 3 or pc_normal.shape != pc.shape or pc.dim() not in (2, 3) or (pc.dim() == 3 and pc.shape[0] != 1):
            raise ValueError("pc / pc_normal must be [1,N,3] (or [N,3])")
        return (canon(pc, torch.float32, pc.device, "pc").reshape(-1, 3), canon(pc_normal, torch.float32, pc.device, "pc_normal").reshape(-1, 3))

    @staticmethod
    def _check_nbrs(nbrs_idx, pc2):
        """the caller's neighbour lists [..., N, k] (int32 / int64, any strides, on the cloud's device) as the i32[N,k] the
        kernels read"""
        nbrs = canon(nbrs_idx, (torch.int32, torch.int64), pc2.device, "nbrs_idx")
        return nbrs.reshape(pc2.shape[0], -1).to(torch.int32)

    @staticmethod
    def _check_dist(dist, pc2):
        """the caller's distance matrix [..., N, N] as the f32[N,N] the neighbour search reads, on the cloud's device"""
        if dist.shape[-2:] != (pc2.shape[0], pc2.shape[0]):
            raise ValueError(f"dist must be [..., N, N], got {tuple(dist.shape)}")
        return canon(dist, torch.float32, pc2.device, "dist").reshape(pc2.shape[0], pc2.shape[0])

    def forward_dyn(self, pc, pc_normal, n_dev, out=None, nbrs=None, nbrs_ready=False):
        """Shape-polymorphic forward for captured chains (cppf_knn_dyn + cppf_point_encoder_forward_dyn): pc / pc_normal are
        capacity-sized f32[n_cap,3] device tensors, `n_dev` a device i32 tensor whose first element is the number of valid
        points (>= k: the caller's duty).  Rows >= n of the result are left untouched.  Returns f32[n_cap, out_dim + out_dim//4].
        nbrs_ready: `nbrs` already holds the k-neighbour sets of the cloud (cppf_knn's output for the same k, e.g. left by
        cppf_frame_cloud_dyn, which fits the normals on them): the search is not repeated."""
        require_cuda()
        if self.precision == "bf16":
            self._refuse_gradients(pc, pc_normal)
        n_cap = pc.shape[0]
        packed, desc = self._packed_weights(pc.device)
        hid = (C.c_int * len(desc["hidden"]))(*desc["hidden"])
        L = _lib.lib()
        W = desc["n_out"] + desc["n_glob"]
        if out is None:
            out = torch.zeros((n_cap, W), dtype=torch.float32, device=pc.device)
        if nbrs is None:
            nbrs = torch.zeros((n_cap, self.k), dtype=torch.int32, device=pc.device)
        ws = workspace(L.cppf_point_encoder_workspace_bytes(n_cap, desc["n_out"], desc["n_glob"], self.num_layers), pc.device,
                       "point_encoder")
        if not nbrs_ready:
            call("cppf_knn_dyn", pc.device, pc, n_cap, n_dev, self.k, nbrs)
        rc = call(self._entry("forward_dyn"), pc.device, pc, pc_normal, nbrs, n_cap, n_dev, self.k, packed, hid, len(desc["hidden"]),
                  desc["rank"], desc["n_nbr_feats"], desc["n_out"], desc["n_glob"], self.num_layers, out, scratch(ws),
                  ok=(_lib.EUNSUPPORTED,))
        if rc == _lib.EUNSUPPORTED:
            raise _lib.CppfError(f"no device kernel ({self.precision}) for PointEncoder(k={self.k}, spfcs={self.spfcs}, "
                                 f"out_dim={self.out_dim})")
        return out


def point_encoder_forward_batch(members):
    """The point encoders of a chain's members in three launches (cppf_point_encoder_forward_batch) instead of three each.
    members: dicts(encoder, pc, nrm, n_dev, out, nbrs[, nbrs_ready]) as PointEncoder.forward_dyn takes them, 1..8 of them, encoders
    of the one-layer standard form with the same k (instances of different categories carry different weights).  -> [out per
    member], bit-equal to forward_dyn member by member; None when the members do not qualify (the caller then loops forward_dyn).
    The members share a precision (PointEncoder.set_precision): a mixed batch raises CppfError, and so does a bf16 batch the bf16
    kernel does not serve (no fall-back to fp32)."""
    require_cuda()
    e0 = members[0]["encoder"]
    for i, m in enumerate(members):
        if m["encoder"].precision != e0.precision:
            raise _lib.CppfError(f"the point encoders of one launch must share a precision: member 0 is {e0.precision!r}, member {i} "
                                 f"is {m['encoder'].precision!r} (PointEncoder.set_precision)")
        if e0.precision == "bf16":
            m["encoder"]._refuse_gradients(m["pc"], m["nrm"])
    if not 1 <= len(members) <= 8 or any(m["encoder"].num_layers != 1 or m["encoder"].k != e0.k or m["encoder"].spfcs != e0.spfcs
                                         or m["encoder"].out_dim != e0.out_dim or m["encoder"].num_nbr_feats != e0.num_nbr_feats
                                         for m in members):
        return None
    dev = members[0]["pc"].device
    L = _lib.lib()
    arr = (_lib.PointEncItem * len(members))()
    keep = []
    desc = None
    for i, m in enumerate(members):
        packed, desc = m["encoder"]._packed_weights(dev)
        n_cap = m["pc"].shape[0]
        ws = workspace(L.cppf_point_encoder_workspace_bytes(n_cap, desc["n_out"], desc["n_glob"], 1), dev, f"point_encoder{i}")
        fill(arr[i], dev, pc=m["pc"], nrm=m["nrm"], nbrs=m["nbrs"], out=m["out"], n_dev=m.get("n_dev"), packed=packed, workspace=scratch(ws),
             n_cap=n_cap, nbrs_ready=bool(m.get("nbrs_ready")))
        keep.append((packed, ws))
    hid = (C.c_int * len(desc["hidden"]))(*desc["hidden"])
    rc = call(e0._entry("forward_batch"), dev, len(members), arr, e0.k, hid, len(desc["hidden"]), desc["rank"],
              desc["n_nbr_feats"], desc["n_out"], desc["n_glob"], 1, ok=(_lib.EUNSUPPORTED,))
    if rc == _lib.EUNSUPPORTED and e0.precision == "bf16":
        raise _lib.CppfError(f"no bf16 device kernel for PointEncoder(k={e0.k}, spfcs={e0.spfcs}, out_dim={e0.out_dim}) (there is no "
                             "fall-back to fp32)")
    return None if rc == _lib.EUNSUPPORTED else [m["out"] for m in members]


class PPFEncoder(_DeviceWeights, nn.Module):
    def __init__(self, ppffcs, out_dim):
        super().__init__()
        self.ppffcs = [int(d) for d in ppffcs]
        self.out_dim = int(out_dim)
        self.res_layers = nn.ModuleList(
            ResLayer(self.ppffcs[i], self.ppffcs[i + 1]) for i in range(len(self.ppffcs) - 1))
        self.final = nn.Linear(self.ppffcs[-1], self.out_dim)
        self._flat = None
        self._flat_key = None

    # ------------------------------------------------------------------ precision (this package: _DeviceWeights.set_precision)
    # "fp32": csrc/pair_mlp.hip.  "bf16": csrc/pair_mlp_bf16.hip -- layer 0 in fp32 as before, every later layer in bf16, fp32 logits
    # and the unchanged fp32 decode (DESIGN.md "bf16 pair encoder"); the standard architecture only.
    _ENTRY = "cppf_pair_mlp"

    def _refuse_gradients(self, feat):
        if torch.is_grad_enabled() and (self.training or feat.requires_grad):
            raise _lib.CppfError("PPFEncoder with precision 'bf16' is inference only (the backward kernels are fp32): call it in eval "
                                 "mode on inputs that need no gradient, or set_precision('fp32') to train")

    # ------------------------------------------------------------------ reference signatures
    def forward(self, pc, pc_normal, feat, dist=None, idxs=None):
        if idxs is not None:                                   # models/model.py:90-91
            return self.forward_with_idx(pc[0], pc_normal[0], feat[0], idxs)[None]
        # Dense all-pairs branch (models/model.py:92-115; no caller in the reference): pair (i, j)
        # for every i, j, evaluated through the same sampled-pair path.  `dist` is not needed: the
        # pair kernel recomputes ||pc_i - pc_j|| itself.
        if pc.dim() != 3 or pc.shape[0] != 1:
            raise ValueError("dense forward supports batch size 1 (the reference asserts it, train.py:32)")
        n = pc.shape[1]
        ii, jj = torch.meshgrid(torch.arange(n, device=pc.device), torch.arange(n, device=pc.device), indexing="ij")
        allp = torch.stack([ii.reshape(-1), jj.reshape(-1)], -1)
        return self.forward_with_idx(pc[0], pc_normal[0], feat[0], allp).reshape(1, n, n, self.out_dim)

    def forward_with_idx(self, pc, pc_normal, feat, idxs):
        if self.precision == "bf16":
            self._refuse_gradients(feat)
            with torch.no_grad():
                return self._forward_device(pc, pc_normal, feat, self._as_index_tensor(idxs, self._device_of(pc)))
        if self._needs_graph(feat) and not self._has_device_backward(pc, feat):      # torch ops: wherever the tensors are
            return self._composite(pc, pc_normal, feat, self._as_index_tensor(idxs, pc.device))
        idxs = self._as_index_tensor(idxs, self._device_of(pc))
        if self._needs_graph(feat):
            return _PairMlpFunction.apply(self, pc, pc_normal, feat, idxs, *self._ordered_params())
        return self._forward_device(pc, pc_normal, feat, idxs)

    def _forward_device(self, pc, pc_normal, feat, idxs):
        pc, pc_normal, feat = self._check_inputs(pc, pc_normal, feat)
        P = idxs.shape[0]
        out = torch.empty((P, self.out_dim), dtype=torch.float32, device=pc.device)
        dims = (C.c_int * len(self.ppffcs))(*self.ppffcs)
        ws = self._scratch(pc, feat, dims)
        call(self._entry("forward"), pc.device, pc, pc_normal, feat, idxs, idxs.dtype == torch.int64, self._packed_weights(pc.device),
             pc.shape[0], feat.shape[1], dims, len(self.ppffcs) - 1, P, self.out_dim, out, scratch(ws))
        return out

    # ------------------------------------------------------------------ fused decode (this package)
    def forward_decode(self, pc, pc_normal, feat, idxs, u_tr, vote_range, u_rot=None, tr_num_bins=32,
                       rot_num_bins=36):
        """forward_with_idx fused with the decode of nocs/inference.py:185-188 (and :245-256 when
        u_rot is given): returns (outputs f32[P,2] = (mu, nu), heads f32[P,8] or None) without ever
        writing the [P,out_dim] logits.  u_* are uniforms in [0,1) standing in for torch.multinomial
        (negative = arg-max bin)."""
        idxs = self._as_index_tensor(idxs, self._device_of(pc))
        pc, pc_normal, feat = self._check_inputs(pc, pc_normal, feat)
        P = idxs.shape[0]
        u_tr = canon(u_tr, torch.float32, pc.device, "u_tr", (P, 2))
        u_rot = None if u_rot is None else canon(u_rot, torch.float32, pc.device, "u_rot", (P, 2))
        outputs = torch.empty((P, 2), dtype=torch.float32, device=pc.device)
        heads = torch.empty((P, 8), dtype=torch.float32, device=pc.device) if u_rot is not None else None
        dims = (C.c_int * len(self.ppffcs))(*self.ppffcs)
        ws = self._scratch(pc, feat, dims)
        if self.precision == "bf16":             # one list = the batch of one (no per-variant single entry points)
            item = self._item(_lib.PairMlpItem(), pc, pc_normal, feat, idxs, ws, u_tr=u_tr, u_rot=u_rot, outputs=outputs, heads=heads,
                              vr0=float(vote_range[0]), vr1=float(vote_range[1]))
            rc = call("cppf_pair_mlp_bf16_decode_batch", pc.device, 1, C.byref(item), feat.shape[1], dims, len(self.ppffcs) - 1,
                      self.out_dim, tr_num_bins, rot_num_bins, ok=(_lib.EUNSUPPORTED,))
        else:
            rc = call("cppf_pair_mlp_decode", pc.device, pc, pc_normal, feat, idxs, idxs.dtype == torch.int64, self._packed_weights(pc.device),
                      pc.shape[0], feat.shape[1], dims, len(self.ppffcs) - 1, P, self.out_dim, tr_num_bins, rot_num_bins,
                      float(vote_range[0]), float(vote_range[1]), u_tr, u_rot, outputs, heads, scratch(ws), ok=(_lib.EUNSUPPORTED,))
        if rc == _lib.EUNSUPPORTED:  # architecture / bin counts outside the fused kernel: logits (of the same precision) + decode kernels
            with torch.no_grad():
                logits = self._forward_device(pc, pc_normal, feat, idxs) if self.precision == "bf16" else \
                    self.forward_with_idx(pc, pc_normal, feat, idxs)
            call("cppf_decode_center", pc.device, logits, P, self.out_dim, tr_num_bins, float(vote_range[0]), float(vote_range[1]), u_tr,
                 outputs)
            if heads is not None:
                call("cppf_decode_rot", pc.device, logits, P, self.out_dim, self.out_dim, tr_num_bins, rot_num_bins, u_rot, heads)
        return outputs, heads

    def fused_decode_supported(self, tr_num_bins=32, rot_num_bins=36):
        """True when cppf_pair_mlp_decode / cppf_pair_mlp_decode_sel serve this encoder and these bin counts in one fused
        launch (train.py:35's architecture with config/config.yaml's 32 / 36 bins); other configurations go through the logits
        and the stand-alone decode kernels."""
        return (self.ppffcs == [84, 32, 32, 16] and self.out_dim == 141 and int(tr_num_bins) == 32
                and int(rot_num_bins) == 36)

    def forward_decode_sel(self, pc, pc_normal, feat, idxs, u_rot, sel, n_sel, heads, max_sel=None, tr_num_bins=32,
                           rot_num_bins=36):
        """The second MLP pass of nocs/inference.py:236-256 on the pairs that survived the back-vote: for i < min(n_sel[0],
        max_sel) the pair sel[i] gets its heads row {theta_up, theta_right, aux_up, aux_right, sx, sy, sz, 0} written into
        `heads` f32[P,8] (other rows untouched); u_rot f32[P,2] is indexed by original pair.  Must follow a forward_decode /
        forward_with_idx call on the same (feat, parameters) in the same scratch scope: the per-point table it left is reused.
        sel i32[>=max_sel] and n_sel i32[1] are device tensors (cppf_compact_mask's outputs), so no host sync."""
        idxs = self._as_index_tensor(idxs, self._device_of(pc))
        pc, pc_normal, feat = self._check_inputs(pc, pc_normal, feat)
        P = idxs.shape[0]
        u_rot = canon(u_rot, torch.float32, pc.device, "u_rot", (P, 2))
        # (sel / n_sel are another kernel's outputs and heads is written in place: checked, never converted)
        dev_tensor(sel, torch.int32, "sel", None, pc.device)
        dev_tensor(n_sel, torch.int32, "n_sel", None, pc.device)
        dev_tensor(heads, torch.float32, "heads", (P, 8), pc.device)
        max_sel = P if max_sel is None else min(int(max_sel), P)
        dims = (C.c_int * len(self.ppffcs))(*self.ppffcs)
        ws = self._scratch(pc, feat, dims)
        if self.precision == "bf16":
            item = self._item(_lib.PairMlpItem(), pc, pc_normal, feat, idxs, ws, u_rot=u_rot, heads=heads, sel=sel, n_sel_dev=n_sel,
                              max_sel=max_sel)
            rc = call("cppf_pair_mlp_bf16_decode_sel_batch", pc.device, 1, C.byref(item), feat.shape[1], dims, len(self.ppffcs) - 1,
                      self.out_dim, tr_num_bins, rot_num_bins, ok=(_lib.EUNSUPPORTED,))
        else:
            rc = call("cppf_pair_mlp_decode_sel", pc.device, pc, pc_normal, feat, idxs, idxs.dtype == torch.int64,
                      self._packed_weights(pc.device), pc.shape[0], feat.shape[1], dims, len(self.ppffcs) - 1, P, self.out_dim, tr_num_bins,
                      rot_num_bins, u_rot, sel, n_sel, max_sel, heads, scratch(ws), ok=(_lib.EUNSUPPORTED,))
        if rc == _lib.EUNSUPPORTED:
            # architecture / bin counts outside the fused kernel: the logits of the selected pairs + cppf_decode_rot, rows
            # scattered back.  The count is read on the host (one sync; not capturable -- the pose pipelines run such
            # configurations in their full-first form instead, see inference.PosePipeline).
            n = min(int(n_sel.item()), max_sel)
            if n > 0:
                rows = sel[:n].long()
                logits = self._forward_device(pc, pc_normal, feat, idxs[rows].contiguous())
                sub = torch.empty((n, 8), dtype=torch.float32, device=pc.device)
                call("cppf_decode_rot", pc.device, logits, n, self.out_dim, self.out_dim, tr_num_bins, rot_num_bins,
                     u_rot[rows].contiguous(), sub)
                heads[rows] = sub
        return heads

    # ------------------------------------------------------------------ internals
    def _item(self, item, pc, pc_normal, feat, idxs, ws, **more):
        """one pair list of cppf_pair_mlp*_decode_batch / _decode_sel_batch: what every pass reads, then the pass's own fields"""
        return fill(item, pc.device, pc=pc, nrm=pc_normal, feat=feat, idxs=idxs, packed=self._packed_weights(pc.device),
                    workspace=scratch(ws), n_points=pc.shape[0], n_pairs=idxs.shape[0], idx_is_i64=idxs.dtype == torch.int64, **more)

    def _scratch(self, pc, feat, dims):
        need = _lib.lib().cppf_pair_mlp_workspace_bytes(pc.shape[0], feat.shape[1], dims, len(self.ppffcs) - 1,
                                                        self.out_dim)
        return workspace(max(int(need), 256), pc.device, "pair_mlp")

    def _needs_graph(self, feat):
        if not torch.is_grad_enabled():
            return False
        return feat.requires_grad or any(p.requires_grad for p in _params_of(self))

    def _has_device_backward(self, pc, feat):
        """csrc/pair_mlp_bwd.hip covers ppffcs = [84,32,32,16] (train.py:35) on a HIP device."""
        return (pc.is_cuda and self.ppffcs == [84, 32, 32, 16] and feat.dim() == 2 and feat.shape[1] == 40
                and self.out_dim <= 144)

    def _param_presence(self):
        pres = []
        for layer in self.res_layers:
            pres += [True, True, True, True, layer.fc0 is not None, layer.fc0 is not None]
        return pres + [True, True]

    def _ordered_params(self):
        """parameters in `flatten_state_dict` order: per layer fc1.w, fc1.b, fc2.w, fc2.b, [fc0.w, fc0.b]; final
        (cached like `_params_of`)"""
        cached = self.__dict__.get("_cppf_ordered")
        if cached is not None:
            return cached
        ps = []
        for layer in self.res_layers:
            ps += [layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias]
            if layer.fc0 is not None:
                ps += [layer.fc0.weight, layer.fc0.bias]
        ps += [self.final.weight, self.final.bias]
        self.__dict__["_cppf_ordered"] = ps
        return ps

    def _composite(self, pc, pc_normal, feat, idxs):
        """models/model.py:118-137 as torch ops (autograd path for shapes without a device backward)."""
        a, b = idxs[:, 0].long(), idxs[:, 1].long()
        xy = pc[a] - pc[b]
        d = torch.norm(xy, dim=-1)
        u = xy / (d[..., None] + 1e-7)
        na, nb = pc_normal[a], pc_normal[b]
        ppf = torch.stack([(na * u).sum(-1), (nb * u).sum(-1), (na * nb).sum(-1), d], -1)
        x = torch.cat([feat[a], feat[b], ppf], -1)
        for layer in self.res_layers:
            x = layer(x)
        return self.final(x)

    @staticmethod
    def _as_index_tensor(idxs, device):
        if isinstance(idxs, np.ndarray):                       # nocs/inference.py:177,182
            if idxs.dtype not in (np.int64, np.int32):
                idxs = idxs.astype(np.int64)
            idxs = torch.from_numpy(np.ascontiguousarray(idxs)).to(device, non_blocking=True)
        if not isinstance(idxs, torch.Tensor):
            raise TypeError(f"idxs: expected numpy array or torch tensor, got {type(idxs).__name__}")
        if idxs.dtype not in (torch.int64, torch.int32):
            raise TypeError(f"idxs: expected int64/int32, got {idxs.dtype}")
        if idxs.dim() != 2 or idxs.shape[1] != 2:
            raise ValueError(f"idxs: expected shape [P,2], got {tuple(idxs.shape)}")
        if idxs.device != torch.device(device):
            raise ValueError(f"idxs: tensor on {idxs.device}, expected {device} (a numpy pair list is uploaded, a tensor is not)")
        return idxs.contiguous()

    @staticmethod
    def _device_of(pc):
        """the device every other argument must share: pc's -- looked at first, so that a cloud left on the host is what the error
        names (not the pair list that disagrees with it)"""
        if not isinstance(pc, torch.Tensor) or not pc.is_cuda:
            raise _lib.CppfError(f"pc: PPFEncoder inference runs on a HIP device only (no CPU fallback), got pc on "
                                 f"{getattr(pc, 'device', type(pc).__name__)}; move the module and its inputs to cuda")
        return pc.device

    def _check_inputs(self, pc, pc_normal, feat):
        require_cuda()
        self._device_of(pc)
        if pc.dim() != 2 or pc.shape[1] != 3 or pc_normal.shape != pc.shape:
            raise ValueError("pc / pc_normal must be [N,3]")
        if feat.dim() != 2 or feat.shape[0] != pc.shape[0] or 2 * feat.shape[1] + 4 != self.ppffcs[0]:
            raise ValueError(f"feat must be [N,F] with 2F+4 == ppffcs[0] == {self.ppffcs[0]}")
        # (a pc_normal / feat left on the host or on another GPU is refused here: its address means nothing to the launch)
        return (canon(pc, torch.float32, pc.device, "pc"), canon(pc_normal, torch.float32, pc.device, "pc_normal"),
                canon(feat, torch.float32, pc.device, "feat"))

    def _flat_params(self, device):
        """(flat device f32 copy of the parameters in `flatten_state_dict` order, host i64 offset table), rebuilt when a
        parameter changes (one torch.cat on the device, no host round trip)."""
        key = self._param_key(device)
        if self._flat is None or self._flat_key != key:
            ps = self._ordered_params()
            dev = torch.device(device)
            parts = [p.detach().reshape(-1).float() for p in ps]
            old = self._flat[0] if self._flat is not None else None
            if old is not None and old.device == dev and parts[0].device == dev and old.numel() == sum(t.numel() for t in parts):
                flat = torch.cat(parts, out=old)             # same buffer: see _DeviceWeights
            else:
                flat = torch.cat(parts).to(device).contiguous()
            offs, pos = [], 0
            it = iter(ps)
            for present in self._param_presence():
                if present:
                    offs.append(pos)
                    pos += next(it).numel()
                else:
                    offs.append(-1)
            self._flat = (flat, (C.c_int64 * len(offs))(*offs))
            self._flat_key = key
        return self._flat

    def _shape_args(self):
        return ((self.ppffcs[0] - 4) // 2, (C.c_int * len(self.ppffcs))(*self.ppffcs), len(self.ppffcs) - 1, self.out_dim)

    def _image_words(self, precision):
        L = _lib.lib()
        if precision == "bf16":
            return int(L.cppf_pair_mlp_bf16_packed_bytes(*self._shape_args())) // 4
        return int(L.cppf_pair_mlp_packed_floats(*self._shape_args()))

    def _no_kernel(self, precision):
        if precision == "bf16":
            return (f"no bf16 kernel for ppffcs={self.ppffcs}, out_dim={self.out_dim}: csrc/pair_mlp_bf16.hip covers "
                    "ppffcs=[84,32,32,16], out_dim<=144 (train.py:35); there is no fall-back to fp32")
        return f"no device kernel for ppffcs={self.ppffcs}, out_dim={self.out_dim} (layers wider than 128 units are unsupported)"

    def _pack_image(self, dev, buf):
        """-> the lane-ordered image.  The standard architecture packs on the device (a training loop changes the weights every
        step and never leaves the stream); other stacks (fp32 only) and the host device pack on the host."""
        pack = self._entry("pack")
        if dev.type == "cuda" and self.ppffcs == [84, 32, 32, 16] and self.out_dim <= 144:
            call(pack + "_device", dev, *self._flat_params(dev), *self._shape_args(), buf)
        else:
            sd = {k: v.detach().float().cpu().numpy() for k, v in self.state_dict().items()}
            image = torch.zeros(buf.numel(), dtype=buf.dtype)
            call(pack, None, *flatten_state_dict(sd, self.ppffcs), *self._shape_args(), image)
            buf.copy_(image)
        return buf


def flatten_state_dict(sd, ppffcs):
    """state_dict (numpy values, reference key names) -> (flat f32 params, i64 offset table) in the
    layout cppf_pair_mlp_pack() documents: 6 offsets per res layer, then final.weight/bias."""
    chunks, offs, pos = [], [], 0
    names = []
    for i in range(len(ppffcs) - 1):
        names += [f"res_layers.{i}.{k}" for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc0.weight",
                                                   "fc0.bias")]
    names += ["final.weight", "final.bias"]
    for nme in names:
        if nme not in sd:
            offs.append(-1)
            continue
        a = np.ascontiguousarray(sd[nme], dtype=np.float32).reshape(-1)
        chunks.append(a)
        offs.append(pos)
        pos += a.size
    return np.concatenate(chunks).astype(np.float32), np.asarray(offs, dtype=np.int64)


def batch_plan(n_pairs):
    """geometry of forward_decode_batch for lists of these lengths (cppf_pair_mlp_batch_plan): dict(per_xcd, grid, wg_begin) --
    per_xcd > 0: the XCD-pinned mapping (1, 2, 4 or 8 lists of nearly equal length), 0: contiguous workgroup ranges"""
    n = len(n_pairs)
    arr = (C.c_int64 * n)(*[int(v) for v in n_pairs])
    per_xcd, grid, wb = C.c_int(0), C.c_int(0), (C.c_int * (n + 1))()
    call("cppf_pair_mlp_batch_plan", None, n, arr, C.byref(per_xcd), C.byref(grid), wb)
    return dict(per_xcd=per_xcd.value, grid=grid.value, wg_begin=list(wb))


def forward_decode_batch(items, tr_num_bins=32, rot_num_bins=36, tables_out=None):
    """PPFEncoder.forward_decode for up to 8 pair lists in ONE launch (cppf_pair_mlp_decode_batch): the instances of a frame, each
    with its own cloud, pair list and encoder (the reference keeps one network per category, nocs/inference.py:79-90).  `items`:
    dicts {encoder, pc, pc_normal, feat, idxs, u_tr, vote_range[, u_rot]}; all with u_rot or none.  Returns [(outputs, heads)] in
    order -- the same bits as one forward_decode call per item; what the batch saves is the ~9 us a launch spends before its
    first MFMA (weights -> LDS, the first cold index -> gather chain), paid once instead of once per list."""
    if not 1 <= len(items) <= 8:
        raise ValueError("1 to 8 pair lists per launch")
    enc0 = items[0]["encoder"]
    dev = enc0._device_of(items[0]["pc"])
    dims = (C.c_int * len(enc0.ppffcs))(*enc0.ppffcs)
    arr = (_lib.PairMlpItem * len(items))()
    keep, outs = [], []
    for i, it in enumerate(items):
        enc = it["encoder"]
        if enc.ppffcs != enc0.ppffcs or enc.out_dim != enc0.out_dim:
            raise ValueError("the encoders of one launch must share an architecture")
        if enc.precision != enc0.precision:
            raise _lib.CppfError(f"the encoders of one launch must share a precision: item 0 is {enc0.precision!r}, item {i} is "
                                 f"{enc.precision!r} (PPFEncoder.set_precision)")
        idxs = enc._as_index_tensor(it["idxs"], dev)
        pc, nrm, feat = enc._check_inputs(it["pc"], it["pc_normal"], it["feat"])
        if pc.device != dev:
            raise ValueError(f"item {i}: pc on {pc.device}, the launch is on {dev}")
        P = idxs.shape[0]
        # (converted like forward_decode's: a captured pipeline's own buffers are canonical and pass as they are)
        u_tr, u_rot = canon(it["u_tr"], torch.float32, dev, "u_tr", (P, 2)), it.get("u_rot")
        u_rot = None if u_rot is None else canon(u_rot, torch.float32, dev, "u_rot", (P, 2))
        outputs = torch.empty((P, 2), dtype=torch.float32, device=dev)
        heads = torch.empty((P, 8), dtype=torch.float32, device=dev) if u_rot is not None else None
        need = _lib.lib().cppf_pair_mlp_workspace_bytes(pc.shape[0], feat.shape[1], dims, len(enc.ppffcs) - 1, enc.out_dim)
        ws = workspace(max(int(need), 256), dev, f"pair_mlp_batch{i}")       # (each list its own per-point table)
        enc._item(arr[i], pc, nrm, feat, idxs, ws, u_tr=u_tr, u_rot=u_rot, outputs=outputs, heads=heads,
                  vr0=float(it["vote_range"][0]), vr1=float(it["vote_range"][1]))
        keep.append((idxs, pc, nrm, feat, ws, u_tr, u_rot))
        outs.append((outputs, heads))
    call(enc0._entry("decode_batch"), dev, len(items), arr, items[0]["feat"].shape[1], dims, len(enc0.ppffcs) - 1, enc0.out_dim, tr_num_bins,
         rot_num_bins)
    if tables_out is not None:      # the per-point tables this pass left (a batched second pass reuses them: cppf_pose_tail_batch)
        tables_out[:] = [k[4] for k in keep]
    return outs

