"""The inputs tests/test_pair_bf16_cpu.py and tests/test_gpu_pair_bf16.py share: a synthetic object, its per-point features from the
SPRIN encoder (the oracle's CPU statement of it, bit-equal to the device kernels: __graft_entry__.smoke), pair lists, and two
pair-encoder weight sets -- the committed trained bottle network and a seeded random one."""
import functools
import os

import numpy as np
import torch

import cppf_amd.synthetic as syn
from conftest import GOLDEN

N_POINTS = 192
P_CASES = (1, 15, 16, 17, 1000, 4099)
P_MAX = max(P_CASES)
WEIGHTS = ("trained_bottle", "random")


@functools.lru_cache(maxsize=None)
def case(weights, out_dim=141):
    """dict(pc, nrm, feat, idxs i64[P_MAX,2], sd: the pair encoder's state dict as numpy arrays)"""
    from oracle import oracle as O
    from cppf_amd.models.model import PPFEncoder, PointEncoder
    cfg = syn.CATEGORIES["bottle"]
    ob = syn.make_object("bottle", N_POINTS, 7)
    if weights == "trained_bottle":
        z = np.load(os.path.join(GOLDEN, "trained_bottle.npz"))
        psd = {k[5:]: z[k] for k in z.files if k.startswith("penc.")}
        sd = {k[4:]: z[k].astype(np.float32) for k in z.files if k.startswith("enc.")}
    else:
        torch.manual_seed(1234)
        penc = PointEncoder(k=cfg.knn, spfcs=[32, 64, 32, 32], num_layers=1, out_dim=32)
        psd = {k: v.detach().numpy().copy() for k, v in penc.state_dict().items()}
        sd = {k: v.detach().numpy().copy() for k, v in PPFEncoder(cfg.ppffcs, 141).state_dict().items()}
    if out_dim != 141:          # the notebook's 9-column head (nocs/zero_shot.ipynb): the first rows of the same final layer
        sd = dict(sd)
        sd["final.weight"], sd["final.bias"] = sd["final.weight"][:out_dim].copy(), sd["final.bias"][:out_dim].copy()
    packed, desc = O.pack_point_encoder(psd, 1)
    k = min(cfg.knn, N_POINTS)
    feat = O.point_encoder(ob["pc"], ob["normals"], O.knn(ob["pc"], k), packed, desc, order=1)
    idxs = np.random.default_rng(99).integers(0, N_POINTS, (P_MAX, 2)).astype(np.int64)
    return dict(pc=ob["pc"].astype(np.float32), nrm=ob["normals"].astype(np.float32), feat=feat.astype(np.float32), idxs=idxs, sd=sd,
                cfg=cfg)


@functools.lru_cache(maxsize=None)
def bounds(weights, out_dim=141):
    """pair_bf16_ref.order_spread_and_cap on the case's whole pair list, computed once"""
    import pair_bf16_ref as R
    c = case(weights, out_dim)
    return R.order_spread_and_cap(c["sd"], c["pc"], c["nrm"], c["feat"], c["idxs"])


@functools.lru_cache(maxsize=None)
def dyadic_case(out_dim=141):
    """the rounding-free case: dyadic weights, {0, 1} features, PPF columns of layer 0 zeroed (pair_bf16_ref.dyadic_state_dict)"""
    import pair_bf16_ref as R
    c = case("random")
    rng = np.random.default_rng(5)
    feat = (rng.random((N_POINTS, 40)) < 0.3).astype(np.float32)
    return dict(pc=c["pc"], nrm=c["nrm"], feat=feat, idxs=c["idxs"], sd=R.dyadic_state_dict(out_dim, 11))
