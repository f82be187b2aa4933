"""CPU statement of the bf16 pair encoder's numerics (DESIGN.md "bf16 pair encoder"), the checker of csrc/pair_mlp_bf16.hip.

Written from the reference's semantics -- ResLayer.forward (models/model.py:27-31: fc2(relu(fc1(x))) + (fc0(x) | x)) and
PPFEncoder.forward_with_idx (:117-137: PPF, cat(feat[a], feat[b], ppf), three ResLayers, final) -- with the roundings the kernel
specifies: layer 0 in fp32 (per-point tables TA / TB as fused multiply-add chains over the 40 feature columns, then the 4 PPF
inputs), every later layer as bf16 x bf16 products (exact in fp32) accumulated in fp32 on a bias seed, fp32 residual adds.

    forward(sd, pc, nrm, feat, idxs, order, bf16=True)  -> (logits f32[P,out_dim], changed)

order: "asc" / "desc", the k order of every accumulation after the per-point tables (the hardware's own order inside a matrix
instruction is a third, unknown one).  bf16=False: the fp32 restatement, the same code with bf() the identity.  changed: whether
any bf() of the run -- of a weight or of an activation -- changed a value (False: the run was rounding-free, and then both
precisions and both orders agree bit for bit).  numpy + torch.bfloat16 only; no device, no project code."""
import numpy as np
import torch

F32 = np.float32


class _Bf:
    """bf(): round to nearest even to bf16 (torch's conversion), remembering whether it ever changed a value"""

    def __init__(self, on):
        self.on, self.changed = on, False

    def __call__(self, x):
        x = np.ascontiguousarray(x, F32)
        if not self.on:
            return x
        y = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
        if not np.array_equal(x, y):
            self.changed = True
        return y


def _fma(w, x, acc):
    """fl32(w * x + acc): the product is exact in float64, the sum there is rounded once more than a fused multiply-add would
    (a double rounding that needs a 29-bit tie: beyond what any bound here looks at)"""
    return (w.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(F32)


def _linear(W, X, seed, order):
    """seed[P,M] + X[P,K] W[M,K]^T, one fused multiply-add per k in `order`"""
    acc = np.ascontiguousarray(np.broadcast_to(seed, (X.shape[0], W.shape[0])), F32).copy()
    ks = range(W.shape[1]) if order == "asc" else range(W.shape[1] - 1, -1, -1)
    for k in ks:
        acc = _fma(W[None, :, k], X[:, k, None], acc)
    return acc


def ppf(pc, nrm, idxs):
    """models/model.py:118-129 in fp32, left to right"""
    a, b = idxs[:, 0].astype(np.int64), idxs[:, 1].astype(np.int64)
    pc, nrm = pc.astype(F32), nrm.astype(F32)
    xy = pc[a] - pc[b]
    d = np.sqrt((xy[:, 0] * xy[:, 0] + xy[:, 1] * xy[:, 1]) + xy[:, 2] * xy[:, 2]).astype(F32)
    u = xy / (d + F32(1e-7))[:, None]
    na, nb = nrm[a], nrm[b]
    dot = lambda p, q: (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
    return np.stack([dot(na, u), dot(nb, u), dot(na, nb), d], -1).astype(F32)


def forward(sd, pc, nrm, feat, idxs, order="asc", bf16=True):
    assert order in ("asc", "desc")
    g = lambda k: np.ascontiguousarray(sd[k], F32)
    bf = _Bf(bf16)
    a, b = idxs[:, 0].astype(np.int64), idxs[:, 1].astype(np.int64)
    feat = np.ascontiguousarray(feat, F32)
    Fd = feat.shape[1]
    # ---- layer 0, fp32 in both precisions.  Tables: chains over the feature columns in ascending k (the kernel's one order);
    #      fc1 and fc0 share the inputs
    W10, W00 = g("res_layers.0.fc1.weight"), g("res_layers.0.fc0.weight")
    Wcat = np.concatenate([W10, W00], 0)                                   # [64, 84]
    bcat = np.concatenate([g("res_layers.0.fc1.bias"), g("res_layers.0.fc0.bias")])
    TA = _linear(Wcat[:, :Fd], feat, bcat[None], "asc")
    TB = _linear(Wcat[:, Fd:2 * Fd], feat, np.zeros((1, 64), F32), "asc")
    pre = _linear(Wcat[:, 2 * Fd:], ppf(pc, nrm, idxs), TA[a] + TB[b], order)   # the 4 PPF inputs on top of (TA[a] + TB[b])
    fc1_0, fc0_0 = pre[:, :32], pre[:, 32:]
    # ---- the bf16 chain
    a0 = bf(np.maximum(fc1_0, 0))
    x1 = _linear(bf(g("res_layers.0.fc2.weight")), a0, g("res_layers.0.fc2.bias")[None], order) + fc0_0
    h = bf(x1)
    a1 = bf(np.maximum(_linear(bf(g("res_layers.1.fc1.weight")), h, g("res_layers.1.fc1.bias")[None], order), 0))
    x2 = _linear(bf(g("res_layers.1.fc2.weight")), a1, g("res_layers.1.fc2.bias")[None], order) + x1    # the unrounded fp32 x1
    h = bf(x2)
    a2 = bf(np.maximum(_linear(bf(g("res_layers.2.fc1.weight")), h, g("res_layers.2.fc1.bias")[None], order), 0))
    s2 = _linear(bf(g("res_layers.2.fc0.weight")), h, g("res_layers.2.fc0.bias")[None], order)
    x3 = _linear(bf(g("res_layers.2.fc2.weight")), a2, g("res_layers.2.fc2.bias")[None], order) + s2
    logits = _linear(bf(g("final.weight")), bf(x3), g("final.bias")[None], order)
    return logits.astype(F32), bf.changed


# ------------------------------------------------------------------------------------------------ the tests' shared inputs
def dyadic_state_dict(out_dim, seed):
    """a rounding-free network: weights and biases in {0, +-1/4, +-1/2, +-1} / fan-in scale, so that with {0, 1} features and the PPF
    columns of layer 0 zeroed every partial sum of every layer is a small multiple of a power of two that bf16 holds exactly"""
    rng = np.random.default_rng(seed)
    sd = {}

    def lin(name, m, k, vals, density):
        w = rng.choice(np.asarray(vals, F32), size=(m, k)) * (rng.random((m, k)) < density)
        sd[name + ".weight"] = w.astype(F32)
        sd[name + ".bias"] = rng.choice(np.asarray([0, 0.5, -0.5, 1], F32), size=m).astype(F32)

    # values are kept to 8 significant bits THROUGH the chain: layer 0 sums a few +-1 (integers < 16), later layers see sparse
    # {+-1/2, +-1} weights on small integers / halves
    lin("res_layers.0.fc1", 32, 84, [1, -1], 0.05)
    lin("res_layers.0.fc0", 32, 84, [1, -1], 0.05)
    for k in ("res_layers.0.fc1.weight", "res_layers.0.fc0.weight"):
        sd[k][:, 80:] = 0                                                   # PPF columns: geometry must not enter
    lin("res_layers.0.fc2", 32, 32, [1, -1], 0.06)
    lin("res_layers.1.fc1", 32, 32, [1, -1], 0.06)
    lin("res_layers.1.fc2", 32, 32, [1, -1], 0.06)
    lin("res_layers.2.fc1", 16, 32, [1, -1], 0.06)
    lin("res_layers.2.fc0", 16, 32, [1, -1], 0.06)
    lin("res_layers.2.fc2", 16, 16, [1, -1], 0.1)
    lin("final", out_dim, 16, [1, -1, 0.5, -0.5], 0.2)
    return sd


def order_spread_and_cap(sd, pc, nrm, feat, idxs):
    """what the GPU test's bounds are made of, for one case: E (k ascending), tol = 4 x the fp32 restatement's own order spread,
    the cap 2 x max|E - F| on |G - F| of unmatched pairs, and the share of pairs on which the two emulation orders disagree by more
    than tol (pairs where a hidden activation sat on a bf16 rounding boundary and the order tipped it)"""
    E_asc, _ = forward(sd, pc, nrm, feat, idxs, "asc", True)
    E_desc, _ = forward(sd, pc, nrm, feat, idxs, "desc", True)
    F_asc, _ = forward(sd, pc, nrm, feat, idxs, "asc", False)
    F_desc, _ = forward(sd, pc, nrm, feat, idxs, "desc", False)
    tol = 4.0 * float(np.max(np.abs(F_asc.astype(np.float64) - F_desc)))
    cap = 2.0 * float(np.max(np.abs(E_asc.astype(np.float64) - F_asc)))
    unmatched = np.max(np.abs(E_asc.astype(np.float64) - E_desc), -1) > tol
    return dict(E=E_asc, F=F_asc, tol=tol, cap=cap, emu_share=float(np.mean(unmatched)), logit_max=float(np.max(np.abs(F_asc))))
