"""CPU statement of the bf16 point encoder's numerics (csrc/sprin_bf16.hip).  numpy and torch.bfloat16 only -- no
project code.

    forward(sd, pc, nrm, nbrs, order, bf16=True, num_layers=1) -> (out f32[N, 40], changed)

sd: the PointEncoder's state_dict as numpy arrays (spconvs.l.kernel.{0,3,6,9,12}, .{1,4,7,10} = the LayerNorms, spconvs.l.outnet,
spconvs.l.layer_norm, aggrs.l.linear).  bf() = round to nearest even to bf16.  Per layer and neighbour:
    x6 = rifeat (fp32)                                  y1 = W1 x6 + b1             fp32, ascending inputs
    a1 = bf(relu(LN1(y1)))                              y2 = bf(W2) a1 + b2         bf16 x bf16 products, fp32 sums on the bias seed
    a2 = bf(relu(LN2(y2))) ... layers 3, 4 alike        kern = bf(W5) a4 + b5       fp32, not rounded
then the rank contraction, the outnet, its LayerNorm and GlobalInfoProp in fp32 on kern.
`order` ("asc" / "desc") is the order in which layers 2..5 add their products: the matrix instruction's own order is not
specified, so a test compares the device against "asc" with a tolerance taken from the spread between the two.  Everything else
runs in the kernel's one order: bias-seeded fma chains over ascending inputs, sums over ascending neighbours, the LayerNorm's
partial sums grouped as sp_ln_relu4 groups them (channel 16 ob + 4 g + r: per g sequentially over (ob, r), then (p0 + p1) + (p2 + p3)).
bf16=False is the same code with bf() as the identity: the fp32 kernel's arithmetic (F in the tests).
`changed`: whether any bf() changed a value (weights or activations)."""
import numpy as np
import torch

F32 = np.float32


class _Bf:
    def __init__(self, on):
        self.on, self.changed = on, False

    def __call__(self, x):
        x = np.ascontiguousarray(x, F32)
        if not self.on:
            return x
        y = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
        self.changed = self.changed or not np.array_equal(x, y)
        return y


def _fma(w, x, acc):
    return (w.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(F32)


def _lin(W, X, b, order="asc"):
    """[M, O]: bias-seeded fma chain over the inputs of X [M, K] in `order`"""
    acc = np.broadcast_to(b[None].astype(F32), (X.shape[0], W.shape[0])).copy()
    ks = range(W.shape[1]) if order == "asc" else range(W.shape[1] - 1, -1, -1)
    for k in ks:
        acc = _fma(W[None, :, k], X[:, k, None], acc)
    return acc


def _lane_sum(v):
    """v [M, nob, 4 g, 4 r] -> [M, 1]: sp_ln_relu4's grouping"""
    p = np.zeros((v.shape[0], 4), F32)
    for ob in range(v.shape[1]):
        for r in range(4):
            p = p + v[:, ob, :, r]
    return ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3]))[:, None]


def _ln_relu(y, gamma, beta):
    M, H = y.shape
    Hf = F32(H)
    mean = _lane_sum(y.reshape(M, H // 16, 4, 4)) / Hf
    d = y - mean
    q = _lane_sum((d * d).reshape(M, H // 16, 4, 4))
    inv = F32(1) / np.sqrt(q / Hf + F32(1e-5))
    z = (d * inv) * gamma[None].astype(F32) + beta[None].astype(F32)
    return np.maximum(z, F32(0))


def _norm3(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _layer(sd, l, pc, nrm, nbrs, feat_in, order, bf):
    g = lambda s: np.ascontiguousarray(sd[f"spconvs.{l}.{s}"], F32)
    N, k = nbrs.shape
    r, s = pc[nbrs], pc[:, None, :]                       # [N, k, 3], [N, 1, 3]
    m = np.zeros((N, 3), F32)
    for j in range(k):
        m = m + r[:, j]
    m = (m / F32(k))[:, None, :]
    l1, l2, l3 = m - r, r - s, np.broadcast_to(s - m, r.shape)
    n1, n2, n3 = _norm3(l1), _norm3(l2), _norm3(l3)
    eps = F32(1e-7)
    x6 = np.stack([n1, n2, n3, _dot3(l1, l2) / (n1 * n2 + eps), _dot3(l2, l3) / (n2 * n3 + eps), _dot3(l3, l1) / (n3 * n1 + eps)],
                  -1).astype(F32).reshape(N * k, 6)
    h = _ln_relu(_lin(g("kernel.0.weight"), x6, g("kernel.0.bias")), g("kernel.1.weight"), g("kernel.1.bias"))
    for L in (3, 6, 9):
        y = _lin(bf(g(f"kernel.{L}.weight")), bf(h), g(f"kernel.{L}.bias"), order)
        h = _ln_relu(y, g(f"kernel.{L + 1}.weight"), g(f"kernel.{L + 1}.bias"))
    kern = _lin(bf(g("kernel.12.weight")), bf(h), g("kernel.12.bias"), order).reshape(N, k, 32)
    if feat_in is None:
        nf = np.stack([n2, _dot3(nrm[nbrs], nrm[:, None, :])], -1).astype(F32)      # |p_j - p_i|, n_j . n_i
    else:
        nf = feat_in[nbrs]
    n_in = nf.shape[-1]
    con = np.zeros((N, 32, n_in), F32)                    # einsum("bnkr,bnki->bnri"), sequentially over the neighbours
    for j in range(k):
        con = _fma(kern[:, j, :, None], nf[:, j, None, :], con)
    y = _lin(g("outnet.weight"), con.reshape(N, 32 * n_in), g("outnet.bias"))
    s_ = np.zeros(N, F32)
    for q in range(32):
        s_ = s_ + y[:, q]
    mean = (s_ / F32(32))[:, None]
    v = np.zeros(N, F32)
    for q in range(32):
        dd = y[:, q] - mean[:, 0]
        v = v + dd * dd
    inv = (F32(1) / np.sqrt(v / F32(32) + F32(1e-5)))[:, None]
    z = ((y - mean) * inv) * g("layer_norm.weight")[None] + g("layer_norm.bias")[None]
    glob = global_columns(sd, l, z)
    return np.concatenate([z, np.broadcast_to(glob[None], (N, glob.size))], 1).astype(F32)


def global_columns(sd, l, local):
    """GlobalInfoProp of layer l on the local columns [N, 32]: the linear (bias-seeded fma chain, ascending) and the maximum"""
    Wa, ba = np.ascontiguousarray(sd[f"aggrs.{l}.linear.weight"], F32), np.ascontiguousarray(sd[f"aggrs.{l}.linear.bias"], F32)
    return _lin(Wa, np.ascontiguousarray(local, F32), ba).max(0)


def forward(sd, pc, nrm, nbrs, order, bf16=True, num_layers=1):
    assert order in ("asc", "desc")
    bf = _Bf(bf16)
    pc, nrm, nbrs = np.ascontiguousarray(pc, F32), np.ascontiguousarray(nrm, F32), np.asarray(nbrs).astype(np.int64)
    feat = None
    for l in range(num_layers):
        feat = _layer(sd, l, pc, nrm, nbrs, feat, order, bf)
    return feat, bf.changed
