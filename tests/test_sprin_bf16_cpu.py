"""bf16 point encoder, the part that needs no device: the additive C ABI (exports, image size, the pack contracts), the host packer's
layout against its written definition, the CPU emulation (tests/sprin_bf16_ref.py) against the reference's own output, and the
emulation against itself on the cases tests/test_gpu_sprin_bf16.py uses."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_cache_protocol
import sprin_bf16_cases as cases
import sprin_bf16_ref as R
from cppf_amd import _lib
from cppf_amd.models.model import PointEncoder
from cppf_amd.models.sprin import pack_point_encoder

NEW = ["cppf_point_encoder_bf16_packed_bytes", "cppf_point_encoder_bf16_pack", "cppf_point_encoder_bf16_pack_device",
       "cppf_point_encoder_bf16_forward", "cppf_point_encoder_bf16_forward_dyn", "cppf_point_encoder_bf16_forward_batch"]
EINVAL, EUNSUPPORTED = -1, -3              # include/cppf.h: CPPF_EINVAL, CPPF_EUNSUPPORTED
IMAGE_WORDS = 3840                         # csrc/sprin_layout_bf16.h: SPB_WORDS
L1, L2, L3, L4, L5, VEC = 0, 256, 1280, 2304, 2816, 3328   # SPB_L1 .. SPB_VEC, words
STD = [32, 64, 32, 32]


def _hid(h=STD):
    return (C.c_int * len(h))(*h)


def _bf_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)


def _natural_floats(num_layers):
    return int(_lib.lib().cppf_point_encoder_packed_floats(_hid(), 4, 32, 2, 32, 8, num_layers)) - 6912 * num_layers   # SPW_FLOATS


def test_exports_and_sizes():
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.cppf_abi_version() == 4                                   # additive: the version stays
    for layers in (1, 2, 3):
        assert L.cppf_point_encoder_bf16_packed_bytes(_hid(), 4, 32, 2, 32, 8, layers) == 4 * (_natural_floats(layers) + IMAGE_WORDS * layers)
    assert _natural_floats(1) == 9256
    assert L.cppf_point_encoder_bf16_packed_bytes(_hid([32, 64, 64, 32]), 4, 32, 2, 32, 8, 1) == 0
    assert L.cppf_point_encoder_bf16_packed_bytes(_hid(), 4, 16, 2, 32, 8, 1) == 0
    assert L.cppf_point_encoder_bf16_packed_bytes(_hid(), 4, 32, 3, 32, 8, 1) == 0
    assert L.cppf_point_encoder_bf16_packed_bytes(_hid(), 4, 32, 2, 64, 16, 1) == 0
    assert L.cppf_point_encoder_bf16_packed_bytes(_hid(), 3, 32, 2, 32, 8, 1) == 0
    assert L.cppf_point_encoder_bf16_packed_bytes(_hid(), 4, 32, 2, 32, 8, 0) == 0
    assert L.cppf_point_encoder_bf16_packed_bytes(None, 4, 32, 2, 32, 8, 1) == 0


def test_pack_contracts():
    L = _lib.lib()
    natural, desc = pack_point_encoder(cases.weights("random"), 1)
    assert natural.size == _natural_floats(1)
    out = np.zeros(natural.size + IMAGE_WORDS, np.uint32)
    nat, outp = natural.ctypes.data, out.ctypes.data
    assert L.cppf_point_encoder_bf16_pack(nat, _hid(), 4, 32, 2, 32, 8, 1, outp) == 0
    assert L.cppf_point_encoder_bf16_pack(None, _hid(), 4, 32, 2, 32, 8, 1, outp) == EINVAL
    assert L.cppf_point_encoder_bf16_pack(nat, None, 4, 32, 2, 32, 8, 1, outp) == EINVAL
    assert L.cppf_point_encoder_bf16_pack(nat, _hid(), 4, 32, 2, 32, 8, 1, None) == EINVAL
    assert L.cppf_point_encoder_bf16_pack(nat, _hid(), 4, 32, 2, 32, 8, 0, outp) == EINVAL
    assert L.cppf_point_encoder_bf16_pack(nat, _hid([32, 64, 64, 32]), 4, 32, 2, 32, 8, 1, outp) == EUNSUPPORTED   # no generic bf16 kernel
    assert L.cppf_point_encoder_bf16_pack(nat, _hid(), 4, 32, 3, 32, 8, 1, outp) == EUNSUPPORTED
    assert L.cppf_point_encoder_bf16_pack(nat, _hid(), 4, 32, 2, 64, 16, 1, outp) == EUNSUPPORTED
    # the device pack refuses the same things before it touches a device
    assert L.cppf_point_encoder_bf16_pack_device(None, _hid(), 4, 32, 2, 32, 8, 1, outp, None) == EINVAL
    assert L.cppf_point_encoder_bf16_pack_device(nat, _hid(), 4, 32, 2, 32, 8, 1, None, None) == EINVAL
    assert L.cppf_point_encoder_bf16_pack_device(nat, _hid([32, 64, 64, 32]), 4, 32, 2, 32, 8, 1, outp, None) == EUNSUPPORTED
    # the forward entries: arguments checked in the fp32 entries' order, before anything is launched
    args = lambda n, k, packed, h=STD: (nat, nat, nat, n, k, packed, _hid(h), 4, 32, 2, 32, 8, 1, outp, None, 0, None)
    assert L.cppf_point_encoder_bf16_forward(*args(0, 8, nat)) == 0                    # n_points == 0: a no-op
    assert L.cppf_point_encoder_bf16_forward(*args(16, 8, None)) == EINVAL
    assert L.cppf_point_encoder_bf16_forward(*args(16, 8, nat, [32, 64, 64, 32])) == EUNSUPPORTED
    assert L.cppf_point_encoder_bf16_forward(*args(128, 65, nat)) == EUNSUPPORTED
    assert L.cppf_point_encoder_bf16_forward(*args(16, 8, nat)) == -2                  # CPPF_EWORKSPACE
    assert L.cppf_point_encoder_bf16_forward_dyn(nat, nat, nat, 16, None, 8, nat, _hid(), 4, 32, 2, 32, 8, 1, outp, None, 0, None) == EINVAL
    assert L.cppf_point_encoder_bf16_forward_batch(1, None, 8, _hid(), 4, 32, 2, 32, 8, 1, None) == EINVAL
    arr = (_lib.PointEncItem * 1)()
    assert L.cppf_point_encoder_bf16_forward_batch(1, arr, 65, _hid(), 4, 32, 2, 32, 8, 1, None) == EUNSUPPORTED
    assert L.cppf_point_encoder_bf16_forward_batch(1, arr, 8, _hid(), 4, 32, 2, 32, 8, 2, None) == EUNSUPPORTED    # one-layer encoders
    assert L.cppf_point_encoder_bf16_forward_batch(1, arr, 8, _hid([32, 64, 64, 32]), 4, 32, 2, 32, 8, 1, None) == EUNSUPPORTED


@pytest.mark.parametrize("name,num_layers", [("trained_bottle", 1), ("random", 2)])
def test_host_image_layout(name, num_layers):
    """the image against its definition: the natural block verbatim; per layer the fp32 image's layer-1 and vector sections word
    for word, and for layers 2..5 bf(W[16 ob + j][32 h + 16 (e >> 2) + 4 g + (e & 3)]) in k-slot e of lane (j, g) of (ob, h)"""
    L = _lib.lib()
    sd = cases.weights(name, num_layers)
    natural, desc = pack_point_encoder(sd, num_layers)
    nat = natural.size
    img = np.zeros(nat + IMAGE_WORDS * num_layers, np.uint32)
    assert L.cppf_point_encoder_bf16_pack(natural.ctypes.data, _hid(), 4, 32, 2, 32, 8, num_layers, img.ctypes.data) == 0
    img32 = np.zeros(nat + 6912 * num_layers, np.float32)
    assert L.cppf_point_encoder_pack(natural.ctypes.data, _hid(), 4, 32, 2, 32, 8, num_layers, img32.ctypes.data) == 0
    assert np.array_equal(img[:nat], natural.view(np.uint32))
    lane = np.arange(64)
    j, g = lane & 15, lane >> 4
    e = np.arange(8)
    for l in range(num_layers):
        words = img[nat + l * IMAGE_WORDS: nat + (l + 1) * IMAGE_WORDS]
        w32 = img32[nat + l * 6912: nat + (l + 1) * 6912].view(np.uint32)
        assert np.array_equal(words[L1:L2], w32[:256])                         # layer 1, fp32
        assert np.array_equal(words[VEC:], w32[6912 - 512:])                   # bias / gamma / beta vectors, fp32
        half = words.view(np.uint16)
        for key, off, n_ob, n_h in ((3, L2, 4, 1), (6, L3, 2, 2), (9, L4, 2, 1), (12, L5, 2, 1)):
            W = sd[f"spconvs.{l}.kernel.{key}.weight"]
            for ob in range(n_ob):
                for h in range(n_h):
                    k32 = 32 * h + 16 * (e[None, :] >> 2) + 4 * g[:, None] + (e[None, :] & 3)      # [lane][slot]
                    want = _bf_bits(W[(16 * ob + j)[:, None], k32])
                    at = off + (ob * n_h + h) * 256
                    assert np.array_equal(half[2 * at: 2 * (at + 256)].reshape(64, 8), want), (l, key, ob, h)
    assert 2 * (L3 - L2 + L4 - L3 + L5 - L4 + VEC - L5) == 6144                # bf16 values per layer: 12 KB against 24 KB


def test_set_precision_on_the_host():
    enc = PointEncoder(k=60, spfcs=STD, out_dim=32, num_layers=1)
    assert enc.precision == "fp32"
    assert enc.set_precision("bf16") is enc and enc.precision == "bf16"
    assert enc.set_precision("fp32").precision == "fp32"
    with pytest.raises(ValueError):
        enc.set_precision("fp16")
    for bad in (dict(k=60, spfcs=[32, 64, 64, 32], out_dim=32), dict(k=60, spfcs=STD, out_dim=64), dict(k=65, spfcs=STD, out_dim=32),
                dict(k=60, spfcs=STD, out_dim=32, num_nbr_feats=3)):
        with pytest.raises(_lib.CppfError, match="bf16"):
            PointEncoder(num_layers=1, **bad).set_precision("bf16")
    # each precision keeps its own image and its own re-pack bookkeeping (host pack: no device needed)
    enc = PointEncoder(k=60, spfcs=STD, out_dim=32, num_layers=2).eval()
    p32, _ = enc._packed_weights("cpu")
    p16, desc = enc.set_precision("bf16")._packed_weights("cpu")
    assert p16.dtype == torch.int32 and p16.numel() == _natural_floats(2) + 2 * IMAGE_WORDS and desc["num_layers"] == 2
    assert enc._packed_weights("cpu")[0] is p16 and enc._current_image()[0] is p16
    assert enc.set_precision("fp32")._packed_weights("cpu")[0] is p32 and enc._current_image()[0] is p32
    before = p16.clone()
    with torch.no_grad():
        enc.spconvs[0].kernel[3].weight.mul_(2.0)
    p16b = enc.set_precision("bf16")._packed_weights("cpu")[0]
    assert p16b is p16 and not torch.equal(p16b, before)               # re-packed in place, as the fp32 image is
    assert torch.equal(enc.set_precision("fp32")._packed_weights("cpu")[0][:_natural_floats(2)].view(torch.int32), p16b[:_natural_floats(2)])


def test_image_cache_protocol_on_the_host():
    """one image per precision, rebuilt in place and only when asked for (host pack: no device needed)"""
    torch.manual_seed(3)
    enc = PointEncoder(k=60, spfcs=STD, out_dim=32, num_layers=1).eval()
    image_cache_protocol.check(enc, enc.spconvs[0].kernel[3].weight, tensor_of=lambda cached: cached[0])


def test_emulation_without_rounding_is_the_reference(golden):
    """bf16=False: the fp32 kernel's arithmetic, within 2e-5 of the reference's own output"""
    z = golden("sprin_l1.npz")
    sd = {k[4:]: z[k] for k in z.files if k.startswith("sd::")}
    nbrs = z["nbrs_topk"].astype(np.int32)
    for order in ("asc", "desc"):
        F, changed = R.forward(sd, z["pc"], z["nrm"], nbrs, order, bf16=False, num_layers=1)
        assert not changed
        np.testing.assert_allclose(F, z["out"], atol=2e-5, rtol=0)
    E, changed = R.forward(sd, z["pc"][:64], z["nrm"][:64], cases.knn(z["pc"][:64], 16), "asc", bf16=True)
    assert changed and E.shape == (64, 40)


@pytest.mark.parametrize("num_layers", [1, 2])
def test_rounding_free_set_is_rounding_free(num_layers):
    sd = cases.exact_weights(num_layers)
    for n, k in ((40, 17), (70, 64)):
        pc, nrm, nbrs = cases.cloud(n, k)
        E, changed = R.forward(sd, pc, nrm, nbrs, "asc", True, num_layers)
        F, _ = R.forward(sd, pc, nrm, nbrs, "desc", False, num_layers)
        assert not changed                                              # no bf() changed a value
        assert np.array_equal(E, F)                                     # and the order of layers 2..5 does not matter
        assert np.isfinite(E).all() and np.ptp(E[:, :32]) > 0.5


@pytest.mark.parametrize("name,n,k,num_layers", cases.NUMERIC_CASES)
def test_bounds_hold_for_the_emulation_alone(name, n, k, num_layers):
    """what test_gpu_sprin_bf16.py asks of the device, asked of the emulation's other accumulation order: the share of points
    outside tol is at most 4 % (the device may use 10 %), those stay within the cap, and tol sits far below the bf16 effect"""
    b = cases.bounds(name, n, k, num_layers)
    share, worst = cases.emulation_order_share(name, n, k, num_layers)
    print(f"{name} N={n} k={k} layers={num_layers}: tol {b['tol']:.3g}, bf16 effect max|E-F| {b['cap'] / 2:.3g}, "
          f"emulation asc/desc unmatched share {share:.2%}, their max|E_desc-F| {worst:.3g}")
    assert 0 < b["tol"] < 1e-4 and b["cap"] / 2 > 30 * b["tol"]
    assert share <= 0.04
    assert worst <= b["cap"]
    assert np.array_equal(b["E"][:, 32:], np.broadcast_to(b["E"][:1, 32:], (n, 8)))
