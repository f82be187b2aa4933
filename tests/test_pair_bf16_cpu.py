"""bf16 pair encoder, the part that needs no device: the additive C ABI (exports, image size, the pack contracts), the host packer's
layout against its written definition, and the CPU emulation (tests/pair_bf16_ref.py) against itself -- bit-equal to its fp32
restatement on the rounding-free case, and its two accumulation orders within the cap on the inputs tests/test_gpu_pair_bf16.py uses."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_cache_protocol
import pair_bf16_cases as cases
import pair_bf16_ref as R
from cppf_amd import _lib
from cppf_amd.models.model import PPFEncoder, flatten_state_dict

STD = [84, 32, 32, 16]
NEW = ["cppf_pair_mlp_bf16_packed_bytes", "cppf_pair_mlp_bf16_pack", "cppf_pair_mlp_bf16_pack_device", "cppf_pair_mlp_bf16_forward",
       "cppf_pair_mlp_bf16_decode_batch", "cppf_pair_mlp_bf16_decode_sel_batch"]
EINVAL, EUNSUPPORTED = -1, -3              # include/cppf.h: CPPF_EINVAL, CPPF_EUNSUPPORTED
OFF_WPT, IMAGE_WORDS = 7968, 13152          # csrc/pair_layout.h: OFF_WPT; csrc/pair_layout_bf16.h: BF16_PACKED


def _dims(d=STD):
    return (C.c_int * len(d))(*d)


def _bf_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)


def test_exports_and_sizes():
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.cppf_abi_version() == 4                                   # additive: the version stays
    for od in (1, 9, 141, 144):
        assert L.cppf_pair_mlp_bf16_packed_bytes(40, _dims(), 3, od) == 4 * IMAGE_WORDS
    assert L.cppf_pair_mlp_bf16_packed_bytes(40, _dims(), 3, 145) == 0
    assert L.cppf_pair_mlp_bf16_packed_bytes(40, _dims(), 3, 0) == 0
    assert L.cppf_pair_mlp_bf16_packed_bytes(32, _dims([68, 32, 32, 16]), 3, 141) == 0
    assert L.cppf_pair_mlp_bf16_packed_bytes(40, _dims([84, 64, 32, 16]), 3, 141) == 0
    assert L.cppf_pair_mlp_bf16_packed_bytes(40, _dims([84, 32, 32]), 2, 141) == 0
    assert L.cppf_pair_mlp_bf16_packed_bytes(40, None, 3, 141) == 0


def test_pack_contracts():
    L = _lib.lib()
    sd = cases.case("random")["sd"]
    params, offs = flatten_state_dict(sd, STD)
    out = np.zeros(IMAGE_WORDS, np.uint32)
    pp, op, outp = params.ctypes.data, offs.ctypes.data, out.ctypes.data
    assert L.cppf_pair_mlp_bf16_pack(pp, op, 40, _dims(), 3, 141, outp) == 0
    assert L.cppf_pair_mlp_bf16_pack(None, op, 40, _dims(), 3, 141, outp) == EINVAL
    assert L.cppf_pair_mlp_bf16_pack(pp, None, 40, _dims(), 3, 141, outp) == EINVAL
    assert L.cppf_pair_mlp_bf16_pack(pp, op, 40, _dims(), 3, 141, None) == EINVAL
    assert L.cppf_pair_mlp_bf16_pack(pp, op, 40, _dims(), 3, 145, outp) == EUNSUPPORTED
    assert L.cppf_pair_mlp_bf16_pack(pp, op, 40, _dims([84, 64, 64, 16]), 3, 141, outp) == EUNSUPPORTED   # no generic bf16 kernel
    bad = offs.copy()
    bad[4] = -1                                                        # layer 0 without fc0: not the standard network
    assert L.cppf_pair_mlp_bf16_pack(pp, bad.ctypes.data, 40, _dims(), 3, 141, outp) == EINVAL
    # the device pack refuses the same things before it touches a device
    assert L.cppf_pair_mlp_bf16_pack_device(pp, offs.ctypes.data_as(C.POINTER(C.c_int64)), 40, _dims(), 3, 145, outp, None) == EUNSUPPORTED
    assert L.cppf_pair_mlp_bf16_pack_device(None, offs.ctypes.data_as(C.POINTER(C.c_int64)), 40, _dims(), 3, 141, outp, None) == EINVAL


@pytest.mark.parametrize("out_dim", [141, 9])
def test_host_image_layout(out_dim):
    """the image against its definition: layer 0 and the biases are the fp32 image's words, a hidden layer's A operand holds
    bf(W[16 ob + j][16 (jj >> 2) + 4 g + (jj & 3)]) in k-slot jj of lane (j, g), the K = 16 layers natural k = 4 g + i"""
    L = _lib.lib()
    sd = cases.case("trained_bottle", out_dim)["sd"]
    params, offs = flatten_state_dict(sd, STD)
    img = np.zeros(IMAGE_WORDS, np.uint32)
    assert L.cppf_pair_mlp_bf16_pack(params.ctypes.data, offs.ctypes.data, 40, _dims(), 3, out_dim, img.ctypes.data) == 0
    n32 = L.cppf_pair_mlp_packed_floats(40, _dims(), 3, out_dim)
    img32 = np.zeros(n32, np.float32)
    assert L.cppf_pair_mlp_pack(params.ctypes.data, offs.ctypes.data, 40, _dims(), 3, out_dim, img32.ctypes.data) == 0
    w32 = img32.view(np.uint32)
    assert np.array_equal(img[:256], w32[:256])                                    # PPF k-step of layer 0
    assert np.array_equal(img[OFF_WPT:], w32[OFF_WPT:OFF_WPT + 40 * 128 + 64])     # per-point projection weights + fc1 | fc0 bias
    half = img.view(np.uint16)
    lane = np.arange(64)
    j, g = lane & 15, lane >> 4
    jj = np.arange(8)
    k32 = 16 * (jj[None, :] >> 2) + 4 * g[:, None] + (jj[None, :] & 3)             # [lane][slot]
    blocks = [("res_layers.0.fc2.weight", 256), ("res_layers.1.fc1.weight", 768), ("res_layers.1.fc2.weight", 1280)]
    for name, off in blocks:
        W = sd[name]
        for ob in range(2):
            want = _bf_bits(W[(16 * ob + j)[:, None], k32])
            got = half[2 * (off + ob * 256): 2 * (off + ob * 256 + 256)].reshape(64, 8)
            assert np.array_equal(got, want), (name, ob)
    for ob, name in enumerate(("res_layers.2.fc1.weight", "res_layers.2.fc0.weight")):
        got = half[2 * (1792 + ob * 256): 2 * (1792 + ob * 256 + 256)].reshape(64, 8)
        assert np.array_equal(got, _bf_bits(sd[name][j[:, None], k32])), name
    k16 = 4 * g[:, None] + np.arange(4)[None, :]
    assert np.array_equal(half[2 * 2304: 2 * 2432].reshape(64, 4), _bf_bits(sd["res_layers.2.fc2.weight"][j[:, None], k16]))
    Wf = np.zeros((144, 16), np.float32)
    Wf[:out_dim] = sd["final.weight"]
    for ob in range(9):
        got = half[2 * (2432 + ob * 128): 2 * (2432 + ob * 128 + 128)].reshape(64, 4)
        assert np.array_equal(got, _bf_bits(Wf[(16 * ob + j)[:, None], k16])), ob
    bias = np.zeros(144, np.float32)
    bias[:out_dim] = sd["final.bias"]
    assert np.array_equal(img[3728:3872].view(np.float32), bias)
    assert np.array_equal(img[3584:3616].view(np.float32), sd["res_layers.0.fc2.bias"])


def test_set_precision_on_the_host():
    enc = PPFEncoder(STD, 141)
    assert enc.precision == "fp32"
    assert enc.set_precision("bf16") is enc and enc.precision == "bf16"
    assert enc.set_precision("fp32").precision == "fp32"
    with pytest.raises(ValueError):
        enc.set_precision("fp16")
    with pytest.raises(_lib.CppfError, match="bf16"):
        PPFEncoder([84, 64, 64, 16], 141).set_precision("bf16")        # no silent fp32 fall-back for other architectures
    with pytest.raises(_lib.CppfError, match="bf16"):
        PPFEncoder(STD, 200).set_precision("bf16")


def test_image_cache_protocol_on_the_host():
    """one image per precision, rebuilt in place and only when asked for (host pack: no device needed)"""
    torch.manual_seed(3)
    enc = PPFEncoder(STD, 141).eval()
    image_cache_protocol.check(enc, enc.res_layers[1].fc1.weight)


def test_emulation_equals_its_fp32_restatement_when_nothing_rounds():
    d = cases.dyadic_case()
    args = (d["sd"], d["pc"], d["nrm"], d["feat"], d["idxs"])
    E_asc, changed = R.forward(*args, "asc", True)
    assert not changed                                                 # no bf() changed a weight or an activation
    E_desc, changed = R.forward(*args, "desc", True)
    assert not changed
    F_asc, _ = R.forward(*args, "asc", False)
    F_desc, _ = R.forward(*args, "desc", False)
    assert np.array_equal(E_asc, F_asc) and np.array_equal(E_desc, F_desc) and np.array_equal(E_asc, E_desc)
    # and the case is not a trivial one: every output column moves, the logits take hundreds of values
    assert (np.abs(E_asc).max(0) > 0).sum() >= 140 and len(np.unique(E_asc)) > 200


def test_emulation_rounds_on_real_weights():
    c = cases.case("trained_bottle")
    _, changed = R.forward(c["sd"], c["pc"], c["nrm"], c["feat"], c["idxs"][:64], "asc", True)
    assert changed


@pytest.mark.parametrize("weights,out_dim", [("trained_bottle", 141), ("random", 141), ("random", 9)])
def test_emulation_orders_agree_within_the_cap_on_the_gpu_inputs(weights, out_dim):
    """the GPU test allows 2 % of a case's pairs to miss E by more than tol (a hidden activation on a bf16 rounding boundary, tipped by
    the accumulation order); the emulation's own two orders must stay below 1 % on those very inputs, or other seeds are due"""
    b = cases.bounds(weights, out_dim)
    print(weights, out_dim, "tol %.3g cap %.3g |logit| <= %.3g emulation-vs-emulation share %.4f" % (b["tol"], b["cap"], b["logit_max"], b["emu_share"]))
    assert b["tol"] > 0 and b["cap"] > b["tol"]
    assert b["emu_share"] <= 0.01
