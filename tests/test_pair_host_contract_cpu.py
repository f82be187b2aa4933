"""What the pair encoder's entry points answer to a defective call, fp32 and bf16 side by side: one table of calls with exactly one
defect each, run against cppf_pair_mlp_{forward, decode_batch, decode_sel_batch} and their _bf16_ twins.  Every refusal (and every
no-op) returns before the first HIP call, so no device is needed and the dummy addresses are never dereferenced.  The two variants
share their host path (csrc/pair_mlp_common.h: PairVariant): they may differ only where the header says so -- a list without pairs."""
import ctypes as C

import pytest

from cppf_amd import _lib

STD = [84, 32, 32, 16]
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3        # include/cppf.h
ADDR = 0x10000                                              # a non-null host address; nothing reads it
N, P = 64, 53
TABLE_BYTES = N * 128 * 4                                   # cppf_pair_mlp_workspace_bytes(N, ...): N x PROJ_COLS floats
FORWARD, BATCH, SEL = "forward", "decode_batch", "decode_sel_batch"
ENTRY = {(FORWARD, "fp32"): "cppf_pair_mlp_forward", (FORWARD, "bf16"): "cppf_pair_mlp_bf16_forward",
         (BATCH, "fp32"): "cppf_pair_mlp_decode_batch", (BATCH, "bf16"): "cppf_pair_mlp_bf16_decode_batch",
         (SEL, "fp32"): "cppf_pair_mlp_decode_sel_batch", (SEL, "bf16"): "cppf_pair_mlp_bf16_decode_sel_batch"}
POINTERS = ("pc", "nrm", "feat", "idxs", "packed", "u_tr", "u_rot", "outputs", "heads", "workspace", "sel", "n_sel_dev")


def _item(**changes):
    """one sound pair list (with the rotation heads); the forward reads its cloud, list, image, `outputs` (as `out`) and workspace"""
    it = {k: ADDR for k in POINTERS}
    it.update(workspace_bytes=TABLE_BYTES, n_points=N, n_pairs=P, max_sel=P, vr0=0.5, vr1=0.5, idx_is_i64=1)
    it.update(changes)
    return it


def _sound():
    return dict(n_items=1, items=[_item()], items_null=False, dims=list(STD), tr_bins=32, rot_bins=36, out_dim=141)


def _set(**kw):
    return lambda s: s.update(kw)


def _it(**kw):
    return lambda s: s["items"][0].update(kw)


def _run(kind, variant, mutate):
    s = _sound()
    mutate(s)
    fn = getattr(_lib.lib(), ENTRY[kind, variant])
    dims = None if s["dims"] is None else (C.c_int * len(s["dims"]))(*s["dims"])
    if kind == FORWARD:
        it = s["items"][0]
        return fn(it["pc"], it["nrm"], it["feat"], it["idxs"], it["idx_is_i64"], it["packed"], it["n_points"], 40, dims, 3, it["n_pairs"],
                  s["out_dim"], it["outputs"], it["workspace"], it["workspace_bytes"], None)
    arr = (_lib.PairMlpItem * len(s["items"]))()
    for dst, src in zip(arr, s["items"]):
        for k, v in src.items():
            setattr(dst, k, v)
    return fn(s["n_items"], None if s["items_null"] else C.cast(arr, C.c_void_p), 40, dims, 3, s["out_dim"], s["tr_bins"], s["rot_bins"], None)


# (row, what it changes in a sound call, {kind: code}).  A code is what both variants answer; a pair is (fp32, bf16), None in it = the
# row is not run against that variant.  A kind that is missing has no such argument, or the call would be sound and launch.
ROWS = [
    ("n_items 0", _set(n_items=0), {BATCH: EINVAL, SEL: EINVAL}),
    ("n_items 9", _set(n_items=9, items=[_item() for _ in range(9)]), {BATCH: EINVAL, SEL: EINVAL}),
    ("items NULL", _set(items_null=True), {BATCH: EINVAL, SEL: EINVAL}),
    ("dims NULL", _set(dims=None), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("tr_bins 30", _set(tr_bins=30), {BATCH: EUNSUPPORTED, SEL: EUNSUPPORTED}),
    ("out_dim 100", _set(out_dim=100), {BATCH: EUNSUPPORTED, SEL: EUNSUPPORTED}),
    # (the fp32 forward serves other widths and stacks with its generic kernel: for it these two calls are sound)
    ("out_dim 145", _set(out_dim=145), {FORWARD: (None, EUNSUPPORTED)}),
    ("dims 84-64-32-16", _set(dims=[84, 64, 32, 16]), {FORWARD: (None, EUNSUPPORTED), BATCH: EUNSUPPORTED, SEL: EUNSUPPORTED}),
    ("pc NULL", _it(pc=None), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("nrm NULL", _it(nrm=None), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("feat NULL", _it(feat=None), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("idxs NULL", _it(idxs=None), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("packed NULL", _it(packed=None), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("u_tr NULL", _it(u_tr=None), {BATCH: EINVAL}),
    ("outputs NULL", _it(outputs=None), {FORWARD: EINVAL, BATCH: EINVAL}),
    ("u_rot NULL = heads without u_rot", _it(u_rot=None), {BATCH: EINVAL, SEL: EINVAL}),
    ("heads NULL = u_rot without heads", _it(heads=None), {BATCH: EINVAL, SEL: EINVAL}),
    ("sel NULL", _it(sel=None), {SEL: EINVAL}),
    ("n_sel_dev NULL", _it(n_sel_dev=None), {SEL: EINVAL}),
    ("two items disagree about heads", _set(n_items=2, items=[_item(), _item(heads=None, u_rot=None)]), {BATCH: EINVAL}),
    # (the fp32 second-pass batch did not look at n_points before this table was written; the row is run against the bf16 entry)
    ("n_points 0", _it(n_points=0), {FORWARD: EINVAL, BATCH: EINVAL, SEL: (None, EINVAL)}),
    ("n_points 2^23", _it(n_points=1 << 23, workspace_bytes=(1 << 23) * 512), {FORWARD: EUNSUPPORTED, BATCH: EUNSUPPORTED, SEL: EUNSUPPORTED}),
    ("n_pairs 2^27", _it(n_pairs=1 << 27), {FORWARD: EUNSUPPORTED, BATCH: EUNSUPPORTED, SEL: EUNSUPPORTED}),
    ("n_pairs -1", _it(n_pairs=-1), {FORWARD: EINVAL, BATCH: EINVAL, SEL: EINVAL}),
    ("workspace NULL", _it(workspace=None), {FORWARD: EWORKSPACE, BATCH: EWORKSPACE, SEL: EWORKSPACE}),
    ("workspace one byte short", _it(workspace_bytes=TABLE_BYTES - 1), {FORWARD: EWORKSPACE, BATCH: EWORKSPACE, SEL: EWORKSPACE}),
    ("max_sel -1", _it(max_sel=-1), {SEL: EINVAL}),
    ("n_pairs == 0", _it(n_pairs=0), {FORWARD: OK, BATCH: (EINVAL, OK), SEL: OK}),
    ("max_sel == 0", _it(max_sel=0), {SEL: OK}),
]


def _expected(codes, kind, variant):
    want = codes.get(kind)
    return want[("fp32", "bf16").index(variant)] if isinstance(want, tuple) else want


@pytest.mark.parametrize("variant", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", [FORWARD, BATCH, SEL])
def test_defective_calls(kind, variant):
    got, want = {}, {}
    for row, mutate, codes in ROWS:
        w = _expected(codes, kind, variant)
        if w is not None:
            want[row] = w
            got[row] = _run(kind, variant, mutate)
    assert len(want) >= 12
    assert got == want


def test_the_variants_differ_only_on_a_list_without_pairs():
    differing = [(row, kind) for row, _, codes in ROWS for kind, c in codes.items()
                 if isinstance(c, tuple) and None not in c and c[0] != c[1]]
    assert differing == [("n_pairs == 0", BATCH)]
    # and every row names each kind's two variants, or says why one is left out (above)
    assert [row for row, _, codes in ROWS for c in codes.values() if isinstance(c, tuple) and None in c] == \
        ["out_dim 145", "dims 84-64-32-16", "n_points 0"]
