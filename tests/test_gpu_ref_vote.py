"""The reference's OWN vote-kernel text, executed on the device, against the product kernels.

oracle/ref_build.py compiles the text of the reference's models/voting.py (extracted at build time, never stored here) for
gfx950 twice -- hipcc defaults (what a straight HIP port of the reference would run: contraction on, ocml trigonometry) and
-ffp-contract=off -- and oracle/_ref/ref_vote_runner launches one kernel of a code object per process, with the reference's
launch convention.  Every runner call is a fresh child process under a time limit; after a call that does not exit 0 no
further call is started in this session (the remaining tests fail at once and say so).

The product side is the models.voting drop-ins (ppf_kernel, backvote_kernel = cppf_backvote, rot_voting_kernel) and
voting.vote_argmax (cppf_vote_argmax), on the cases of tests/ref_vote_cases.py.

The executed reference is one more member of the arithmetic family tests/test_oracle_variants.py brackets, and gets that
test's bands, no new ones:
  trip counts   no flip at all, as in that test.  With probs = 1 every in-grid sample deposits a total weight of 1, so
                sum(grid) counts the in-grid samples, and a pair whose trip count (voting.py:31) flips gains or loses a whole
                sample.  The reference's sum must lie within a quarter of one sample, plus what accumulation can move it
                (2^-24 * sum(n * g) for the fp32 atomics), of the exact sum of the oracle's variant 0.  Where that term is not
                small against one sample (a peaked grid: it grows with the square of the density) the pair list is voted in
                slices, each with a term below MASS_ACC, and every slice is held to the band.  The product's sum gets the same
                band with half a quantum per deposit added for its fixed point.  (An in-grid flip also moves the sum by one:
                the check demands that there is neither; samples that merely move show in the next checks.)
  vote grid     same arg-max cell; `ka` inputs: max |grid_ref - grid_product| < 0.5 * the top-1 / top-2 margin; cells non-zero
                on one side only <= 8 * (1e-4 * in_grid + 2) (a floor-cell flip moves eight deposits)
  back-vote     mask flips <= max(4, 4e-3 * n_surv0); rows surviving on both sides within 2 * envelope
  rot_voting    within 2 * envelope
envelope = the largest |variant - variant 0| over O.VARIANTS on the same inputs, computed here by the oracle (for rot_voting
without the rows whose rot is exactly 0, where the ULP variants flip the sign branch of voting.py:142 and the envelope would be
2; those rows are held to the same band as the others); the factor two because ocml's trigonometry is documented "within a
few ulp" and the ULP variants stop at u = 2.  The two `-tol-` cases are the first case with another tol: only their back-vote
differs, and only it is run.  The measured figures are printed (pytest -s) and recorded in DESIGN.md "Oracle"."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_vote_cases as RC
from cppf_amd.models import voting

pytestmark = pytest.mark.gpu
RUNNER = os.path.join(RC.REF_DIR, "ref_vote_runner")
CODE_OBJECTS = {"default": "ref_vote_gfx950.hsaco", "nofma": "ref_vote_gfx950_nofma.hsaco"}
GPU_CASES = [s[0] for s in RC.SPECS] + [RC.SPECS[0][0] + t for t in ("-shell", "-tol-below", "-tol-above")]
MASS_ACC = 0.05        # largest fp32 accumulation term (in samples) a grid may carry into the trip-count check
_stopped = []          # the first runner call that did not exit 0: nothing more is started on the device after it


@pytest.fixture(scope="module")
def cases(oracle):
    return {c["name"]: c for c in RC.all_cases(oracle)}


@pytest.fixture(scope="module")
def artefacts():
    paths = [RUNNER] + [os.path.join(RC.REF_DIR, v) for v in CODE_OBJECTS.values()]
    if not all(os.path.isfile(p) for p in paths):
        pytest.fail("oracle/_ref/ is not built: build() makes it where the reference is present, and it travels with the tree")


def run_ref(c, kernel, obj, tmp_path):
    """one kernel of one code object on case c, in a fresh process -> its output array"""
    if _stopped:
        pytest.fail(f"not started: an earlier runner call failed ({_stopped[0]})")
    job, out = str(tmp_path / "job.bin"), str(tmp_path / f"{kernel}.{obj}.bin")
    RC.write_job(c, job)
    cmd = ["timeout", "-k", "10", "60", RUNNER, os.path.join(RC.REF_DIR, CODE_OBJECTS[obj]), kernel, job, out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        _stopped.append(f"{c['name']} {kernel} {obj}: exit {p.returncode}: {p.stderr.strip()[-300:]}")
        pytest.fail(_stopped[0])
    return np.fromfile(out, np.float32).reshape(RC.out_shape(c, kernel))


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def product(c, dev, backvote_only=False):
    """the three drop-ins and vote_argmax on case c"""
    P = c["idx"].shape[0]
    gx, gy, gz = (int(d) for d in c["dims"])
    pts, out, probs, idx, corner = (t(c[k], dev) for k in ("points", "outputs", "probs", "idx", "corner"))
    res = np.float32(c["res"])
    offs = torch.zeros((P, 3), dtype=torch.float32, device=dev)
    voting.backvote_kernel((1, 1, 1), (32, 1, 1), (pts, out, offs, idx, corner, res, P, c["n_rots"], gx, gy, gz, t(c["gt"], dev),
                                                   np.float32(c["tol"])))
    if backvote_only:
        torch.cuda.synchronize()
        return dict(offsets=offs.cpu().numpy())
    grid = torch.zeros((gx, gy, gz), dtype=torch.float32, device=dev)
    voting.ppf_kernel((1, 1, 1), (32, 1, 1), (pts, out, probs, idx, grid, corner, res, P, c["n_rots"], gx, gy, gz, c["adaptive"]))
    grid2 = torch.zeros_like(grid)
    oi, _ = voting.vote_argmax(pts, out, probs, idx, grid2, corner, float(res), c["n_rots"], c["adaptive"], accumulate=False)
    up = torch.zeros((P, c["n_rots"], 3), dtype=torch.float32, device=dev)
    voting.rot_voting_kernel((1, 1, 1), (32, 1, 1), (pts, out, t(c["rot"], dev), up, idx, corner, res, P, c["n_rots"], gx, gy, gz))
    torch.cuda.synchronize()
    return dict(grid=grid.cpu().numpy(), grid_argmax=grid2.cpu().numpy(), argmax=int(oi.item()), offsets=offs.cpu().numpy(),
                up=up.cpu().numpy())


def check_centre_vote(O, c, prod, g, name, obj, shell, run):
    """g: the reference's ppf_voting grid from the device (as fp64), against the product's two grids and the oracle's exact one;
    run(sub-case) -> the reference's grid for a slice of the pair list"""
    def exact(cc):
        v, n = O.ppf_voting_variant(cc["points"], cc["outputs"], cc["probs"], cc["idx"], cc["dims"], cc["corner"], cc["res"],
                                    cc["n_rots"], cc["adaptive"], 0, return_counts=True)
        return v, n, 2.0 ** -24 * float((n * v).sum())
    v0, n, acc32 = exact(c)
    top2 = np.partition(v0.reshape(-1), -2)[-2:]
    margin = float(top2[1] - top2[0])
    in_grid = O.vote_flips(c["points"], c["outputs"], c["idx"], c["dims"], c["corner"], c["res"], c["n_rots"], c["adaptive"],
                           0)["in_grid"]
    bits = voting.vote_fixed_point_bits(c["idx"].shape[0], c["n_rots"], c["dims"])
    acc_fixed = 0.5 * 2.0 ** -bits * float(n.sum())
    dm0 = abs(g.sum() - v0.sum())
    print(f"[{name} {obj}] ppf_voting: in-grid samples {in_grid}, |d mass| against the exact grid {dm0:.4f} (fp32 accumulation "
          f"term {acc32:.4f}; fixed-point term {acc_fixed:.4f} at {bits} bits)")
    if shell:
        assert in_grid == 0 and not g.any() and not prod["grid"].any() and not prod["grid_argmax"].any()
        return
    assert dm0 <= 0.25 + acc32, (dm0, acc32)
    if acc32 > MASS_ACC:                     # the term grows with the square of the pairs voted together
        k = int(np.ceil(np.sqrt(acc32 / MASS_ACC))) + 1
        P = c["idx"].shape[0]
        worst = 0.0
        for j in range(k):
            cc = dict(c)
            for f in ("idx", "outputs", "rot"):
                cc[f] = c[f][P * j // k:P * (j + 1) // k]
            vj, _, accj = exact(cc)
            dmj = abs(run(cc).astype(np.float64).sum() - vj.sum())
            worst = max(worst, dmj)
            assert accj <= MASS_ACC and dmj <= 0.25 + accj, (j, k, dmj, accj)
        print(f"[{name} {obj}] ppf_voting in {k} slices: largest |d mass| of a slice {worst:.4f}")
    for key in ("grid", "grid_argmax"):
        gp = prod[key].astype(np.float64)
        one_sided = int(((g != 0) != (gp != 0)).sum())
        dmass = abs(g.sum() - gp.sum())
        dmax = float(np.abs(g - gp).max())
        print(f"[{name} {obj}] ppf_voting vs {key}: |d mass| {dmass:.4f}, max |d cell| {dmax:.3e}, margin {margin:.4f}, "
              f"one-sided cells {one_sided}")
        assert dmass <= 0.25 + acc32 + acc_fixed, (key, dmass, acc32, acc_fixed)
        assert int(np.argmax(g)) == int(np.argmax(gp)) == prod["argmax"], key
        if c["mode"] == "ka":
            assert dmax < 0.5 * margin, (key, dmax, margin)
        assert one_sided <= 8 * (1e-4 * in_grid + 2), (key, one_sided)


@pytest.mark.parametrize("obj", list(CODE_OBJECTS))
@pytest.mark.parametrize("name", GPU_CASES)
def test_reference_text_on_the_device_against_the_product(oracle, dev, artefacts, cases, tmp_path, name, obj):
    O, c = oracle, cases[name]
    shell = name.endswith("-shell")
    if _stopped:
        pytest.fail(f"not started: an earlier runner call failed ({_stopped[0]})")
    tol_case = "-tol-" in name
    prod = product(c, dev, backvote_only=tol_case)
    a = (c["points"], c["outputs"], c["idx"])
    if not tol_case:
        check_centre_vote(O, c, prod, run_ref(c, "ppf_voting", obj, tmp_path).astype(np.float64), name, obj, shell,
                          lambda cc: run_ref(cc, "ppf_voting", obj, tmp_path))

    # ---- back-vote
    bo = run_ref(c, "backvote", obj, tmp_path)
    oo0, m0 = O.backvote_variant(*a, c["corner"], c["res"], c["n_rots"], c["dims"], c["gt"], np.float32(c["tol"]), 0)
    np.testing.assert_array_equal(prod["offsets"], oo0)                        # (the product IS variant 0)
    env_b = 0.0
    for v in O.VARIANTS.values():
        oov, mv = O.backvote_variant(*a, c["corner"], c["res"], c["n_rots"], c["dims"], c["gt"], np.float32(c["tol"]), v)
        both = mv & m0
        env_b = max(env_b, float(np.abs(oov[both] - oo0[both]).max()) if both.any() else 0.0)
    mr, mp = np.any(bo != 0, -1), np.any(prod["offsets"] != 0, -1)
    n0, flips, both = int(mp.sum()), int((mr != mp).sum()), mr & mp
    d_b = float(np.abs(bo[both] - prod["offsets"][both]).max()) if both.any() else 0.0
    print(f"[{name} {obj}] backvote: survivors {n0}, mask flips {flips}, max |d offset| {d_b:.3e}, family envelope {env_b:.3e}")
    if shell:
        assert mr.all() and mp.all()
    assert flips <= max(4, 4e-3 * n0)
    assert d_b <= 2 * env_b, (d_b, env_b)
    if tol_case:                             # the probed survivor: its accepted sample is rejected below, accepted above
        k = c["probe"]
        tol0 = np.float32(cases[RC.SPECS[0][0]]["tol"])
        full, _ = O.backvote_variant(*a, c["corner"], c["res"], c["n_rots"], c["dims"], c["gt"], tol0, 0)
        assert full[k].any() and (np.abs(bo[k] - full[k]).max() <= 2 * env_b) == name.endswith("above")
        return

    # ---- orientation candidates
    ru = run_ref(c, "rot_voting", obj, tmp_path)
    u0 = O.rot_voting_variant(c["points"], c["rot"], c["idx"], c["n_rots"], 0)
    np.testing.assert_array_equal(prod["up"], u0)
    # (a row with rot == 0 is left out of the envelope: tan is exactly 0 there and the ULP variants push it across the sign
    # test of voting.py:142, which turns the row round -- an envelope of 2 would bound nothing.  The row itself is compared.)
    live = c["rot"] != 0
    env_r = max(float(np.abs(O.rot_voting_variant(c["points"], c["rot"], c["idx"], c["n_rots"], v) - u0)[live].max())
                for v in O.VARIANTS.values())
    d_r = float(np.abs(ru - prod["up"]).max())
    print(f"[{name} {obj}] rot_voting: max |d candidate| {d_r:.3e}, family envelope {env_r:.3e}, "
          f"elements that differ {int((ru != prod['up']).sum())} of {ru.size}")
    assert np.array_equal(np.any(ru != 0, (1, 2)), np.any(prod["up"] != 0, (1, 2)))      # the same early returns
    assert d_r <= 2 * env_r, (d_r, env_r)
