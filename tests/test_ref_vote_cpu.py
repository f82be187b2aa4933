"""The oracle's three vote kernels against the reference's OWN executed text.

oracle/ref_build.py extracts ppf_voting / backvote / rot_voting from the reference's models/voting.py at build time and
compiles them as host C++ (contraction off, glibc trig) into oracle/_ref/libref_vote_host.so; that is the arithmetic of the
oracle's ORV_LIBM member (oracle/voting_variants.c), so

  rot_voting, backvote   bit-equal to O.rot_voting_variant / O.backvote_variant with O.LIBM (offsets and mask)
  ppf_voting             the serial fp32 grid against the exact fp64 grid of O.ppf_voting_variant(..., O.LIBM): the same set of
                         non-zero cells, and per cell |g32 - g64| <= n_deposits(cell) * 2^-24 * g64(cell) -- deposits are
                         non-negative, so each fp32 add errs by at most half an ulp of a running sum that never exceeds the
                         final value; the deposit counts come from the oracle

on the cases of tests/ref_vote_cases.py (edges listed there).  Every test runs twice over: against tests/golden/ref_vote.npz
(what the host build gave on a prefix of each case, tests/golden/make_golden_vote.py) always, and against the host build itself
on the whole case when oracle/_ref/ exists.  tests/test_oracle_variants.py::test_variant_zero_is_the_oracle ties variant 0, and
with it this pin, to cppf_oracle.c.  CPU only."""
import numpy as np
import pytest

import ref_vote_cases as RC

F = np.float32


@pytest.fixture(scope="module")
def cases(oracle):
    return {c["name"]: c for c in RC.all_cases(oracle)}


@pytest.fixture(scope="module")
def fixture_cases(golden):
    g = golden("ref_vote.npz")
    out = {}
    for name in g["names"]:
        k = str(name) + "."
        res, tol, n_rots, adaptive = g[k + "meta"]
        c = dict(name=str(name), res=float(res), tol=float(tol), n_rots=int(n_rots), adaptive=bool(adaptive))
        src = k if k + "points" in g.files else RC.SPECS[0][0] + "."       # (-tol- cases: the first case's inputs)
        for f in ("points", "outputs", "idx", "rot", "corner", "dims", "gt"):
            c[f] = g[src + f]
        c["probs"] = np.ones(c["points"].shape[0], F)
        c["ref"] = dict(backvote=g[k + "offsets"])
        if k + "probe" in g.files:
            c["probe"] = int(g[k + "probe"])
        if src == k:
            grid = np.zeros(int(np.prod(c["dims"])), F)
            grid[g[k + "grid_cells"]] = g[k + "grid_vals"]
            c["ref"].update(ppf_voting=grid.reshape(tuple(int(d) for d in c["dims"])), rot_voting=g[k + "up"])
        out[str(name)] = c
    return out


NAMES = [s[0] for s in RC.SPECS] + [RC.SPECS[0][0] + "-shell"]
NAMES_BACKVOTE = NAMES + [RC.SPECS[0][0] + t for t in ("-tol-below", "-tol-above")]      # same inputs, another tol


def _sides(cases, fixture_cases, name, kernel):
    """(case, what the reference's text gave) from the fixture and, when oracle/_ref/ is built, from the host build"""
    fc = fixture_cases[name]
    ref = fc["ref"][kernel]
    if kernel == "rot_voting":
        fc = RC.prefix(fc, ref.shape[0])
    yield "fixture", fc, ref
    if RC.host_lib() is not None:
        c = cases[name]
        yield "host build", c, RC.host_run(c, kernel)
        # the fixture is what the host build gives on the prefix (and the case builder still makes the fixture's inputs)
        p = RC.prefix(c, fc["idx"].shape[0])
        for f in ("points", "outputs", "idx", "rot", "corner", "dims", "gt"):
            np.testing.assert_array_equal(p[f], fc[f], err_msg=f"{name}.{f}: regenerate tests/golden/ref_vote.npz")
        np.testing.assert_array_equal(RC.host_run(p, kernel), ref, err_msg=f"{name}: fixture is stale")


def test_fixture_holds_every_case_and_stays_small(fixture_cases):
    assert sorted(fixture_cases) == sorted(NAMES_BACKVOTE)
    for name in NAMES:
        c = fixture_cases[name]
        assert c["ref"]["rot_voting"].shape[0] * c["n_rots"] <= 256 * 72
        assert c["idx"].shape[0] % 32 != 0


@pytest.mark.parametrize("name", NAMES)
def test_rot_voting_is_the_reference_text_bit_for_bit(oracle, cases, fixture_cases, name):
    O = oracle
    for side, c, ref in _sides(cases, fixture_cases, name, "rot_voting"):
        got = O.rot_voting_variant(c["points"], c["rot"], c["idx"], c["n_rots"], O.LIBM)
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=f"{name} ({side})")
        assert np.isfinite(ref).all()
        # the edges are exercised: early returns leave zeros, every other row is a unit vector
        a, b = c["points"][c["idx"][:, 0]], c["points"][c["idx"][:, 1]]
        dead = np.linalg.norm(a.astype(np.float64) - b, axis=-1) < 0.9e-7
        if not name.endswith("-shell"):
            assert dead[2] and dead[4:8].all() and not dead[[0, 1, 3]].any()
        assert not ref[dead].any() and np.allclose(np.linalg.norm(ref[~dead].astype(np.float64), axis=-1), 1, atol=1e-5)


@pytest.mark.parametrize("name", NAMES_BACKVOTE)
def test_backvote_is_the_reference_text_bit_for_bit(oracle, cases, fixture_cases, name):
    O = oracle
    for side, c, ref in _sides(cases, fixture_cases, name, "backvote"):
        oo, mask = O.backvote_variant(c["points"], c["outputs"], c["idx"], c["corner"], c["res"], c["n_rots"], c["dims"], c["gt"],
                                      F(c["tol"]), O.LIBM)
        np.testing.assert_array_equal(oo.view(np.uint32), ref.view(np.uint32), err_msg=f"{name} ({side})")
        np.testing.assert_array_equal(mask, np.any(ref != 0, -1), err_msg=f"{name} ({side})")
        if name.endswith("-shell"):          # every centre lies in the shell that backvote accepts
            assert mask.all()
        elif "-tol-" in name:                # the probed survivor's accepted sample is rejected below, accepted above
            k = c["probe"]
            b0 = RC.SPECS[0][0]
            base = fixture_cases[b0]["ref"]["backvote"] if side == "fixture" else RC.host_run(cases[b0], "backvote")
            assert k < ref.shape[0] and base[k].any()
            assert np.array_equal(ref[k], base[k]) == name.endswith("above"), (name, side)
        else:
            assert not mask[2] and not mask[4:8].any() and not mask[8:12].any()    # early return / zero rotations
    if name == RC.SPECS[0][0]:
        assert fixture_cases[name]["ref"]["backvote"].any()


@pytest.mark.parametrize("name", NAMES)
def test_ppf_voting_fp32_grid_is_the_reference_text_within_its_rounding(oracle, cases, fixture_cases, name):
    O = oracle
    for side, c, ref in _sides(cases, fixture_cases, name, "ppf_voting"):
        g64, n = O.ppf_voting_variant(c["points"], c["outputs"], c["probs"], c["idx"], c["dims"], c["corner"], c["res"], c["n_rots"],
                                      c["adaptive"], O.LIBM, return_counts=True)
        np.testing.assert_array_equal(ref != 0, g64 != 0, err_msg=f"{name} ({side}): set of non-zero cells")
        np.testing.assert_array_equal(n != 0, g64 != 0)
        err = np.abs(ref.astype(np.float64) - g64)
        bound = n * 2.0 ** -24 * g64
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{name} ({side}): {int((g64 != 0).sum())} cells, {int(n.sum())} deposits, worst |g32 - g64| / bound = {worst:.3f}")
        assert (err <= bound).all(), (name, side, worst)
        if name.endswith("-shell"):          # ... and ppf_voting rejects all of it
            assert not ref.any()
        else:
            assert ref.any()
