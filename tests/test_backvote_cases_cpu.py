"""Conditions on the back-vote boundary family (tests/backvote_cases.py), checked with no GPU, for every configuration that
tests/test_gpu_backvote_edges.py runs: they keep that test from passing trivially.

  * acceptance by the exhaustive loop (oracle.backvote) straddles every fine eps class of the main grid: 10 .. 90 % of the pairs at
    eps = 0, +-1e-7, +-1e-6, +-1e-5; all at -1e-3 and -1e-2; at most 10 % at +1e-3 and +1e-2 (tiny circles, where another sample passes)
  * the inside group holds pairs with several passing rotations, among them n - 1 together with 0 (the wrap), and the near-axis,
    touching and L-switch groups reach the branches they are named after
  * teeth: an fp32 numpy restatement of the stage-1 screen and an fp64 restatement of bv_arc (both in backvote_cases.py) lose no pair
    and no rotation that the loop accepts with the kernel's margins, and at least 50 pairs each with every margin term at zero.
    That proves the inputs reach the region where a tight margin fails; what the device's approximate sqrt / rcp / acos / atan2 take
    out of the margins is the device test's business.
"""
import functools

import numpy as np
import pytest

import backvote_cases as BC

F = np.float32
IDS = [f"gt{BC.CENTRES.index(g)}-res{r:g}-rots{n}" for g, r, n in BC.CONFIGS]


@functools.lru_cache(maxsize=None)
def _family(cfg):
    from oracle import oracle as O
    c = BC.family(*cfg)
    oo, mask = O.backvote(c["points"], c["outputs"], c["idx"], c["corner"], c["res"], c["n_rots"], c["dims"], c["gt"], F(c["tol"]))
    passing, dist, fr = BC.exhaustive(O, c)
    return c, oo, mask, passing, dist, fr


def test_configurations_cover_what_the_device_test_must_run():
    assert {g for g, _, _ in BC.CONFIGS} == set(BC.CENTRES)
    assert {r for _, r, _ in BC.CONFIGS} == set(BC.RESOLUTIONS) == {2e-3, 4e-3, 0.03}
    assert {n for _, _, n in BC.CONFIGS} == set(BC.ROTATIONS) == {7, 72, 120}
    assert ((0.1, -0.05, 0.7), 4e-3, 72) in BC.CONFIGS and len(BC.CONFIGS) == 21


@pytest.mark.parametrize("cfg", BC.CONFIGS, ids=IDS)
def test_family_shape_and_exhaustive_loop_is_the_oracle(oracle, cfg):
    c, oo, mask, passing, dist, fr = _family(cfg)
    P = c["idx"].shape[0]
    assert int((c["group"] == BC.MAIN).sum()) == 840 * len(BC.EPS) and 10_000 < P < 16_000
    assert c["points"].dtype == F and c["points"].shape == (2 * P, 3) and np.array_equal(c["idx"].reshape(-1), np.arange(2 * P))
    assert set(np.unique(c["n"])) >= {1, c["n_rots"]} and c["n"].min() >= 1
    live = fr["nr"] > 0                                              # (far from the origin fp32 merges the closest points: a == b)
    np.testing.assert_array_equal(c["n"][live], fr["nr"][live])
    assert (live | (c["group"] == BC.L_TINY)).all()
    # the loop without its break finds the oracle's winner first
    np.testing.assert_array_equal(passing.any(1), mask)
    first = np.argmax(passing, 1)
    off = np.array([oracle.rot_cs(int(i), int(n)) for i, n in zip(first[mask], fr["nr"][mask])], F)
    want = -((off[:, :1] * fr["x"][mask]).astype(F) + (off[:, 1:] * fr["y"][mask]).astype(F)).astype(F)
    np.testing.assert_array_equal(oo[mask], want)
    # no face is near: every sample within 2 tol of gt is at least 5 cells inside
    lo = (c["gt"] - 2 * c["tol"] - c["corner"]) / c["res"]
    hi = c["dims"] - 1 - (c["gt"] + 2 * c["tol"] - c["corner"]) / c["res"]
    assert lo.min() > 5 and hi.min() > 5


@pytest.mark.parametrize("cfg", BC.CONFIGS, ids=IDS)
def test_acceptance_straddles_the_fine_classes(oracle, cfg):
    c, oo, mask, passing, dist, fr = _family(cfg)
    main = c["group"] == BC.MAIN
    for e in BC.EPS:
        rows = main & (c["eps"] == e)
        frac = mask[rows].mean()
        print(f"eps {e:+.0e}: accepted {int(mask[rows].sum())} of {int(rows.sum())}")
        if abs(e) <= 1e-5:
            assert 0.10 <= frac <= 0.90, (e, frac)
        elif e <= -1e-3:
            assert mask[rows].all(), (e, frac)
        elif e >= 1e-3:
            assert frac <= 0.10, (e, frac)


@pytest.mark.parametrize("cfg", BC.CONFIGS, ids=IDS)
def test_groups_reach_their_branches(oracle, cfg):
    c, oo, mask, passing, dist, fr = _family(cfg)
    n, g = fr["nr"], c["group"]
    rows = np.arange(n.size)
    ins = g == BC.INSIDE
    several = ins & (passing.sum(1) >= 2)
    wrap = several & passing[:, 0] & passing[rows, n - 1] & (n > 1)
    assert several.sum() >= 50 and wrap.sum() >= 50, (several.sum(), wrap.sum())
    assert (np.argmax(passing, 1)[wrap] == 0).all()                  # index order: 0 wins over n - 1
    # the L switches, on both sides, as the kernels compute L2
    p = c["points"]
    dd = p[c["idx"][:, 0]] - p[c["idx"][:, 1]]
    L2 = ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]).astype(F) + dd[:, 2] * dd[:, 2]).astype(F)
    v = L2[g == BC.L_1E3]
    assert (v >= F(1e-6)).sum() >= 20 and (v < F(1e-6)).sum() >= 20 and 0.99e-6 < v.min() and v.max() < 1.01e-6, (v.min(), v.max())
    v = L2[g == BC.L_TINY]
    print(f"L2 of the closest pairs: {int((v == 0).sum())} merged, {int(((v > 0) & (v < F(1e-13))).sum())} below 1e-13, "
          f"{int((v >= F(1e-13)).sum())} at or above")
    if np.abs(p).max() < 2.0:                                        # where fp32 holds 3.2e-7 between two points
        assert ((v > F(1e-14)) & (v < F(1e-13))).sum() >= 20 and (v >= F(1e-13)).sum() >= 20
    # near axis: M = |(w.x, w.y)| from 0 up, c = K / M on both sides of its cuts; touching: c at 1
    w = c["gt"].astype(np.float64) - fr["cc"].astype(np.float64)
    A, B = (w * fr["x"]).sum(-1), (w * fr["y"]).sum(-1)
    M = np.hypot(A, B)
    ax = g == BC.AXIS
    assert (M[ax] < 1e-12).sum() >= 20 and (M[ax] > 1e-9).sum() >= 20
    assert 0.2 < mask[ax].mean() < 0.8
    K = 0.5 * ((w * w).sum(-1) + (fr["x"].astype(np.float64) ** 2).sum(-1) - float(F(c["tol"])) ** 2)
    tc = g == BC.TOUCH
    with np.errstate(divide="ignore", invalid="ignore"):
        cq = K / M
    assert (np.abs(cq[tc & (n > 2)] - 1) < 2e-3).all() and mask[tc].any() and not mask[tc].all()


@pytest.mark.parametrize("cfg", BC.CONFIGS, ids=IDS)
def test_teeth_of_the_two_shortcuts(oracle, cfg):
    c, oo, mask, passing, dist, fr = _family(cfg)
    keep = BC.screen(c, fr)
    assert not (mask & ~keep).any(), np.nonzero(mask & ~keep)[0]
    bare = BC.screen(c, fr, margins=False)
    member, cnt = BC.arc(c, fr)
    assert not (passing & ~member).any(), np.nonzero((passing & ~member).any(1))[0]
    bare_member, _ = BC.arc(c, fr, margins=False)
    lost_s, lost_a = int((mask & ~bare).sum()), int((passing & ~bare_member).any(1).sum())
    first = np.argmax(passing, 1)
    lost_first = int((mask & ~bare_member[np.arange(mask.size), first]).sum())
    print(f"margin-free: screen loses {lost_s} accepted pairs, arc loses a passing rotation of {lost_a} pairs (the winner of {lost_first}); "
          f"largest arc {int(cnt[cnt < fr['nr']].max())} rotations")
    assert lost_s >= 50 and lost_a >= 50 and lost_first >= 50
    many = fr["nr"] > 40
    assert not many.any() or (cnt[many] < fr["nr"][many]).mean() > 0.5       # the arc is a shortcut there, not the whole circle


def test_multi_centres(oracle):
    c = _family(BC.CONFIGS[4])[0]
    cs = BC.centres(c)
    assert cs.shape == (32, 3) and cs.dtype == F and np.array_equal(cs[0], c["gt"]) and np.array_equal(BC.centres(c, 5), cs[:5])
    d = np.linalg.norm(cs[1:17].astype(np.float64) - c["gt"], axis=-1) / c["tol"]
    assert (d < 2e-4).all() and len({tuple(r) for r in cs[:17]}) >= 9     # (displacements below an ulp of gt collapse onto it)
    lo, hi = c["corner"] + 10 * F(c["res"]), c["corner"] + (c["dims"] - 11) * F(c["res"])
    assert (cs >= lo).all() and (cs <= hi).all()
