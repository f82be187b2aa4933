"""The device path of cppf_amd.evaluation (csrc/pose_eval.hip; include/cppf.h "Pose evaluation") against its host path, and against
the reference's recorded outputs in tests/golden/eval_map.npz.

Bounds: both sides run the same fp64 algorithm on O(1) quantities, so 1e-9 on IoU and centimetres is far above rounding; near 0
degrees one ulp of the cosine is about 1e-6 degrees, hence 1e-5 there; 1e-6 against the reference's hull-based IoU is the bound
tests/test_evaluation.py uses for the host path.  Match tables must be equal, APs within 1e-12."""
import copy
import pickle

import numpy as np
import pytest

from cppf_amd import evaluation as E

pytestmark = pytest.mark.gpu

NOCS = dict(degree_thresholds=[5, 10, 15], shift_thresholds=[5, 10, 15], iou_3d_thresholds=np.linspace(0, 1, 101), iou_pose_thres=0.1,
            use_matches_for_pose=True)
DETECTION = dict(degree_thresholds=[5, 10], shift_thresholds=[2, 5], iou_3d_thresholds=[0.1, 0.25, 0.5], iou_pose_thres=0.1,
                 use_matches_for_pose=False)
SEED = 0                       # the seeded random set of test 6 (chosen on the CPU: the host's values keep clear of every threshold)


@pytest.fixture(scope="module")
def z(golden):
    return golden("eval_map.npz")


def _results(z):
    return [{k.split("::", 1)[1]: z[k] for k in z.files if k.startswith(f"img{i}::")} for i in range(int(z["n_images"]))]


def _rot(rng, max_deg=None):
    """a random rotation; with max_deg a turn by at most that angle about a random axis"""
    if max_deg is None:
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, zq = q
    else:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        th = np.deg2rad(rng.uniform(0, max_deg))
        w, (x, y, zq) = np.cos(th / 2), np.sin(th / 2) * ax
    return np.array([[1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * w), 2 * (x * zq + y * w)],
                     [2 * (x * y + zq * w), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * w)],
                     [2 * (x * zq - y * w), 2 * (y * zq + x * w), 1 - 2 * (x * x + y * y)]])


def _rt(R, t, s=1.0):
    M = np.eye(4)
    M[:3, :3] = R * s
    M[:3, 3] = t
    return M


def random_results(seed, n_images=40, max_inst=6):
    """seeded NOCS-style result dicts: ground truths of all six classes with a scale inside the RT, predictions that are perturbed
    copies (up to 20 degrees, 8 cm, 15 % in size), some missing, some of another class, some with no ground truth at all; images
    0, 1, 2 have no predictions, no ground truths and neither"""
    rng = np.random.default_rng(seed)
    out = []
    for img in range(n_images):
        n = int(rng.integers(1, max_inst + 1))
        cls = rng.integers(1, 7, n).astype(np.int32)
        if img == 3:
            cls[:] = np.arange(n) % 6 + 1
        gt_RTs = np.stack([_rt(_rot(rng), rng.uniform(-0.5, 0.5, 3) + [0, 0, 1.0], rng.uniform(0.15, 0.5)) for _ in range(n)])
        gt_scales = rng.uniform(0.3, 1.0, (n, 3))
        vis = np.where((cls == 6) & (rng.random(n) < 0.5), 0, 1).astype(np.int32)
        p_cls, p_RTs, p_scales = [], [], []
        for k in range(n):
            if rng.random() < 0.2:
                continue                                                          # a missed instance
            R, s = gt_RTs[k, :3, :3], np.cbrt(np.linalg.det(gt_RTs[k, :3, :3]))
            p_RTs.append(_rt((R / s) @ _rot(rng, 20.0), gt_RTs[k, :3, 3] + rng.normal(0, 0.03, 3), s * rng.uniform(0.9, 1.1)))
            p_scales.append(gt_scales[k] * rng.uniform(0.85, 1.15, 3))
            p_cls.append(cls[k] if rng.random() < 0.9 else rng.integers(1, 7))     # sometimes the wrong class
        if rng.random() < 0.3:                                                    # a detection of nothing
            p_RTs.append(_rt(_rot(rng), rng.uniform(-0.5, 0.5, 3) + [0, 0, 1.0], rng.uniform(0.15, 0.5)))
            p_scales.append(rng.uniform(0.3, 1.0, 3))
            p_cls.append(rng.integers(1, 7))
        res = dict(gt_class_ids=cls, gt_RTs=gt_RTs, gt_scales=gt_scales, gt_handle_visibility=vis,
                   pred_class_ids=np.array(p_cls, np.int32), pred_RTs=np.array(p_RTs, np.float64).reshape(-1, 4, 4).astype(np.float32),
                   pred_scales=np.array(p_scales, np.float64).reshape(-1, 3).astype(np.float32),
                   pred_scores=rng.uniform(0.3, 1.0, len(p_cls)).astype(np.float32))
        if img in (0, 2):
            res.update(pred_class_ids=np.zeros(0, np.int32), pred_RTs=np.zeros((0, 4, 4), np.float32),
                       pred_scales=np.zeros((0, 3), np.float32), pred_scores=np.zeros(0, np.float32))
        if img in (1, 2):
            res.update(gt_class_ids=np.zeros(0, np.int32), gt_RTs=np.zeros((0, 4, 4)), gt_scales=np.zeros((0, 3)),
                       gt_handle_visibility=np.zeros(0, np.int32))
        out.append(E.mark_up_symmetry(res))
    return out


def record_host_values(monkeypatch):
    """the host path's per-pair functions wrapped so that they record every value they return, and return a value they have
    already computed for the same arguments from a table (two calls of the metric then cost one): (ious, errs) dicts"""
    ious, errs = {}, {}
    real_iou, real_err = E.compute_3d_iou, E.compute_RT_degree_cm_symmetry

    def iou(RT_1, RT_2, s1, s2, sym, c1, c2):
        key = (RT_1.tobytes(), RT_2.tobytes(), s1.tobytes(), s2.tobytes(), bool(sym), c1 == c2)
        if key not in ious:
            ious[key] = real_iou(RT_1, RT_2, s1, s2, sym, c1, c2)
        return ious[key]

    def err(RT_1, RT_2, sym):
        key = (RT_1.tobytes(), RT_2.tobytes(), bool(sym))
        if key not in errs:
            errs[key] = real_err(RT_1, RT_2, sym)
        return errs[key]

    monkeypatch.setattr(E, "compute_3d_iou", iou)
    monkeypatch.setattr(E, "compute_RT_degree_cm_symmetry", err)
    return ious, errs


def clearance(values, thresholds):
    """the smallest distance of any value to any threshold"""
    values, thresholds = np.asarray(values, np.float64).reshape(-1, 1), np.asarray(thresholds, np.float64).reshape(1, -1)
    return np.abs(values - thresholds).min() if values.size else np.inf


def assert_same_tables(dev_out, host_out):
    for d, h, name in zip(dev_out, host_out, ("iou_aps", "pose_aps", "pose_pred_matches", "pose_gt_matches")):
        assert d.shape == h.shape and d.dtype == h.dtype, name
    np.testing.assert_allclose(dev_out[0], host_out[0], atol=1e-12, rtol=0)
    np.testing.assert_allclose(dev_out[1], host_out[1], atol=1e-12, rtol=0)
    assert np.array_equal(dev_out[2], host_out[2]) and np.array_equal(dev_out[3], host_out[3])


def both_paths(results, dev, **kw):
    host = E.compute_degree_cm_mAP(copy.deepcopy(results), E.SYNSET_NAMES, None, **kw)
    got = E.compute_degree_cm_mAP(copy.deepcopy(results), E.SYNSET_NAMES, None, device=dev, **kw)
    assert_same_tables(got, host)
    return got


# ------------------------------------------------------------------------------------------------ 1. fixture pairs
def test_fixture_pairs_plain_and_swept(z, dev):
    a, b, s1, s2 = z["pair_a"], z["pair_b"], z["pair_s1"], z["pair_s2"]
    n = len(a)
    assert n == 60
    # ground truths twice: rows n.. carry the up-symmetry flag (the errors follow the flag, the IoU follows `sweep`)
    pairs = np.stack([np.tile(np.arange(n), 2), np.arange(2 * n)], -1)
    sym = np.repeat([0, 1], n)
    iou, deg, cm = E.pose_metrics_device(a, s1, np.concatenate([b, b]), np.concatenate([s2, s2]), sym, pairs, sym, device=dev)
    iou, deg, cm = iou.cpu().numpy(), deg.cpu().numpy(), cm.cpu().numpy()
    assert iou.dtype == np.float64 and iou.shape == (2 * n,)
    ref = np.concatenate([z["iou_plain"], z["iou_sym"]])
    h_iou = np.array([E.compute_3d_iou(a[i % n], b[i % n], s1[i % n], s2[i % n], bool(sym[i]), "can", "can") for i in range(2 * n)])
    h_err = np.array([E.compute_RT_degree_cm_symmetry(a[i % n], b[i % n], bool(sym[i])) for i in range(2 * n)])
    print("max |iou - reference|", np.abs(iou - ref).max(), "max |iou - host|", np.abs(iou - h_iou).max(),
          "max |deg - host|", np.abs(deg - h_err[:, 0]).max(), "max |cm - host|", np.abs(cm - h_err[:, 1]).max())
    np.testing.assert_allclose(iou, ref, atol=1e-6, rtol=0)
    np.testing.assert_allclose(iou, h_iou, atol=1e-9, rtol=0)
    np.testing.assert_allclose(cm, h_err[:, 1], atol=1e-9, rtol=0)
    np.testing.assert_allclose(deg, h_err[:, 0], atol=1e-5, rtol=0)


# ------------------------------------------------------------------------------------------------ 2. closed forms
def test_closed_forms_on_the_device(dev):
    """the cases of tests/test_evaluation.py::test_box_volume_identities, and the degenerate ones"""
    rng = np.random.default_rng(1)
    I = np.eye(4)
    T = np.eye(4); T[0, 3] = 0.5
    c = np.sqrt(0.5)
    Ry = np.array([[c, 0, c, 0], [0, 1, 0, 0], [-c, 0, c, 0], [0, 0, 0, 1]])
    inter = 2 * (np.sqrt(2) - 1)
    a9 = 2 / (1 + np.sin(np.deg2rad(9)) + np.cos(np.deg2rad(9)))
    far = np.eye(4); far[:3, 3] = [5.0, 0.0, 0.0]
    cases = [(I, [1, 1, 1], I, [0.5, 0.5, 0.5], 0, 0.125), (I, [1, 2, 3], T, [1, 2, 3], 0, 1 / 3),
             (I, [1, 1, 1], Ry, [1, 1, 1], 0, inter / (2 - inter)), (I, [1, 1, 1], Ry, [1, 1, 1], 1, a9 / (2 - a9))]
    for _ in range(5):
        M = _rt(_rot(rng), rng.normal(size=3))
        cases.append((M @ I @ np.diag([3.0, 3.0, 3.0, 1.0]), [1, 2, 3], M @ T, [1, 2, 3], 0, 1 / 3))
    n_closed = len(cases)
    M = _rt(_rot(rng), rng.normal(size=3), 0.4)
    cases += [(I, [1, 2, 3], far, [1, 2, 3], 0, 0.0), (I, [1, 2, 3], far, [1, 2, 3], 1, 0.0),          # disjoint
              (M, [0.3, 0.5, 0.7], M, [0.3, 0.5, 0.7], 0, 1.0), (M, [0.3, 0.5, 0.7], M, [0.3, 0.5, 0.7], 1, 1.0),      # identical
              (I, [1, 0, 1], I, [1, 1, 1], 0, 0.0), (I, [1, 1, 1], M, [0, 0.5, 0.7], 1, 0.0)]          # a zero extent
    k = len(cases)
    iou, deg, cm = E.pose_metrics_device(np.array([c_[0] for c_ in cases]), np.array([c_[1] for c_ in cases], np.float64),
                                         np.array([c_[2] for c_ in cases]), np.array([c_[3] for c_ in cases], np.float64),
                                         np.zeros(k, bool), np.stack([np.arange(k), np.arange(k)], -1),
                                         np.array([c_[4] for c_ in cases]), device=dev)
    iou = iou.cpu().numpy()
    want = np.array([c_[5] for c_ in cases])
    print("closed forms: max error", np.abs(iou - want).max())
    assert np.isfinite(iou).all() and np.isfinite(deg.cpu().numpy()).all() and np.isfinite(cm.cpu().numpy()).all()
    np.testing.assert_allclose(iou[:n_closed], want[:n_closed], atol=1e-9, rtol=0)
    assert np.all(iou[n_closed:n_closed + 2] == 0.0)
    np.testing.assert_allclose(iou[n_closed + 2:n_closed + 4], 1.0, atol=1e-9, rtol=0)
    assert np.all(iou[n_closed + 4:] == 0.0)


# ------------------------------------------------------------------------------------------------ 3. tables
def test_map_tables_equal_the_reference_on_the_device(z, dev, tmp_path):
    """both calls of tests/test_evaluation.py::test_map_tables_equal_the_reference, and the pickled round trip"""
    res = _results(z)
    iou_aps, pose_aps, ppm, pgm = E.compute_degree_cm_mAP(copy.deepcopy(res), E.SYNSET_NAMES, str(tmp_path / "log"), device=dev, **NOCS)
    np.testing.assert_allclose(iou_aps, z["iou_aps"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(pose_aps, z["pose_aps"], atol=1e-12, rtol=0)
    assert np.array_equal(ppm, z["pose_pred_matches"]) and np.array_equal(pgm, z["pose_gt_matches"])
    assert iou_aps.shape == (8, 101) and pose_aps.shape == (8, 4, 4) and ppm.shape == (4, 4, len(res), 20) and ppm.dtype == pgm.dtype == int
    with open(tmp_path / "log" / "Pose_Only_AP_5-15degree_5-15cm.pkl", "rb") as f:
        assert np.array_equal(pickle.load(f)["aps"], pose_aps)
    with open(tmp_path / "log" / "IoU_3D_AP_0.0-1.0.pkl", "rb") as f:
        assert np.array_equal(pickle.load(f)["aps"], iou_aps)
    iou2, pose2, _, _ = E.compute_degree_cm_mAP(copy.deepcopy(res), E.SYNSET_NAMES, None, device=dev, **DETECTION)
    np.testing.assert_allclose(iou2, z["iou_aps_detection"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(pose2, z["pose_aps_detection"], atol=1e-12, rtol=0)
    d = tmp_path / "pred"
    d.mkdir()
    for i, r in enumerate(res):
        with open(d / f"results_{i:04d}.pkl", "wb") as f:
            pickle.dump({k: v for k, v in r.items() if k != "gt_up_syms"}, f)
    iou3, pose3, ppm3, _ = E.evaluate_prediction_dir(str(d), stride=1, device=dev)
    np.testing.assert_allclose(iou3, z["iou_aps"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(pose3, z["pose_aps"], atol=1e-12, rtol=0)
    assert np.array_equal(ppm3, z["pose_pred_matches"]) and (tmp_path / "pred_map" / "Pose_Only_AP_5-15degree_5-15cm.pkl").exists()


# ------------------------------------------------------------------------------------------------ 4. launch-shape edges
@pytest.fixture(scope="module")
def edge_pairs():
    """65 work pairs, swept (20 items) and plain (1 item) mixed so that swept pairs straddle the 64-lane workgroups, with the host's
    values (computed once)"""
    rng = np.random.default_rng(7)
    n = 65
    gt = np.stack([_rt(_rot(rng), rng.uniform(-0.2, 0.2, 3), rng.uniform(0.5, 2.0)) for _ in range(n)])
    gt_s = rng.uniform(0.3, 1.0, (n, 3))
    pr = np.stack([_rt((g[:3, :3] / np.cbrt(np.linalg.det(g[:3, :3]))) @ _rot(rng, 40.0), g[:3, 3] + rng.normal(0, 0.1, 3), rng.uniform(0.5, 2.0))
                   for g in gt])
    pr_s = gt_s * rng.uniform(0.8, 1.2, (n, 3))
    sweep = (np.arange(n) % 3 != 1).astype(np.int32)               # items 20, 1, 20, 20, 1, ...: pair 3 covers items 61..80
    sym = (np.arange(n) % 2).astype(np.int32)
    pairs = np.stack([np.arange(n), np.arange(n)[::-1]], -1).astype(np.int32)
    iou = np.array([E.compute_3d_iou(pr[i], gt[j], pr_s[i], gt_s[j], bool(sweep[m]), "a", "a") for m, (i, j) in enumerate(pairs)])
    err = np.array([E.compute_RT_degree_cm_symmetry(pr[i], gt[j], bool(sym[j])) for i, j in pairs])
    return dict(pr=pr, pr_s=pr_s, gt=gt, gt_s=gt_s, sym=sym, pairs=pairs, sweep=sweep, iou=iou, err=err)


@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_work_pair_counts_around_a_workgroup(edge_pairs, dev, M):
    import torch
    e = edge_pairs
    sel = slice(65 - M, 65)                                        # (the tail: M = 1 is a plain pair, M = 63 starts inside a sweep)
    iou, deg, cm = E.pose_metrics_device(e["pr"], e["pr_s"], e["gt"], e["gt_s"], e["sym"], e["pairs"][sel], e["sweep"][sel], device=dev)
    assert iou.is_cuda and iou.shape == (M,) and deg.shape == (M,) and cm.shape == (M,)
    np.testing.assert_allclose(iou.cpu().numpy(), e["iou"][sel], atol=1e-9, rtol=0)
    np.testing.assert_allclose(cm.cpu().numpy(), e["err"][sel, 1], atol=1e-9, rtol=0)
    np.testing.assert_allclose(deg.cpu().numpy(), e["err"][sel, 0], atol=1e-5, rtol=0)
    if M == 65:                                                    # device tensors in, the first M pairs, an empty list
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
        iou2, _, _ = E.pose_metrics_device(t(e["pr"], torch.float64), t(e["pr_s"], torch.float64), t(e["gt"], torch.float64),
                                           t(e["gt_s"], torch.float64), t(e["sym"], torch.int32), t(e["pairs"][:64], torch.int32),
                                           t(e["sweep"][:64], torch.int32))
        np.testing.assert_allclose(iou2.cpu().numpy(), e["iou"][:64], atol=1e-9, rtol=0)
        iou0, deg0, _ = E.pose_metrics_device(e["pr"], e["pr_s"], e["gt"], e["gt_s"], e["sym"], np.zeros((0, 2), np.int32), np.zeros(0, np.int32),
                                              device=dev)
        assert iou0.shape == (0,) and deg0.shape == (0,)
        with pytest.raises(ValueError, match="outside"):
            E.pose_metrics_device(e["pr"], e["pr_s"], e["gt"], e["gt_s"], e["sym"], np.array([[0, 65]]), np.array([0]), device=dev)


def _one_instance_images(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        g = _rt(_rot(rng), rng.uniform(-0.2, 0.2, 3), rng.uniform(0.2, 0.5))
        s = rng.uniform(0.3, 1.0, 3)
        p = _rt((g[:3, :3] / np.cbrt(np.linalg.det(g[:3, :3]))) @ _rot(rng, 25.0), g[:3, 3] + rng.normal(0, 0.04, 3), rng.uniform(0.2, 0.5))
        cls = np.array([k % 6 + 1], np.int32)
        out.append(E.mark_up_symmetry(dict(gt_class_ids=cls, gt_RTs=g[None], gt_scales=s[None], gt_handle_visibility=np.ones(1, np.int32),
                                           pred_class_ids=cls.copy(), pred_RTs=p[None], pred_scales=(s * rng.uniform(0.9, 1.1, 3))[None],
                                           pred_scores=rng.uniform(0.3, 1.0, 1))))
    return out


def test_one_group_one_threshold_and_many_groups(dev):
    imgs = _one_instance_images(65, 11)
    one = dict(degree_thresholds=[], shift_thresholds=[], iou_3d_thresholds=[0.25], iou_pose_thres=0.25, use_matches_for_pose=True)
    both_paths(imgs[:1], dev, **one)                                # one group, one IoU threshold, one (360, 100) pose cell
    three = dict(degree_thresholds=[10], shift_thresholds=[5], iou_3d_thresholds=[0.1, 0.3, 0.6], iou_pose_thres=0.3, use_matches_for_pose=True)
    got = both_paths(imgs, dev, **three)                            # 3 thresholds x 65 groups
    assert got[0].shape == (8, 3) and got[0][1:7].max() > 0


def test_empty_images_and_classes_without_ground_truth(dev):
    res = random_results(3, n_images=6)
    assert len(res[0]["pred_class_ids"]) == 0 and len(res[1]["gt_class_ids"]) == 0 and len(res[2]["gt_class_ids"]) == len(res[2]["pred_class_ids"]) == 0
    lone = copy.deepcopy(res[4])                                    # a prediction whose class has no ground truth in its image
    missing = [c for c in range(1, 7) if c not in lone["gt_class_ids"]]
    lone["pred_class_ids"] = np.concatenate([lone["pred_class_ids"], [missing[0]]]).astype(np.int32)
    lone["pred_RTs"] = np.concatenate([lone["pred_RTs"], np.eye(4, dtype=np.float32)[None]])
    lone["pred_scales"] = np.concatenate([lone["pred_scales"], np.ones((1, 3), np.float32)])
    lone["pred_scores"] = np.concatenate([lone["pred_scores"], np.array([0.99], np.float32)])
    res.append(lone)
    both_paths(res, dev, **NOCS)
    both_paths(res, dev, **DETECTION)
    both_paths(res[:3], dev, **DETECTION)                           # predictions only / ground truths only / nothing
    both_paths(res[2:3], dev, **NOCS)                               # no group at all: no launch, empty tables
    both_paths([], dev, **DETECTION)


def _row_of_boxes(n, seed, cls=5):
    """n well separated ground truths of one (not symmetric) class with a perturbed prediction each"""
    rng = np.random.default_rng(seed)
    gt = np.stack([_rt(_rot(rng), [0.6 * k, 0.0, 1.0], 0.3) for k in range(n)])
    gs = rng.uniform(0.5, 1.0, (n, 3))
    pr = np.stack([_rt((g[:3, :3] / 0.3) @ _rot(rng, 12.0), g[:3, 3] + rng.normal(0, 0.02, 3), 0.3) for g in gt])
    perm = rng.permutation(n)
    res = dict(gt_class_ids=np.full(n, cls, np.int32), gt_RTs=gt, gt_scales=gs, gt_handle_visibility=np.ones(n, np.int32),
               pred_class_ids=np.full(n, cls, np.int32), pred_RTs=pr[perm], pred_scales=(gs * rng.uniform(0.9, 1.1, (n, 3)))[perm],
               pred_scores=rng.uniform(0.3, 1.0, n))
    return E.mark_up_symmetry(res)


def test_group_cap(dev, monkeypatch):
    full = _row_of_boxes(32, 5)
    # the per-image tables of the reference stop at 20 instances: the 32 x 32 group is scored through the flat tables
    flat = E._flatten_results([copy.deepcopy(full)], 7)
    assert len(flat["pairs"]) == 32 * 32
    thr, deg, sh = [0.1, 0.5], [10.0, 360.0], [5.0, 100.0]
    ipm, igm, ppm, pgm = E._match_tables_on_device(flat, thr, deg, sh, 0, dev)
    gt_RTs, gt_scales = E._unit_scale(full["gt_RTs"], full["gt_scales"], 0.0)
    pr_RTs, pr_scales = E._unit_scale(full["pred_RTs"], full["pred_scales"], 1e-9)
    gm, pm, _, order = E.compute_3d_matches(full["gt_class_ids"], gt_RTs, gt_scales, full["gt_up_syms"], E.SYNSET_NAMES, None,
                                            full["pred_class_ids"], full["pred_scores"], pr_RTs, pr_scales, thr)
    assert np.array_equal(ipm, pm) and np.array_equal(igm, gm) and (pm[0] > -1).sum() >= 24
    keep_p, keep_g = pm[0] > -1, gm[0] > -1
    errs = E.compute_RT_overlaps(full["gt_class_ids"][keep_g], gt_RTs[keep_g], full["gt_up_syms"][keep_g], full["pred_class_ids"][keep_p],
                                 pr_RTs[order][keep_p])
    h_gm, h_pm = E.compute_match_from_degree_cm(errs, full["pred_class_ids"][keep_p], full["gt_class_ids"][keep_g], deg, sh)
    # the device's indices are local to the whole group, the host's to the kept instances
    kp, kg = np.where(keep_p)[0], np.where(keep_g)[0]
    assert np.array_equal(ppm[:, :, keep_p], np.where(h_pm >= 0, kg[np.maximum(h_pm.astype(int), 0)], -1))
    assert np.array_equal(pgm[:, :, keep_g], np.where(h_gm >= 0, kp[np.maximum(h_gm.astype(int), 0)], -1))
    assert np.all(ppm[:, :, ~keep_p] == -1) and np.all(pgm[:, :, ~keep_g] == -1)
    # 33 of a class in one image: refused on the host, with the cap in the message, before anything is launched
    monkeypatch.setattr(E, "_match_tables_on_device", lambda *a, **k: pytest.fail("launched"))
    over = _row_of_boxes(33, 6)
    with pytest.raises(ValueError, match="at most 32"):
        E.compute_degree_cm_mAP([over], E.SYNSET_NAMES, None, device=dev, **DETECTION)
    only_gt = copy.deepcopy(over)
    only_gt.update(pred_class_ids=over["pred_class_ids"][:2], pred_RTs=over["pred_RTs"][:2], pred_scales=over["pred_scales"][:2],
                   pred_scores=over["pred_scores"][:2])
    with pytest.raises(ValueError, match="at most 32"):
        E.compute_degree_cm_mAP([only_gt], E.SYNSET_NAMES, None, device=dev, **DETECTION)


def test_bad_input_is_refused_with_image_and_instance(dev, monkeypatch):
    monkeypatch.setattr(E, "_match_tables_on_device", lambda *a, **k: pytest.fail("launched"))
    good = _one_instance_images(3, 2)
    for key, edit, what in (("pred_RTs", lambda m: m.__setitem__((0, 1, 2), np.nan), "non-finite"),
                            ("gt_RTs", lambda m: m.__setitem__((0, 0, 3), np.inf), "non-finite"),
                            ("pred_scales", lambda m: m.__setitem__((0, 1), np.nan), "non-finite"),
                            ("gt_RTs", lambda m: m.__setitem__((0, slice(0, 3), 2), m[0, :3, 1].copy()), "singular"),
                            ("pred_RTs", lambda m: m.__setitem__((0, slice(0, 3), slice(0, 3)), 0.0), "singular"),
                            ("pred_RTs", lambda m: m.__setitem__((0, 3, 0), 1.0), "homogeneous row")):
        bad = copy.deepcopy(good)
        edit(bad[2][key])
        with pytest.raises(ValueError, match=r"image 2, (predicted|ground-truth) instance 0: " + what):
            E.compute_degree_cm_mAP(bad, E.SYNSET_NAMES, None, device=dev, **DETECTION)


# ------------------------------------------------------------------------------------------------ 5. documented tie rules
def _match_raw(dev, iou, err, n_p, n_g, thr, deg, sh):
    """one group of n_p x n_g hand-made values through the two matching kernels: (iou pred_match [T,n_p], pose pred_match [D,S,n_p])"""
    import torch
    from cppf_amd._torch_util import call
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
    iou_d, err_d = t(iou, np.float64), t(err, np.float64)
    po, go, pair_off = t([0, n_p], np.int32), t([0, n_g], np.int32), t([0], np.int64)
    ipm, igm = torch.full((len(thr), n_p), 7, dtype=torch.int32, device=dev), torch.full((len(thr), n_g), 7, dtype=torch.int32, device=dev)
    ppm = torch.full((len(deg), len(sh), n_p), 7, dtype=torch.int32, device=dev)
    pgm = torch.full((len(deg), len(sh), n_g), 7, dtype=torch.int32, device=dev)
    call("cppf_pose_eval_match_iou", dev, iou_d, po, go, pair_off, 1, t(thr, np.float64), len(thr), n_p, n_g, n_p * n_g, ipm, igm)
    call("cppf_pose_eval_match_pose", dev, err_d, po, go, pair_off, 1, t(deg, np.float64), len(deg), t(sh, np.float64), len(sh), None, None,
         n_p, n_g, n_p * n_g, ppm, pgm)
    return ipm.cpu().numpy(), igm.cpu().numpy(), ppm.cpu().numpy(), pgm.cpu().numpy()


def test_tie_rules_are_the_headers(dev):
    """include/cppf.h: equal float32 IoUs -> the HIGHER ground-truth index; equal degree + cm sums -> the LOWER one"""
    import os
    from conftest import ROOT
    hdr = " ".join(open(os.path.join(ROOT, "include", "cppf.h")).read().split())
    assert "EQUAL float32 IoU the one with the HIGHER index is taken" in hdr and "EQUAL sum the one with the LOWER index is taken" in hdr
    # two identical ground-truth boxes, one prediction: through the metric, then the kernels on hand-made values
    one = _one_instance_images(1, 4)[0]
    two = copy.deepcopy(one)
    for k in ("gt_class_ids", "gt_RTs", "gt_scales", "gt_handle_visibility", "gt_up_syms"):
        two[k] = np.concatenate([one[k], one[k]])
    kw = dict(degree_thresholds=[], shift_thresholds=[], iou_3d_thresholds=[0.05], iou_pose_thres=0.05)
    _, _, ppm, pgm = E.compute_degree_cm_mAP([copy.deepcopy(two)], E.SYNSET_NAMES, None, use_matches_for_pose=True, device=dev, **kw)
    assert ppm[0, 0, 0, 0] == 1 and pgm[0, 0, 0, :2].tolist() == [-1, 0]          # the IoU match (and so the pose match) is gt 1
    _, _, ppm, pgm = E.compute_degree_cm_mAP([copy.deepcopy(two)], E.SYNSET_NAMES, None, use_matches_for_pose=False, device=dev, **kw)
    assert ppm[0, 0, 0, 0] == 0 and pgm[0, 0, 0, :2].tolist() == [0, -1]          # every instance scored: equal sums, gt 0
    # float32 equality decides: 0.5 and 0.5 + 1e-9 are one float32 value; two predictions, three ground truths
    iou = [[0.5, 0.5 + 1e-9, 0.2], [0.5, 0.5, 0.5]]
    err = [[[3.0, 2.0], [1.0, 4.0], [2.0, 3.0]], [[4.0, 1.0], [1.0, 4.0], [2.5, 2.5]]]
    ipm, igm, ppm, pgm = _match_raw(dev, iou, err, 2, 3, [0.3, 0.5], [360.0, 2.5], [100.0])
    assert ipm.tolist() == [[1, 2], [-1, -1]] and igm.tolist() == [[-1, 0, 1], [-1, -1, -1]]      # (0.5 is not strictly above 0.5)
    assert ppm[0, 0].tolist() == [0, 1] and pgm[0, 0].tolist() == [0, 1, -1]
    assert ppm[1, 0].tolist() == [1, 2] and pgm[1, 0].tolist() == [-1, 0, 1]       # degrees <= 2.5: gt 0 is out, gt 1 before gt 2


# ------------------------------------------------------------------------------------------------ 6. seeded random sets
def test_seeded_random_sets(dev, monkeypatch):
    """40 images, up to 6 instances each, all six classes, perturbed / missing / misclassified / spurious predictions: the tables of
    both calls are the host's.  First the host's own per-pair values (recorded while it runs) are shown to keep clear of every
    threshold by 1e-6 (chosen by the seed, on the CPU), so a flipped comparison cannot be excused by rounding.  IoUs of exactly 0.0
    (disjoint boxes) are exempt from the distance to the threshold 0.0: both paths produce that zero by the same
    `v <= 1e-9 min(va, vb) -> 0.0` rule, not by rounding, and 0.0 is not strictly above 0.0 on either."""
    res = random_results(SEED)
    assert set(np.concatenate([r["gt_class_ids"] for r in res]).tolist()) == {1, 2, 3, 4, 5, 6}
    assert sum(len(r["pred_class_ids"]) for r in res) > 80
    ious, errs = record_host_values(monkeypatch)
    host_b = E.compute_degree_cm_mAP(copy.deepcopy(res), E.SYNSET_NAMES, None, **DETECTION)      # (scores every same-class pair)
    host_a = E.compute_degree_cm_mAP(copy.deepcopy(res), E.SYNSET_NAMES, None, **NOCS)
    iou, err = np.array(list(ious.values()), np.float64), np.array(list(errs.values())).reshape(-1, 2)
    assert len(iou) > 60 and (iou > 0).sum() > 40 and len(err) == len(iou)
    near = [clearance(iou[iou != 0.0], np.linspace(0, 1, 101)), clearance(iou[iou != 0.0], [0.1, 0.25, 0.5]),
            clearance(err[:, 0], [2, 5, 10, 15, 360]), clearance(err[:, 1], [2, 5, 10, 15, 100])]
    print("host clearances (IoU x 2, degrees, cm):", near)
    assert min(near) > 1e-6
    a = E.compute_degree_cm_mAP(copy.deepcopy(res), E.SYNSET_NAMES, None, device=dev, **NOCS)
    b = E.compute_degree_cm_mAP(copy.deepcopy(res), E.SYNSET_NAMES, None, device=dev, **DETECTION)
    assert_same_tables(a, host_a)
    assert_same_tables(b, host_b)
    assert 0 < a[0][-1].mean() < 1 and 0 < b[1][-1].mean() < 1        # neither trivially empty nor perfect
