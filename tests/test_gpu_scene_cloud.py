"""scene_stage.scene_cloud, the one builder of a frame's clouds, against the composition of the single public calls written in
tests/scene_cloud_ref.py: every field bit for bit on a small frame whose flat pixel index is not the rank of its valid pixels, the
"no valid pixels" refusal of everything built on it, and scene_frame's refusal of an unlabelled cloud with segments=."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_cloud_ref as C  # noqa: E402
from cppf_amd import scene_poses, scene_stage, training  # noqa: E402
from cppf_amd import scene_training as ST  # noqa: E402
from cppf_amd import segments as SG  # noqa: E402
from cppf_amd.config import CATEGORIES  # noqa: E402
from cppf_amd.frames import NOCS_INTRINSICS  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 48, 64
CFG = CATEGORIES["bottle"]                # res 4 mm, knn 60: a pixel is ~1.4 mm wide at 0.8 m, so a voxel holds several pixels


def small_frame():
    """(depth u16[48,64], labels i32[48,64]): a tilted surface at ~0.8 m beside one at ~1 m; a band of zero-depth rows at the top and
    a zero-depth hole in the middle, so a valid pixel's flat index is not its rank among the valid pixels; labels 0 / 1 by surface
    and -1 on a patch of valid pixels"""
    r, c = np.mgrid[0:H, 0:W]
    depth = (800 + 2 * c + r).astype(np.uint16)
    depth[:, 40:] = (1000 + r[:, 40:]).astype(np.uint16)
    depth[:6] = 0
    depth[20:28, 24:36] = 0
    labels = np.where(c < 40, 0, 1).astype(np.int32)
    labels[30:, 10:20] = -1
    return depth, labels


@pytest.mark.parametrize("case", ["plain", "labels", "labels_jitter"])
def test_scene_cloud_equals_the_hand_composition(dev, case):
    depth, labels = small_frame()
    lab = None if case == "plain" else torch.from_numpy(labels)
    jit = np.random.default_rng(0).standard_normal((H * W, 3)) if case == "labels_jitter" else None
    got = scene_stage.scene_cloud(depth, NOCS_INTRINSICS, CFG, jit, lab)
    want = C.hand_scene_cloud(depth, NOCS_INTRINSICS, CFG, jit, lab)
    assert isinstance(got, scene_stage.SceneCloud) and got._fields == C.FIELDS
    C.assert_same_cloud(got, want)
    assert all(t is None or t.is_contiguous() for t in got)
    M, N = got.hi.shape[0], got.pc.shape[0]
    assert M >= CFG.knn + 1 and 1 < N < M < int((depth > 0).sum()) and got.ind.dtype == torch.int64
    if lab is None:
        assert got.hi_labels is None and got.labels is None
        same = scene_stage.frame_cloud(depth, NOCS_INTRINSICS, CFG)                      # frame_cloud: the same record, no labels
        C.assert_same_cloud(same, want)
    else:
        assert got.hi_labels.dtype == got.labels.dtype == torch.int32
        assert set(torch.unique(got.hi_labels).tolist()) == {-1, 0, 1}
        # the thin callers: a frame object's labels, a segments dict's
        fr = types.SimpleNamespace(depth_mm=depth, intrinsics=NOCS_INTRINSICS, labels=lab)
        C.assert_same_cloud(ST.labelled_cloud(fr, CFG, jit), want)
        C.assert_same_cloud(SG.labelled_frame_cloud(depth, NOCS_INTRINSICS, CFG, dict(labels=lab.to(dev)), jit), want)
    if case == "labels":                  # (a jittered point moves by up to res / 2 = 2 mm, more than a pixel: no projection check there)
        C.assert_labels_at_own_pixel(got.hi, got.hi_labels, labels, NOCS_INTRINSICS)


def test_a_frame_without_valid_pixels_is_refused(dev):
    depth = np.zeros((H, W), np.uint16)
    penc, enc = training.new_encoders(CFG, dev, seed=0)
    fr = types.SimpleNamespace(depth_mm=depth, intrinsics=NOCS_INTRINSICS, labels=torch.zeros((H, W), dtype=torch.int32))
    for call in (lambda: scene_stage.scene_cloud(depth, NOCS_INTRINSICS, CFG),
                 lambda: scene_stage.frame_cloud(depth, NOCS_INTRINSICS, CFG),
                 lambda: scene_stage.frame_inputs(depth, NOCS_INTRINSICS, penc, CFG, 1000, 0),
                 lambda: ST.labelled_cloud(fr, CFG),
                 lambda: scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, CFG, n_pairs=1000)):
        with pytest.raises(ValueError, match="no valid pixels"):
            call()


def test_segments_refuse_a_cloud_without_labels(dev):
    depth, labels = small_frame()
    penc, enc = training.new_encoders(CFG, dev, seed=0)
    seg = dict(labels=torch.from_numpy(labels).to(dev))
    plain = scene_stage.frame_cloud(depth, NOCS_INTRINSICS, CFG)
    with pytest.raises(ValueError, match="labels"):
        scene_poses.scene_frame(depth, NOCS_INTRINSICS, enc, penc, CFG, n_pairs=1000, segments=seg, cloud=plain)
    with pytest.raises(ValueError, match="labels"):
        SG.segment_inputs(depth, NOCS_INTRINSICS, penc, CFG, 1000, 0, seg, cloud=plain)
