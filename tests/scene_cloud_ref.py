"""The clouds of a whole depth frame composed by hand from the single public calls (cppf_amd.utils.util): the independent side of
every test of scene_stage.scene_cloud and of what is built on it (frame_cloud, frame_inputs, labelled_cloud, labelled_frame_cloud,
segment_inputs).  Needs a HIP device, like the calls it makes."""
import numpy as np
import torch

from cppf_amd.utils.util import backproject, estimate_normals, sparse_quantize

FIELDS = ("hi", "hi_nrm", "hi_labels", "ind", "pc", "nrm", "labels")


def hand_scene_cloud(depth, intrinsics, cfg, jitter=None, labels=None):
    """(hi, hi_nrm, hi_labels, ind, pc, nrm, labels): nocs/zero_shot.ipynb cell 3 -- back-projection of every pixel, /1000, the jitter
    clamp, the two negations, sparse_quantize at res, normals, sparse_quantize at 4 res -- and the label image (integers [H,W], numpy
    or tensor; None: both label fields None) read at each dense point's own flat pixel index"""
    pts, pix = backproject(depth, intrinsics, np.ones(tuple(depth.shape), bool), return_device=True)
    p = pts / 1000.0
    if jitter is not None:
        j = torch.as_tensor(jitter, dtype=torch.float64, device=p.device)[:p.shape[0]]
        p = p + torch.clamp(cfg.res / 4 * j, -cfg.res / 2, cfg.res / 2)
    p = torch.stack([-p[:, 0], -p[:, 1], p[:, 2]], -1)
    _, keep = sparse_quantize(p.float(), return_index=True, quantization_size=cfg.res)
    hi = p[keep].float()
    hi_nrm = estimate_normals(hi, cfg.knn)
    _, ind = sparse_quantize(hi, return_index=True, quantization_size=4 * cfg.res)
    hi_labels = None
    if labels is not None:
        hi_labels = torch.as_tensor(labels).to(p.device).reshape(-1)[pix[keep].long()].to(torch.int32)
    return hi, hi_nrm, hi_labels, ind, hi[ind], hi_nrm[ind], None if labels is None else hi_labels[ind]


def assert_same_cloud(got, want, fields=FIELDS):
    """the named fields of two 7-tuples agree in presence, dtype, shape and every bit"""
    for name in fields:
        a, b = got[FIELDS.index(name)], want[FIELDS.index(name)]
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
            bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
            assert torch.equal(bits(a), bits(b)), name


def assert_labels_at_own_pixel(hi, hi_labels, label_image, intrinsics):
    """every dense point (no jitter) projects back into the pixel its label was read from: the frame path returns ((c - cx) z / fx,
    (r - cy) z / fy, z)"""
    p = hi.double().cpu().numpy()
    col = np.rint(p[:, 0] / p[:, 2] * intrinsics[0, 0] + intrinsics[0, 2]).astype(np.int64)
    row = np.rint(p[:, 1] / p[:, 2] * intrinsics[1, 1] + intrinsics[1, 2]).astype(np.int64)
    assert np.array_equal(np.asarray(label_image)[row, col], hi_labels.cpu().numpy())
