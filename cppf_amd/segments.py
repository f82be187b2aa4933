"""Segments of a depth frame, without any network: objects are separated from each other by depth discontinuities
and from what they stand on by a plane.  The mask-free paths draw their pairs uniformly over the whole cloud, so most pairs join two
different objects (3.7e, 3.7i); with a segment per point the draw that training already has (cppf_sample_scene_pairs) takes both
points of a pair from ONE segment.  Everything here is opt-in.

  plane_ransac     cppf_plane_ransac: n_hyp three-point planes and their inlier counts over a cloud, the best of them
  support_mask     up to n_planes dominant planes of a frame's back-projected pixels, one after the other -> the pixels off all of them
  depth_segments   cppf_depth_segments: connected components of the depth image (4-neighbours, a depth-discontinuity rule), the
                   components of min_pixels..max_pixels pixels numbered by their smallest pixel index
  concave_edges    cppf_concave_edges: a plane fit per pixel and the pixels across which the fitted surfaces turn
                   towards each other -- where an object stands on its support or leans on a neighbour; needs no plane model
  frame_segments   support_mask and / or concave_edges, then depth_segments: one dict a caller hands to scene_frame /
                   frame_detections (segments=)
  segment_inputs   scene_stage.cloud_inputs on labelled_frame_cloud's cloud (scene_stage.scene_cloud with the segments' label image),
                   the pairs drawn inside segments (scene_training.sample_scene_pairs)
  segment_clouds   cppf_gather_segments: the labelled cloud's dense points packed segment by segment, and each
                   segment's bounds -- the segments as instance clouds (detections.segment_detections)

The kernels are csrc/segments.hip's and csrc/concave.hip's; the distance tests and compactions of support_mask are torch."""
import numpy as np
import torch

from ._torch_util import call, canon, require_cuda
from .scene_stage import GATHER_CHUNK, GATHER_MAX_CHUNKS, SceneCloud, cloud_inputs, on_device, scene_cloud

F32, I32, I16, U8 = torch.float32, torch.int32, torch.int16, torch.uint8
SEGMENTS_MAX = 1024                       # include/cppf.h: CPPF_SEGMENTS_MAX
PLANE_MAX_HYPOTHESES = 1024               # include/cppf.h: CPPF_PLANE_MAX_HYPOTHESES
MAX_PIXELS = 1 << 24
CONCAVE_MAX_RADIUS, CONCAVE_MAX_STEP = 8, 16  # include/cppf.h: CPPF_CONCAVE_MAX_RADIUS, CPPF_CONCAVE_MAX_STEP
CONCAVE_COS_MAX = float(np.cos(np.deg2rad(30.0)))


def depth_tensor(depth, dev=None):
    """The depth frame as the kernels read it: the int16 bits of the uint16 millimetres, [H,W] on the device.  numpy uint16 / int16 is
    uploaded (to `dev`, default the current HIP device); a device tensor must be int16 (or uint16: reinterpreted).  Anything else --
    float depth, a host tensor -- is refused: nothing is rounded or uploaded behind the caller's back."""
    require_cuda()
    if isinstance(depth, np.ndarray):
        if depth.dtype not in (np.uint16, np.int16):
            raise TypeError(f"depth: expected uint16 millimetres, got {depth.dtype}")
        depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(dev if dev is not None else "cuda")
    if not isinstance(depth, torch.Tensor):
        raise TypeError(f"depth: expected a numpy uint16 array or a device tensor, got {type(depth).__name__}")
    if depth.dtype == getattr(torch, "uint16", None):
        depth = depth.view(I16)
    if depth.dtype != I16:
        raise TypeError(f"depth: expected the int16 bits of the uint16 millimetres, got {depth.dtype}")
    if depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
        raise ValueError(f"depth: expected [H,W], got {tuple(depth.shape)}")
    if not depth.is_cuda:
        raise ValueError(f"depth: a tensor must live on a HIP device, got {depth.device} (hand a numpy array to have it uploaded)")
    return canon(depth, I16, depth.device, "depth")


def check_plane_args(n_points, n_hyp, thresh):
    """cppf_plane_ransac's refusals that need no device, as ValueError"""
    if not 1 <= int(n_points) <= 2 ** 31 - 1:
        raise ValueError(f"plane_ransac takes 1..2^31-1 points, got {n_points}")
    if not 1 <= int(n_hyp) <= PLANE_MAX_HYPOTHESES:
        raise ValueError(f"plane_ransac takes 1..{PLANE_MAX_HYPOTHESES} hypotheses, got {n_hyp}")
    if not (np.isfinite(float(thresh)) and float(thresh) >= 0):
        raise ValueError(f"plane_ransac: thresh must be finite and >= 0, got {thresh}")


def plane_ransac_device(points, n_hyp=256, thresh=0.01, seed=0, out=None):
    """cppf_plane_ransac, enqueued on the current stream with nothing read back: (planes f32[n_hyp,4], counts i32[n_hyp], best i32[2])
    on points' device; out: such a triple to write into (the caller's buffers)"""
    dev = points.device
    check_plane_args(points.shape[0], n_hyp, thresh)
    planes, counts, best = out or (torch.empty((int(n_hyp), 4), dtype=F32, device=dev), torch.empty(int(n_hyp), dtype=I32, device=dev),
                                   torch.empty(2, dtype=I32, device=dev))
    call("cppf_plane_ransac", dev, points, points.shape[0], int(n_hyp), float(thresh), int(seed) & 0xFFFFFFFFFFFFFFFF, planes, counts, best)
    return planes, counts, best


def plane_ransac(points, n_hyp=256, thresh=0.01, seed=0):
    """n_hyp RANSAC plane hypotheses over points f32[N,3] (a device tensor, or a host array that is uploaded) and the best of them.
    Hypothesis h takes three points by Philox (seed, h) and counts the points within `thresh` of their plane (include/cppf.h has the
    arithmetic).  Returns dict(plane f32[4] numpy {n, d} with n.p + d = 0 and d >= 0, or None when every hypothesis is degenerate;
    count, index (-1 then); planes f32[n_hyp,4], counts i32[n_hyp]: device).  One read-back of two integers, and of the one plane."""
    require_cuda()
    dev = points.device if isinstance(points, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    points = on_device(points, dev, "points", (3,))
    if points.dim() != 2:
        raise ValueError(f"points: expected [N,3], got {tuple(points.shape)}")
    planes, counts, best = plane_ransac_device(points, n_hyp, thresh, seed)
    index, count = (int(v) for v in best.cpu().numpy())
    return dict(plane=planes[index].cpu().numpy() if index >= 0 else None, count=count, index=index, planes=planes, counts=counts)


def off_planes(points, planes, band):
    """bool[N]: the points of f32[N,3] further than `band` from every plane of `planes` ([n,4] rows {n, d}; none: all True).  Torch ops
    on points' device (the CPU works); a point that is not finite is off no plane (False) once there is a plane."""
    keep = torch.ones(points.shape[0], dtype=torch.bool, device=points.device)
    for pl in planes:
        pl = torch.as_tensor(np.asarray(pl, np.float32), device=points.device)
        keep &= (points @ pl[:3] + pl[3]).abs() > float(band)
    return keep


def support_mask(depth, intrinsics, n_planes=2, n_hyp=256, thresh=0.01, band=0.015, min_frac=0.05, seed=0):
    """The pixels of a depth frame that lie on none of its dominant planes: (valid u8[H,W] on the device, planes: a list of f32[4]).
    The frame's pixels with depth > 0 are back-projected (utils.util.backproject, metres, no jitter) and planes are fitted to them one
    after the other, up to n_planes: plane j by plane_ransac(seed + j) on the points further than `band` from every earlier plane; the
    loop stops when the best count falls under min_frac of the frame's valid pixels (or nothing is left to fit).  A pixel is valid when
    its depth is > 0 and its point is further than `band` from every plane found."""
    from .utils.util import backproject
    d = depth_tensor(depth)
    dev = d.device
    H, W = d.shape
    valid = torch.zeros(H * W, dtype=U8, device=dev)
    pts, pix = backproject(d, intrinsics, np.ones((H, W), bool), return_device=True)
    n_valid = int(pts.shape[0])
    p = (pts / 1000.0).float().contiguous()
    planes, keep = [], torch.ones(n_valid, dtype=torch.bool, device=dev)
    for j in range(int(n_planes)):
        rest = p[keep].contiguous()
        if rest.shape[0] < 3:
            break
        r = plane_ransac(rest, n_hyp, thresh, int(seed) + j)
        if r["plane"] is None or r["count"] < float(min_frac) * n_valid:
            break
        planes.append(r["plane"])
        keep &= off_planes(p, [r["plane"]], band)
    valid[pix[keep].long()] = 1
    return valid.view(H, W), planes


def check_segment_args(H, W, tol_mm, slope_permille, min_pixels, max_pixels, capacity):
    """cppf_depth_segments' refusals that need no device, as ValueError"""
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) > MAX_PIXELS:
        raise ValueError(f"depth_segments takes frames of 1..2^24 pixels, got {H} x {W}")
    if not 0 <= int(tol_mm) <= 65535 or not 0 <= int(slope_permille) <= 1000:
        raise ValueError(f"depth_segments: tol_mm 0..65535 and slope_permille 0..1000, got {tol_mm}, {slope_permille}")
    if int(min_pixels) < 1 or int(max_pixels) < 0:
        raise ValueError(f"depth_segments: min_pixels >= 1 and max_pixels >= 0 (0: no upper bound), got {min_pixels}, {max_pixels}")
    if not 1 <= int(capacity) <= SEGMENTS_MAX:
        raise ValueError(f"depth_segments lists 1..{SEGMENTS_MAX} segments, got capacity {capacity}")


def depth_segments_device(depth, valid=None, tol_mm=10, slope_permille=10, min_pixels=200, max_pixels=0, capacity=256, out=None):
    """cppf_depth_segments, enqueued on the current stream with nothing read back: dict(labels i32[H,W], comp_size i32[H,W], first
    i32[capacity], sizes i32[capacity], counts i32[4] = {kept, components, live pixels, 0}) on depth's device.  depth: i16[H,W] device
    (depth_tensor's form), valid: u8[H,W] device or None; out: such a dict to write into (the caller's buffers)."""
    dev = depth.device
    H, W = depth.shape
    check_segment_args(H, W, tol_mm, slope_permille, min_pixels, max_pixels, capacity)
    out = out or dict(labels=torch.empty((H, W), dtype=I32, device=dev), comp_size=torch.empty((H, W), dtype=I32, device=dev),
                      first=torch.empty(int(capacity), dtype=I32, device=dev), sizes=torch.empty(int(capacity), dtype=I32, device=dev),
                      counts=torch.empty(4, dtype=I32, device=dev))
    call("cppf_depth_segments", dev, depth, valid, H, W, int(tol_mm), int(slope_permille), int(min_pixels), int(max_pixels), int(capacity),
         out["labels"], out["comp_size"], out["first"], out["sizes"], out["counts"])
    return out


def depth_segments(depth, valid=None, tol_mm=10, slope_permille=10, min_pixels=200, max_pixels=0, capacity=256):
    """Connected components of a depth frame.  depth [H,W]: numpy uint16 millimetres or the device tensor of their int16 bits; valid
    [H,W] bool / uint8 (numpy or device) or None: pixels to leave out.  4-neighbours are linked when |dz| <= tol_mm + slope_permille
    * min(z) / 1000 (integers, floor); the components of min_pixels..max_pixels pixels (max_pixels 0: no upper bound) are numbered by
    their smallest pixel index.  Returns dict(labels i32[H,W] (-1: no kept component), comp_size i32[H,W], first i32[S], sizes i32[S]:
    device; n_segments = S, n_components, n_live: ints).  One read-back of the counts; where S passes `capacity` the kernel runs once
    more with capacity S, and S > 1024 raises ValueError (raise min_pixels)."""
    d = depth_tensor(depth, valid.device if isinstance(valid, torch.Tensor) and valid.is_cuda and isinstance(depth, np.ndarray) else None)
    dev = d.device
    if valid is not None:
        if isinstance(valid, np.ndarray):
            valid = torch.from_numpy(np.ascontiguousarray(valid.astype(np.uint8))).to(dev)
        if isinstance(valid, torch.Tensor) and valid.dtype == torch.bool:
            valid = valid.to(U8)
        valid = canon(valid, U8, dev, "valid")
        if tuple(valid.shape) != tuple(d.shape):
            raise ValueError(f"valid {tuple(valid.shape)} and depth {tuple(d.shape)} must be the same [H,W]")
    out = depth_segments_device(d, valid, tol_mm, slope_permille, min_pixels, max_pixels, capacity)
    S, n_comp, n_live, _ = (int(v) for v in out["counts"].cpu().numpy())
    if S > int(capacity):
        if S > SEGMENTS_MAX:
            raise ValueError(f"depth_segments: {S} components pass the size filter; one call lists at most {SEGMENTS_MAX} (raise min_pixels)")
        out = depth_segments_device(d, valid, tol_mm, slope_permille, min_pixels, max_pixels, S)
    return dict(labels=out["labels"], comp_size=out["comp_size"], first=out["first"][:S], sizes=out["sizes"][:S], n_segments=S,
                n_components=n_comp, n_live=n_live)


def concave_options(radius=3, step=4, tol_mm=10, slope_permille=10, min_count=None, cos_max=CONCAVE_COS_MAX, span_max=0.08):
    """cppf_concave_edges' options with their defaults filled in (min_count None: a third of the window, (2 radius + 1)^2 // 3)"""
    r = int(radius)
    return dict(radius=r, step=int(step), tol_mm=int(tol_mm), slope_permille=int(slope_permille),
                min_count=(2 * r + 1) ** 2 // 3 if min_count is None else int(min_count), cos_max=float(cos_max), span_max=float(span_max))


def check_concave_args(H, W, intrinsics, radius, step, tol_mm, slope_permille, min_count, cos_max, span_max):
    """cppf_concave_edges' refusals that need no device, as ValueError; returns (fx, fy, cx, cy) as floats"""
    K = np.asarray(intrinsics, np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"concave_edges: intrinsics must be a 3x3 matrix, got {K.shape}")
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        raise ValueError(f"concave_edges: fx, fy finite and > 0, cx, cy finite, got {fx}, {fy}, {cx}, {cy}")
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) > MAX_PIXELS:
        raise ValueError(f"concave_edges takes frames of 1..2^24 pixels, got {H} x {W}")
    if not 1 <= int(radius) <= CONCAVE_MAX_RADIUS or not 1 <= int(step) <= CONCAVE_MAX_STEP:
        raise ValueError(f"concave_edges: radius 1..{CONCAVE_MAX_RADIUS} and step 1..{CONCAVE_MAX_STEP}, got {radius}, {step}")
    if not 0 <= int(tol_mm) <= 65535 or not 0 <= int(slope_permille) <= 1000:
        raise ValueError(f"concave_edges: tol_mm 0..65535 and slope_permille 0..1000, got {tol_mm}, {slope_permille}")
    if int(min_count) < 3:
        raise ValueError(f"concave_edges: a plane takes min_count >= 3 pixels, got {min_count}")
    if not -1.0 < float(cos_max) < 1.0:
        raise ValueError(f"concave_edges: cos_max must lie inside (-1, 1), got {cos_max}")
    if not (np.isfinite(float(span_max)) and float(span_max) > 0):
        raise ValueError(f"concave_edges: span_max must be finite and > 0, got {span_max}")
    return fx, fy, cx, cy


def concave_edges_device(depth, intrinsics, valid=None, radius=3, step=4, tol_mm=10, slope_permille=10, min_count=None,
                         cos_max=CONCAVE_COS_MAX, span_max=0.08, out=None):
    """cppf_concave_edges, enqueued on the current stream with nothing read back: dict(edge u8[H,W], normal f64[H,W,3], counts i32[4] =
    {edge pixels, pixels with a fit, live pixels, 0}) on depth's device.  depth: i16[H,W] device (depth_tensor's form), valid: u8[H,W]
    device or None, intrinsics: the 3x3 matrix of the integer pixel coordinates; out: such a dict to write into."""
    dev = depth.device
    H, W = depth.shape
    o = concave_options(radius, step, tol_mm, slope_permille, min_count, cos_max, span_max)
    fx, fy, cx, cy = check_concave_args(H, W, intrinsics, **o)
    out = out or dict(edge=torch.empty((H, W), dtype=U8, device=dev), normal=torch.empty((H, W, 3), dtype=torch.float64, device=dev),
                      counts=torch.empty(4, dtype=I32, device=dev))
    call("cppf_concave_edges", dev, depth, valid, H, W, fx, fy, cx, cy, o["radius"], o["step"], o["tol_mm"], o["slope_permille"],
         o["min_count"], o["cos_max"], o["span_max"], out["edge"], out["normal"], out["counts"])
    return out


def valid_tensor(valid, d):
    """a `valid` mask ([H,W] bool / uint8, numpy or device, or None) as u8[H,W] on the device of the depth tensor d"""
    if valid is None:
        return None
    if isinstance(valid, np.ndarray):
        valid = torch.from_numpy(np.ascontiguousarray(valid.astype(np.uint8))).to(d.device)
    if isinstance(valid, torch.Tensor) and valid.dtype == torch.bool:
        valid = valid.to(U8)
    valid = canon(valid, U8, d.device, "valid")
    if tuple(valid.shape) != tuple(d.shape):
        raise ValueError(f"valid {tuple(valid.shape)} and depth {tuple(d.shape)} must be the same [H,W]")
    return valid


def concave_edges(depth, intrinsics, valid=None, **options):
    """The concave creases of a depth frame (include/cppf.h "Concave edges"): a plane is fitted to every live pixel's (2 radius + 1)^2
    window (pixels within tol_mm + slope_permille z / 1000 per pixel of distance; at least min_count of them), and a live pixel is an
    edge when the fitted surfaces `step` pixels to either side of it, horizontally or vertically, are at most span_max metres apart,
    differ by more than acos(cos_max) and turn towards each other.  depth [H,W]: numpy uint16 millimetres or the device tensor of
    their int16 bits; valid as depth_segments takes it.  Returns dict(edge u8[H,W], normal f64[H,W,3]: device; n_edge, n_fit, n_live:
    ints; options).  One read-back of the counts."""
    d = depth_tensor(depth, valid.device if isinstance(valid, torch.Tensor) and valid.is_cuda and isinstance(depth, np.ndarray) else None)
    out = concave_edges_device(d, intrinsics, valid_tensor(valid, d), **options)
    n_edge, n_fit, n_live, _ = (int(v) for v in out["counts"].cpu().numpy())
    return dict(edge=out["edge"], normal=out["normal"], n_edge=n_edge, n_fit=n_fit, n_live=n_live, options=concave_options(**options))


def frame_segments(depth, intrinsics, n_planes=2, n_hyp=256, thresh=0.01, band=0.015, min_frac=0.05, seed=0, tol_mm=10, slope_permille=10,
                   min_pixels=200, max_pixels=0, capacity=256, concave=None):
    """support_mask (skipped at n_planes = 0: frames with no background) and then depth_segments on what it leaves.  Returns one
    dict: labels i32[H,W], sizes, first (device), n_segments, n_components, valid (u8[H,W] device, or None at n_planes = 0), planes
    (list of f32[4]) and options (the arguments above): what scene_frame / frame_detections take as segments=.
    concave: None, or a dict of concave_edges' options ({} for its defaults).  The creases of the frame (concave_edges on the whole
    frame, no mask) are then cut out as well: valid = support_mask's (all ones at n_planes = 0) AND edge == 0.  The crease pixels
    stay unlabelled (-1); labels are not grown back over the cut band.  The dict gains edge (u8[H,W] device) and concave (the options
    with their defaults filled in); without concave= it has exactly the keys above."""
    options = dict(n_planes=int(n_planes), n_hyp=int(n_hyp), thresh=float(thresh), band=float(band), min_frac=float(min_frac), seed=int(seed),
                   tol_mm=int(tol_mm), slope_permille=int(slope_permille), min_pixels=int(min_pixels), max_pixels=int(max_pixels),
                   capacity=int(capacity))
    d = depth_tensor(depth)
    valid, planes = (None, []) if int(n_planes) == 0 else support_mask(d, intrinsics, n_planes, n_hyp, thresh, band, min_frac, seed)
    extra = {}
    if concave is not None:
        c = concave_edges_device(d, intrinsics, None, **concave)
        valid = (c["edge"] == 0).to(U8) if valid is None else valid * (c["edge"] == 0).to(U8)
        extra = dict(edge=c["edge"], concave=concave_options(**concave))
    s = depth_segments(d, valid, tol_mm, slope_permille, min_pixels, max_pixels, capacity)
    return dict(labels=s["labels"], sizes=s["sizes"], first=s["first"], n_segments=s["n_segments"], n_components=s["n_components"],
                valid=valid, planes=planes, options=options, **extra)


def segment_labels(segments):
    """the label image of `segments` (frame_segments' dict, or anything with labels [H,W] integers, device or numpy) as a tensor"""
    labels = segments["labels"] if isinstance(segments, dict) else segments
    if isinstance(labels, np.ndarray) and labels.dtype.kind in "iu":
        labels = torch.from_numpy(np.ascontiguousarray(labels.astype(np.int32)))
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or labels.dtype.is_floating_point:
        raise TypeError("segments: expected frame_segments' dict (labels: an integer image [H,W])")
    return labels


def labelled_frame_cloud(depth, intrinsics, cfg, segments, jitter=None):
    """scene_stage.scene_cloud with segments' label image (checked here to be an integer image of the depth frame's shape): the
    SceneCloud (hi, hi_nrm, hi_labels, ind, pc, nrm, labels) that segment_inputs, scene_frame and frame_detections take as cloud="""
    labels = segment_labels(segments)
    d = np.asarray(depth) if not isinstance(depth, torch.Tensor) else depth
    if tuple(labels.shape) != tuple(d.shape):
        raise ValueError(f"segments: labels {tuple(labels.shape)} for a depth frame {tuple(d.shape)}")
    return scene_cloud(depth, intrinsics, cfg, jitter, labels=labels)


def segment_members(inst, n_segments, min_points=8):
    """(members, seg_off, n_qualifying): scene_training.target_members with the flag set for exactly the segments that have at least
    min_points points in the sparse cloud (inst i32[N], device)"""
    from .scene_training import FLAG_TARGET, target_members
    K = max(int(n_segments), 1)
    lab = inst.long()
    counts = torch.bincount(lab[lab >= 0].clamp(max=K - 1), minlength=K)[:K].cpu().numpy()
    flags = np.where(counts >= max(int(min_points), 1), FLAG_TARGET, 0).astype(np.int32)
    members, seg_off = target_members(inst, flags)
    return members, seg_off, int((flags != 0).sum())


def segment_inputs(depth, intrinsics, point_encoder, cfg, n_pairs, seed, segments, intra_frac=1.0, min_points=8, jitter=None, cloud=None):
    """scene_stage.cloud_inputs on the labelled cloud with the pairs drawn inside segments.  Returns frame_inputs' tuple plus the
    per-point segment ids of the sparse cloud: hi, hi_nrm, ind, pc, nrm, feat, idx, (u_tr, u_rot), inst.
    The pair list is scene_training.sample_scene_pairs(members, seg_off, inst, n_pairs, round(intra_frac n_pairs), seed): the first
    round(intra_frac n_pairs) pairs join two points of ONE segment, a segment drawn in proportion to its points; the rest are uniform
    over the cloud (the scene draw's uniform rule on Philox stream 4 -- not draw_pairs' pairs).  members: the points of the segments
    with at least min_points sparse points; when no segment qualifies every pair is uniform.  segments: frame_segments' dict; cloud:
    labelled_frame_cloud's for this frame and a config with the same (res, knn) (None: computed here); one without labels is refused."""
    from .scene_training import sample_scene_pairs
    if not 0.0 <= float(intra_frac) <= 1.0:
        raise ValueError(f"intra_frac must be in [0, 1], got {intra_frac}")
    if cloud is None:
        cloud = labelled_frame_cloud(depth, intrinsics, cfg, segments, jitter)
    if not isinstance(cloud, SceneCloud) or cloud.labels is None:
        raise ValueError("segments= needs a cloud with labels (segments.labelled_frame_cloud's SceneCloud), got one without")
    P, inst = int(n_pairs), cloud.labels
    n_seg = int(inst.max().item()) + 1 if inst.numel() else 0
    members, seg_off, _ = segment_members(inst, n_seg, min_points)
    idx = sample_scene_pairs(members, seg_off, inst, P, int(round(float(intra_frac) * P)), seed).long()
    return (*cloud_inputs(cloud, point_encoder, P, seed, pairs=idx), inst)


def check_segment_cloud_args(n_segments, n_dense, capacity):
    """cppf_gather_segments' refusals that need no device, as ValueError"""
    S, M, cap = int(n_segments), int(n_dense), int(capacity)
    if not 1 <= S <= SEGMENTS_MAX:
        raise ValueError(f"segment_clouds takes 1..{SEGMENTS_MAX} segments, got {S}")
    if M < 0 or cap < 0:
        raise ValueError(f"negative size: n_dense {M}, capacity {cap}")
    if M > 2 ** 31 - 1:
        raise ValueError(f"{M} dense points pass the int32 offsets")
    if (M + GATHER_CHUNK - 1) // GATHER_CHUNK > GATHER_MAX_CHUNKS:
        raise ValueError(f"{M} dense points: one call takes at most {GATHER_CHUNK * GATHER_MAX_CHUNKS}")


def _labelled(cloud, who):
    if not isinstance(cloud, SceneCloud) or cloud.hi_labels is None:
        raise ValueError(f"{who} needs a cloud with labels (segments.labelled_frame_cloud's SceneCloud), got one without")
    return cloud


def segment_clouds_device(cloud, n_segments, capacity=None, out=None):
    """cppf_gather_segments on labelled_frame_cloud's SceneCloud, enqueued on the current stream with nothing read back: the dense
    cloud packed segment by segment.  Returns dict(offsets i32[S+1], pts f32[capacity,3], nrm f32[capacity,3], src i32[capacity],
    bounds f32[S,6] = {min x, y, z, max x, y, z} of each segment's finite points) of device tensors; segment s's points are rows
    offsets[s]:offsets[s+1], in increasing dense index -- cloud.hi[cloud.hi_labels == s].  capacity: the dense cloud's size by
    default (segments are disjoint: always enough); out: such a dict to write into (the caller's buffers)."""
    cloud = _labelled(cloud, "segment_clouds")
    hi, hi_nrm, lab = cloud.hi, cloud.hi_nrm, cloud.hi_labels
    dev = hi.device
    S, M = int(n_segments), hi.shape[0]
    capacity = M if capacity is None else int(capacity)
    check_segment_cloud_args(S, M, capacity)
    if out is None:
        out = dict(offsets=torch.empty(S + 1, dtype=I32, device=dev), pts=torch.empty((max(capacity, 1), 3), dtype=F32, device=dev),
                   nrm=torch.empty((max(capacity, 1), 3), dtype=F32, device=dev), src=torch.empty(max(capacity, 1), dtype=I32, device=dev),
                   bounds=torch.empty((S, 6), dtype=F32, device=dev))
    counts = torch.empty(max(S * ((M + GATHER_CHUNK - 1) // GATHER_CHUNK), 1), dtype=I32, device=dev)
    call("cppf_gather_segments", dev, hi, hi_nrm, lab, S, M, capacity, out["offsets"], out["pts"], out["nrm"], out["src"], out.get("bounds"),
         counts)
    return out


def segment_clouds(cloud, n_segments):
    """The segments of a labelled frame cloud as instance clouds: dict(clouds: a list of S (pts f32[n_s,3], nrm f32[n_s,3]) views of
    the packed device buffers, segment s = cloud.hi[cloud.hi_labels == s] and its normals; offsets i64[S+1] numpy; pts, nrm, src: the
    packed device buffers (T rows); bounds f32[S,6] device).  One call, one read-back of the S + 1 offsets.  cloud: labelled_frame_cloud's
    SceneCloud; one without hi_labels is refused (ValueError).  n_segments = 0: no segments, nothing is launched."""
    cloud = _labelled(cloud, "segment_clouds")
    dev, S = cloud.hi.device, int(n_segments)
    if S == 0:
        return dict(clouds=[], offsets=np.zeros(1, np.int64), pts=cloud.hi[:0], nrm=cloud.hi_nrm[:0],
                    src=torch.empty(0, dtype=I32, device=dev), bounds=torch.empty((0, 6), dtype=F32, device=dev))
    hi, hi_nrm, lab = (canon(cloud.hi, F32, dev, "hi", (3,)), canon(cloud.hi_nrm, F32, dev, "hi_nrm", (3,)),
                       canon(cloud.hi_labels, I32, dev, "hi_labels"))
    if lab.shape != (hi.shape[0],) or hi_nrm.shape != hi.shape:
        raise ValueError(f"segment_clouds: hi {tuple(hi.shape)}, hi_nrm {tuple(hi_nrm.shape)}, hi_labels {tuple(lab.shape)}: expected "
                         "[M,3], [M,3], [M]")
    g = segment_clouds_device(cloud._replace(hi=hi, hi_nrm=hi_nrm, hi_labels=lab), S)
    off = g["offsets"].cpu().numpy().astype(np.int64)
    T = int(off[S])
    pts, nrm = g["pts"][:T], g["nrm"][:T]
    return dict(clouds=[(pts[int(a):int(b)], nrm[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])], offsets=off, pts=pts, nrm=nrm,
                src=g["src"][:T], bounds=g["bounds"])


__all__ = ["plane_ransac", "support_mask", "depth_segments", "frame_segments", "segment_inputs", "labelled_frame_cloud", "segment_members",
           "depth_tensor", "off_planes", "concave_edges", "concave_edges_device", "concave_options", "check_concave_args",
           "segment_clouds", "segment_clouds_device", "check_segment_cloud_args"]
