"""Mesh frames: several posed meshes rendered into ONE depth image with an instance label per pixel (meshes.render_instances,
include/cppf.h: cppf_raster_instances), in exactly the form the frame path reads -- uint16 millimetres, instance masks,
intrinsics (frames.frame_poses / FrameRunner.run) -- together with the ground-truth records evaluation.compute_degree_cm_mAP
scores poses against.  Objects occlude each other in the image; their answer is known.

Coordinates.  The render's camera frame is OpenGL's (the camera looks down -z, y up) and it samples pixel CENTRES with no
principal-point offset: pixel (col c, row r) sees the ray x / d = (c + 0.5 - W/2) / fx, y / d = -(r + 0.5 - H/2) / fy.  The frame
path (utils.util.backproject with integer pixel coordinates, / 1000, frames.instance_cloud's x / y negation) returns
((c - cx) z / fx, (r - cy) z / fy, z).  So with cx = W/2 - 0.5, cy = H/2 - 0.5 (`frame_intrinsics`) the frame path returns the
rendered surface points in FRAME coordinates = FRAME_FROM_GL . (OpenGL camera coordinates), FRAME_FROM_GL = diag(1, -1, -1): x
right, y down, z forward.  tests/test_mesh_frames_cpu.py decides this on a slanted plane."""
import numpy as np
import torch

from . import meshes as M
from .config import CATEGORIES, NOCS_CATEGORIES
from .evaluation import SYNSET_NAMES, _UP_SYMMETRIC

FRAME_FROM_GL = np.diag([1.0, -1.0, -1.0])
Z_RANGE = (0.6, 2.0)                     # draw_pose's depth range for the NOCS categories (utils/dataset.py:143-150)


def frame_intrinsics(fx=M.FX, fy=M.FY, width=M.WIDTH, height=M.HEIGHT):
    """the 3x3 matrix for which the frame path's back-projection of a rendered depth image returns the rendered surface"""
    return np.array([[fx, 0.0, width / 2 - 0.5], [0.0, fy, height / 2 - 0.5], [0.0, 0.0, 1.0]])


def depth_to_mm(depth):
    """f32 metres -> the uint16 millimetres of a NOCS depth PNG: min(65535, rint(1000 * depth)) in fp64, 0 for background (numpy)"""
    d = depth.detach().cpu().numpy() if isinstance(depth, torch.Tensor) else np.asarray(depth)
    return np.minimum(65535.0, np.rint(1000.0 * d.astype(np.float64))).astype(np.uint16)


def ground_truth(R_mesh, t, scale, bmin, bmax, is_nocs):
    """(centre, R, half_extents) of one posed mesh in FRAME coordinates, built as MeshViewSampler.sample(canonical=False) builds
    them in the render's: R's columns are the object's axes (FLIP2NOCS for the NOCS categories), half_extents are
    view_half_extents' (x and z swapped, unconditionally)."""
    Robj = R_mesh @ M.FLIP2NOCS.T if is_nocs else np.asarray(R_mesh, np.float64)
    return FRAME_FROM_GL @ np.asarray(t, np.float64), FRAME_FROM_GL @ Robj, M.view_half_extents(bmin, bmax, scale)


class MeshFrame:
    """One rendered frame.  depth f32[H,W] metres and labels i32[H,W] (instance index, -1 = background) as render_instances
    returns them (device tensors; host tensors or numpy arrays work too), categories: one name per instance, and per instance
    the ground truth in frame coordinates: centers f64[K,3], Rs f64[K,3,3], half_extents f64[K,3].

    depth_mm          uint16[H,W] numpy, what frame_poses / FrameRunner.run take as `depth`
    intrinsics        frame_intrinsics of the render
    visible_pixels    i64[K]: pixels each instance kept (torch.bincount of the labels)
    gt_RTs, gt_scales the NOCS-record form: gt_RTs[k][:3,:3] = R |2 half|, gt_RTs[k][:3,3] = centre, gt_scales[k] = 2 half / |2 half|
                      (what estimate_pose's results become in nocs/inference.py:335-339)"""

    def __init__(self, depth, labels, categories, centers, Rs, half_extents, intrinsics, synset_names=SYNSET_NAMES, spec=None):
        self.depth = depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(depth, np.float32))
        self.labels = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels, np.int32))
        self.categories = list(categories)
        K = len(self.categories)
        self.centers = np.asarray(centers, np.float64).reshape(K, 3)
        self.Rs = np.asarray(Rs, np.float64).reshape(K, 3, 3)
        self.half_extents = np.asarray(half_extents, np.float64).reshape(K, 3)
        self.intrinsics = np.asarray(intrinsics, np.float64)
        self.synset_names = list(synset_names)
        self.spec = spec
        self.depth_mm = depth_to_mm(self.depth)
        lab = self.labels.reshape(-1)
        self.visible_pixels = torch.bincount(lab[lab >= 0].long(), minlength=K)[:K].cpu().numpy().astype(np.int64)
        self._labels_host = None
        size = 2.0 * self.half_extents
        norm = np.linalg.norm(size, axis=1)
        self.gt_RTs = np.tile(np.eye(4), (K, 1, 1))
        self.gt_RTs[:, :3, :3] = self.Rs * norm[:, None, None]
        self.gt_RTs[:, :3, 3] = self.centers
        self.gt_scales = size / norm[:, None]
        self.gt_class_ids = np.array([self.synset_names.index(c) for c in self.categories], np.int32)

    def visible(self, min_pixels=100):
        """indices of the instances that kept at least `min_pixels` pixels"""
        return [int(k) for k in np.nonzero(self.visible_pixels >= max(1, int(min_pixels)))[0]]

    def mask(self, k):
        if self._labels_host is None:
            self._labels_host = self.labels.cpu().numpy()
        return self._labels_host == k

    def instances(self, min_pixels=100):
        """[(category, mask bool[H,W] numpy)] of the instances visible(min_pixels) lists: the form frame_poses / FrameRunner.run take"""
        return [(self.categories[k], self.mask(k)) for k in self.visible(min_pixels)]

    def gt_poses(self, min_pixels=100):
        """the ground truth of the visible instances as pose dicts (T, R, scale, scale_norm: what record() reads of a pose)"""
        out = []
        for k in self.visible(min_pixels):
            size = 2.0 * self.half_extents[k]
            out.append(dict(T=self.centers[k].copy(), R=self.Rs[k].copy(), scale=size, scale_norm=float(np.linalg.norm(size))))
        return out

    def record(self, poses, scores=None, min_pixels=100):
        """One result dict with the keys evaluation.compute_degree_cm_mAP reads.  poses: one pose dict (estimate_pose's keys T, R,
        scale, scale_norm) or None per instance of instances(min_pixels), in that order; a None (an instance the frame path
        skipped) makes no prediction.  scores: one per pose (default 1).  Every instance is ground truth: one that was not
        visible enough stays unmatched."""
        vis = self.visible(min_pixels)
        if len(poses) != len(vis):
            raise ValueError(f"{len(poses)} poses for the {len(vis)} instances with at least {min_pixels} pixels")
        scores = np.ones(len(vis)) if scores is None else np.asarray(scores, np.float64).reshape(len(vis))
        kept = [j for j, p in enumerate(poses) if p is not None]
        RTs = np.tile(np.eye(4), (len(kept), 1, 1))
        scales = np.ones((len(kept), 3))
        for i, j in enumerate(kept):
            p = poses[j]
            if not p["scale_norm"] > 0:
                raise ValueError(f"pose {j}: scale_norm {p['scale_norm']}")
            RTs[i, :3, :3] = np.asarray(p["R"], np.float64) * float(p["scale_norm"])          # nocs/inference.py:335-339
            RTs[i, :3, 3] = np.asarray(p["T"], np.float64)
            scales[i] = np.asarray(p["scale"], np.float64) / float(p["scale_norm"])
        K = len(self.categories)
        return dict(gt_class_ids=self.gt_class_ids.copy(), gt_RTs=self.gt_RTs.copy(), gt_scales=self.gt_scales.copy(),
                    gt_handle_visibility=np.ones(K, np.int32),
                    gt_up_syms=np.array([c in _UP_SYMMETRIC for c in self.categories], bool),
                    pred_class_ids=self.gt_class_ids[[vis[j] for j in kept]].astype(np.int32), pred_RTs=RTs, pred_scales=scales,
                    pred_scores=scores[kept].astype(np.float64), gt_visible_pixels=self.visible_pixels.copy())


def bounding_radius(vertices, faces, bmin, bmax):
    """the radius of the sphere about the box centre (bmin + bmax) / 2 that holds every vertex some face references"""
    used = np.asarray(vertices, np.float64)[np.unique(np.asarray(faces))]
    return float(np.sqrt(((used - (np.asarray(bmin) + np.asarray(bmax)) / 2) ** 2).sum(1).max()))


class MeshFrameSampler:
    """Frames of `n_objects` posed meshes.  category_meshes: {category: [(vertices, faces) pairs or OBJ paths]}; cfgs: {category:
    CategoryConfig} (default config.CATEGORIES; every category needs a scale_range).

    draw() is host work only.  From ONE np.random.Generator(seed) it draws, object by object (j = 0 .. n_objects - 1):
      1. the category:  rng.integers(number of categories), over the categories in the order given;
      2. the mesh:      rng.integers(number of meshes of that category);
      3. the scale:     rng.uniform(scale_range[0], scale_range[1]), as MeshViewSampler does;
      4. the rotation:  meshes.draw_pose(rng, category in NOCS_CATEGORIES) -- its translation is drawn too and discarded;
      5. the translation, up to max_attempts times: d = rng.uniform(z_range), then x = rng.uniform(-1, 1) * max(0, d W / (2 fx) - r),
         y = rng.uniform(-1, 1) * max(0, d H / (2 fy) - r), t = (x, y, -d) in the render's camera frame, r = the scale times the
         mesh's bounding radius: the sphere's centre stays so far inside the view frustum that the sphere does (to first order).
         A draw is kept when its bounding sphere intersects none of the spheres placed before (in 3D; the objects still occlude
         each other in the image).  max_attempts refusals in a row raise RuntimeError.
    sample() = draw() + one render_instances call -> MeshFrame.  The same seed gives the same frames bit for bit."""

    def __init__(self, category_meshes, n_objects, device=None, seed=0, cfgs=None, z_range=Z_RANGE, max_attempts=100,
                 fx=M.FX, fy=M.FY, width=M.WIDTH, height=M.HEIGHT, znear=M.ZNEAR, synset_names=None):
        self.categories = list(category_meshes)
        if not self.categories or n_objects < 1:
            raise ValueError("at least one category and one object")
        self.cfgs = cfgs or CATEGORIES
        self.meshes, self.index = [], {}                        # host meshes in one list; (category, i) -> position in it
        self.bounds, self.radius = [], []
        for cat in self.categories:
            if self.cfgs[cat].scale_range is None:
                raise ValueError(f"category {cat}: no scale_range in its config")
            if not category_meshes[cat]:
                raise ValueError(f"category {cat}: no meshes")
            for i, m in enumerate(category_meshes[cat]):
                v, f = M.load_obj(m) if isinstance(m, str) else m
                v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int32)
                bmin, bmax = M.mesh_bounds(v, f)
                self.index[(cat, i)] = len(self.meshes)
                self.meshes.append((v, f))
                self.bounds.append((bmin, bmax))
                self.radius.append(bounding_radius(v, f, bmin, bmax))
        self.n_meshes = {cat: len(category_meshes[cat]) for cat in self.categories}
        self.n_objects, self.max_attempts, self.z_range = int(n_objects), int(max_attempts), (float(z_range[0]), float(z_range[1]))
        self.fx, self.fy, self.width, self.height, self.znear = fx, fy, int(width), int(height), znear
        self.synset_names = list(synset_names) if synset_names is not None else (
            SYNSET_NAMES if all(c in SYNSET_NAMES for c in self.categories) else ["BG"] + self.categories)
        self.rng = np.random.default_rng(seed)
        self.dev = device
        self._set = None

    def draw(self):
        """the host draws of one frame: dict(categories, inst_mesh i32[K], scales, Rs (the meshes' rotations), ts (camera frame of
        the render), radii, model_views f64[K,4,4], centers / gt_Rs / half_extents (frame coordinates))"""
        rng, K = self.rng, self.n_objects
        cats, inst, scales, Rs, ts, radii, models, gts = [], [], [], [], [], [], [], []
        for _ in range(K):
            cat = self.categories[int(rng.integers(len(self.categories)))]
            m = self.index[(cat, int(rng.integers(self.n_meshes[cat])))]
            cfg = self.cfgs[cat]
            scale = rng.uniform(cfg.scale_range[0], cfg.scale_range[1])
            R, _ = M.draw_pose(rng, cat in NOCS_CATEGORIES)
            r = scale * self.radius[m]
            for _ in range(self.max_attempts):
                d = rng.uniform(self.z_range[0], self.z_range[1])
                x = rng.uniform(-1.0, 1.0) * max(0.0, d * self.width / (2 * self.fx) - r)
                y = rng.uniform(-1.0, 1.0) * max(0.0, d * self.height / (2 * self.fy) - r)
                t = np.array([x, y, -d])
                if all(np.linalg.norm(t - t2) > r + r2 for t2, r2 in zip(ts, radii)):
                    break
            else:
                raise RuntimeError(f"{self.max_attempts} placements in a row intersected an object placed before")
            bmin, bmax = self.bounds[m]
            cats.append(cat); inst.append(m); scales.append(scale); Rs.append(R); ts.append(t); radii.append(r)
            models.append(M.model_matrix(R, t, scale, bmin, bmax))
            gts.append(ground_truth(R, t, scale, bmin, bmax, cat in NOCS_CATEGORIES))
        return dict(categories=cats, inst_mesh=np.asarray(inst, np.int32), scales=np.asarray(scales), Rs=np.asarray(Rs),
                    ts=np.asarray(ts), radii=np.asarray(radii), model_views=np.asarray(models),
                    centers=np.asarray([g[0] for g in gts]), gt_Rs=np.asarray([g[1] for g in gts]),
                    half_extents=np.asarray([g[2] for g in gts]))

    def frame(self, spec, depth, labels):
        """the MeshFrame of a draw and its rendered images"""
        return MeshFrame(depth, labels, spec["categories"], spec["centers"], spec["gt_Rs"], spec["half_extents"],
                         frame_intrinsics(self.fx, self.fy, self.width, self.height), self.synset_names, spec)

    def sample(self, cull=True):
        M.require_cuda()
        dev = self.dev or torch.device("cuda", 0)
        if self._set is None:
            self._set = M.mesh_set(self.meshes, dev)
        spec = self.draw()
        depth, labels = M.render_instances(self._set, spec["inst_mesh"], spec["model_views"], cull=cull, fx=self.fx, fy=self.fy,
                                           width=self.width, height=self.height, znear=self.znear, device=dev)
        return self.frame(spec, depth, labels)
