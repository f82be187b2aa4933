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


MAX_INSTANCES = 65536                    # include/cppf.h: cppf_raster_instances' limit on K
# the support of a tabletop frame in its own coordinates: the unit square of the xz plane, facing +y (counter-clockwise seen from +y)
PLANE_MESH = (np.array([[-1.0, 0.0, -1.0], [-1.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 0.0, -1.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def footprint_radius(vertices, faces, bmin, bmax):
    """the radius of the circle about the box centre, in the mesh's xz plane, that holds every vertex some face references"""
    used = np.asarray(vertices, np.float64)[np.unique(np.asarray(faces))]
    c = (np.asarray(bmin) + np.asarray(bmax)) / 2
    return float(np.sqrt(((used[:, [0, 2]] - c[[0, 2]]) ** 2).sum(1).max()))


def plane_quad(up, point, fx, fy, width, height, far, margin=1.1, pad=0.05):
    """The support of a tabletop frame: (centre f64[3], e1, e2 f64[3], half f64[2]) of the rectangle centre +- half[0] e1 +- half[1]
    e2 in the plane up . (p - point) = 0 (camera frame of the render, the camera at the origin ABOVE the plane).  The part of the
    plane inside the view frustum up to the depth `far` is a convex polygon whose corners are the hits of the four corner rays (where
    they reach the plane within `far`) and the crossings of the far rectangle's four sides with the plane; the rectangle is their
    bounding box along e1 = the image's horizontal turned into the plane and e2 = up x e1, each half-side times `margin` plus `pad`
    metres."""
    up, point = np.asarray(up, np.float64), np.asarray(point, np.float64)
    e1 = np.array([1.0, 0.0, 0.0]) - up[0] * up
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(up, e1)
    h = float(up @ point)                                                     # up . p = h on the plane; h < 0: the camera is above it
    tx, ty = width / (2.0 * fx), height / (2.0 * fy)
    corners = [far * np.array([sx * tx, sy * ty, -1.0]) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    pts = []
    for k, c in enumerate(corners):
        s = up @ c
        if s < 0 and h / s <= 1.0:                                            # the corner ray reaches the plane within `far`
            pts.append(c * (h / s))
        a, b = c, corners[(k + 1) % 4]                                        # one side of the far rectangle
        sa, sb = up @ a - h, up @ b - h
        if (sa < 0) != (sb < 0):
            pts.append(a + (b - a) * (sa / (sa - sb)))
    if not pts:
        raise ValueError("the support plane does not cross the view frustum within the far range")
    q = np.asarray(pts) - point
    a, b = q @ e1, q @ e2
    mid = np.array([(a.min() + a.max()) / 2, (b.min() + b.max()) / 2])
    half = np.array([(a.max() - a.min()) / 2, (b.max() - b.min()) / 2]) * margin + pad
    return point + mid[0] * e1 + mid[1] * e2, e1, e2, half


class TabletopFrameSampler(MeshFrameSampler):
    """Frames of `n_objects` meshes STANDING on a table: one support plane under all of them, every object upright on it (its mesh's
    +y along the table's up axis, the bottom face of its box in the plane), objects that may touch (min_gap = 0).  Constructor and
    seeded-generator contract as MeshFrameSampler's; min_gap: the least distance in metres between two footprint circles.

    draw() is host work only.  From ONE np.random.Generator(seed) it draws, in this order:
      1. the camera tilt, once per frame: x = rng.uniform(25, 65) degrees, yy = rng.uniform(-15, 15) degrees (meshes.draw_pose's NOCS
         ranges); Rt = roty(yy) . rotx(x), composed as draw_pose composes them (in the other order yy would only turn the table
         about its own up axis), takes table coordinates into the render's camera frame; up = Rt (0, 1, 0);
      2. the table: d0 = rng.uniform(the far half of z_range); the plane passes through (0, 0, -d0) on the optical axis with the
         normal `up` (the near half would leave no room in the view for an object of a few decimetres);
      3. object by object (j = 0 .. n_objects - 1): the category, the mesh and the scale as MeshFrameSampler draws them; the turn
         about the table's up axis y = rng.uniform(0, 2 pi), R = Rt . roty(y); then the foot (the centre of the box's bottom face),
         up to max_attempts times: the view ray (rng.uniform(-1, 1) W / (2 fx), rng.uniform(-1, 1) H / (2 fy), -1) -- a point drawn
         uniformly over the image -- and foot = where it meets the plane (a ray that does not is a refusal).  When the footprint circle
         (the scale times footprint_radius) lies closer than min_gap to the circle of an object placed before, the foot is moved away
         from the first such object, along the line that joins the two feet, until the circles are min_gap (plus a nanometre)
         apart: this is what makes objects touch at min_gap = 0.  The attempt is kept when every earlier circle is then at least
         min_gap away and the bounding sphere (radius r = the scale times the mesh's bounding radius) about the box centre t = foot +
         up . scale . (box height / 2) lies inside the view frustum to first order, as MeshFrameSampler keeps it: |t.x| <= d_t W / (2 fx)
         - r, |t.y| <= d_t H / (2 fy) - r, d_t = -t.z in z_range.  max_attempts refusals in a row
         raise RuntimeError.
    The table is one more mesh (PLANE_MESH, appended to the mesh set) posed as plane_quad's rectangle with far = z_range[1]: wider
    than the frustum at the far range.  sample() renders it as the LAST instance of the ONE render_instances call, so at equal depth
    the objects win; afterwards its label (n_objects) becomes -1 and its depth stays.  It counts against the rasteriser's instance
    cap: n_objects <= MAX_INSTANCES - 1.  sample() returns a MeshFrame of the n_objects objects (ground truth through
    ground_truth) whose spec also holds `support`: the pixels the table kept (bool[H,W], device).  The same seed gives the same
    frames bit for bit."""

    def __init__(self, category_meshes, n_objects, device=None, seed=0, cfgs=None, z_range=Z_RANGE, max_attempts=100, min_gap=0.0,
                 fx=M.FX, fy=M.FY, width=M.WIDTH, height=M.HEIGHT, znear=M.ZNEAR, synset_names=None):
        if n_objects > MAX_INSTANCES - 1:
            raise ValueError(f"{n_objects} objects and the table: one render takes at most {MAX_INSTANCES} instances")
        if not (np.isfinite(min_gap) and min_gap >= 0):
            raise ValueError(f"min_gap must be finite and >= 0, got {min_gap}")
        super().__init__(category_meshes, n_objects, device, seed, cfgs, z_range, max_attempts, fx, fy, width, height, znear, synset_names)
        self.min_gap = float(min_gap)
        self.footprint = [footprint_radius(v, f, *b) for (v, f), b in zip(self.meshes, self.bounds)]
        self.plane_mesh = len(self.meshes)                      # the table: the last mesh of the set, drawn by the last instance
        self.meshes.append((PLANE_MESH[0].copy(), PLANE_MESH[1].copy()))

    def draw(self):
        """MeshFrameSampler.draw's dict for the n_objects objects (model_views and inst_mesh with the table's entry appended: K + 1
        rows), plus tilt (x, yy), up, table_point, feet f64[K,3], footprints f64[K], quad (plane_quad's tuple)"""
        rng, K = self.rng, self.n_objects
        x, yy = rng.uniform(25 / 180 * np.pi, 65 / 180 * np.pi), rng.uniform(-15 / 180 * np.pi, 15 / 180 * np.pi)
        Rt = M.roty(yy)[:3, :3] @ M.rotx(x)[:3, :3]
        up = Rt[:, 1].copy()
        d0 = rng.uniform((self.z_range[0] + self.z_range[1]) / 2, self.z_range[1])
        o = np.array([0.0, 0.0, -d0])
        cats, inst, scales, Rs, ts, radii, models, gts, feet, foots = [], [], [], [], [], [], [], [], [], []
        for _ in range(K):
            cat = self.categories[int(rng.integers(len(self.categories)))]
            m = self.index[(cat, int(rng.integers(self.n_meshes[cat])))]
            scale = rng.uniform(self.cfgs[cat].scale_range[0], self.cfgs[cat].scale_range[1])
            R = Rt @ M.roty(rng.uniform(0, 2 * np.pi))[:3, :3]
            bmin, bmax = self.bounds[m]
            r, rho, rise = scale * self.radius[m], scale * self.footprint[m], scale * (bmax[1] - bmin[1]) / 2
            for _ in range(self.max_attempts):
                ray = np.array([rng.uniform(-1.0, 1.0) * self.width / (2 * self.fx), rng.uniform(-1.0, 1.0) * self.height / (2 * self.fy), -1.0])
                if not up @ ray < 0:                                          # this ray never reaches the table
                    continue
                foot = ray * ((up @ o) / (up @ ray))
                need = [rho + rho2 + self.min_gap for rho2 in foots]
                near = [j for j, f2 in enumerate(feet) if np.linalg.norm(foot - f2) < need[j]]
                if near:
                    j, gap = near[0], np.linalg.norm(foot - feet[near[0]])
                    if gap == 0.0:
                        continue
                    foot = feet[j] + (foot - feet[j]) * ((need[j] + 1e-9) / gap)
                t = foot + up * rise
                dt = -t[2]
                if (all(np.linalg.norm(foot - f2) >= n2 for f2, n2 in zip(feet, need)) and self.z_range[0] <= dt <= self.z_range[1]
                        and abs(t[0]) <= dt * self.width / (2 * self.fx) - r and abs(t[1]) <= dt * self.height / (2 * self.fy) - r):
                    break
            else:
                raise RuntimeError(f"{self.max_attempts} placements in a row left the view or came too close to an object placed before")
            cats.append(cat); inst.append(m); scales.append(scale); Rs.append(R); ts.append(t); radii.append(r); feet.append(foot); foots.append(rho)
            models.append(M.model_matrix(R, t, scale, bmin, bmax))
            gts.append(ground_truth(R, t, scale, bmin, bmax, cat in NOCS_CATEGORIES))
        quad = plane_quad(up, o, self.fx, self.fy, self.width, self.height, self.z_range[1])
        centre, e1, e2, half = quad
        plane = np.eye(4)
        # PLANE_MESH's x, y, z axes become e1, up and e1 x up = -e2 (right-handed: the winding survives), x and z scaled to the rectangle
        plane[:3, 0], plane[:3, 1], plane[:3, 2], plane[:3, 3] = half[0] * e1, up, half[1] * np.cross(e1, up), centre
        return dict(categories=cats, inst_mesh=np.asarray(inst + [self.plane_mesh], np.int32), scales=np.asarray(scales), Rs=np.asarray(Rs),
                    ts=np.asarray(ts), radii=np.asarray(radii), model_views=np.asarray(models + [plane]),
                    centers=np.asarray([g[0] for g in gts]), gt_Rs=np.asarray([g[1] for g in gts]),
                    half_extents=np.asarray([g[2] for g in gts]), tilt=(x, yy), up=up, table_point=o, feet=np.asarray(feet),
                    footprints=np.asarray(foots), quad=quad)

    def sample(self, cull=True):
        M.require_cuda()
        dev = self.dev or torch.device("cuda", 0)
        if self._set is None:
            self._set = M.mesh_set(self.meshes, dev)
        spec = self.draw()
        depth, labels = M.render_instances(self._set, spec["inst_mesh"], spec["model_views"], cull=cull, fx=self.fx, fy=self.fy,
                                           width=self.width, height=self.height, znear=self.znear, device=dev)
        spec["support"] = labels == self.n_objects
        return self.frame(spec, depth, torch.where(spec["support"], torch.full_like(labels, -1), labels))
