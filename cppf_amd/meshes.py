"""Training views from meshes: the sample of utils/dataset.py:103-250 (`ShapeNetDataset.get_item_impl`) on the device.

A mesh (an OBJ file, `load_obj`) is centred, scaled and posed at random in front of the dataset's pinhole camera, rendered to a
640x480 depth image by the HIP rasteriser (csrc/raster.hip, `render_depth`; pyrender's role), and the covered pixels become the
dataset's point cloud (cppf_depth_points).  The cloud is moved back to the object frame, jittered, voxel-deduplicated, given PCA
normals and pairs, and the vote targets are computed (`MeshViewSampler.sample`).  Everything after the host draws runs on the
device; a sample reads two counts back (the rendered points, the points after deduplication), the reference reads the same
sizes on its host.

`render_instances` renders several posed meshes into one depth image with an instance label per pixel (cppf_raster_instances);
cppf_amd/mesh_frames.py builds frames with ground truth on it."""
import os

import numpy as np
import torch

from . import _lib
from ._torch_util import call, canon, require_cuda, scratch, workspace
from .config import CATEGORIES, NOCS_CATEGORIES

DATASET_K = np.array([[591.0125, 0, 320], [0, 590.16775, 240], [0, 0, 1]])   # utils/dataset.py:96 (not the inference intrinsics)
FX, FY, WIDTH, HEIGHT, ZNEAR = 591.0125, 590.16775, 640, 480, 0.05           # :137 PinholeCamera, pyrender's default znear
FLIP2NOCS = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float64)         # :210


def roty(a):
    """utils/util.py:88-92, its sign convention included"""
    return np.array([[np.cos(a), 0, -np.sin(a), 0], [0, 1, 0, 0], [np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])


def rotx(a):
    """utils/util.py:94-98"""
    return np.array([[1, 0, 0, 0], [0, np.cos(a), -np.sin(a), 0], [0, np.sin(a), np.cos(a), 0], [0, 0, 0, 1]])


# ----------------------------------------------------------------------------------------------------------------- OBJ files
def parse_obj(text):
    """OBJ text -> (vertices f64[V,3], faces i32[F,3], bmin f64[3], bmax f64[3]).  Reads `v` and `f` records; `f` corners may
    be `a`, `a/b`, `a//c` or `a/b/c`, indices 1-based or negative (relative to the vertices read so far); polygons are
    fan-triangulated (a b c d -> a b c, a c d).  Every other record (vt, vn, g, o, usemtl, mtllib, s, ...) and comments are
    ignored.  The bounds are taken over the vertices some face references: they stand in for trimesh's bounds of the loaded
    scene (utils/dataset.py:161), which leave unreferenced vertices out."""
    verts, faces = [], []
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        parts = line.split()
        tag = parts[0]
        if tag == "v":
            if len(parts) < 4:
                raise ValueError(f"OBJ line {ln}: a vertex needs three coordinates")
            verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
        elif tag == "f":
            nv = len(verts)
            corner = []
            for c in parts[1:]:
                k = int(c.split("/", 1)[0])
                i = k - 1 if k > 0 else nv + k
                if k == 0 or not 0 <= i < nv:
                    raise ValueError(f"OBJ line {ln}: vertex index {k} outside the {nv} vertices read so far")
                corner.append(i)
            if len(corner) < 3:
                raise ValueError(f"OBJ line {ln}: a face needs three vertices")
            for j in range(1, len(corner) - 1):
                faces.append((corner[0], corner[j], corner[j + 1]))
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    if f.shape[0] == 0:
        raise ValueError("OBJ holds no faces")
    used = v[np.unique(f)]
    return v, f, used.min(0), used.max(0)


def load_obj(path):
    """(vertices f64[V,3], faces i32[F,3]) of an OBJ file; parse_obj has the rules (bounds: mesh_bounds)"""
    v, f, _, _ = parse_obj(open(path).read())
    return v, f


def mesh_bounds(vertices, faces):
    """(bmin, bmax) over the vertices that some face references"""
    used = np.asarray(vertices, np.float64)[np.unique(np.asarray(faces))]
    return used.min(0), used.max(0)


# ----------------------------------------------------------------------------------------------------------------- rendering
class _Mesh:
    """a mesh on the device: vertices f64, faces i32, the host bounds and the bin-list capacity its renders need"""

    def __init__(self, vertices, faces, dev):
        self.v = torch.as_tensor(np.ascontiguousarray(vertices, np.float64)).to(dev)
        self.f = torch.as_tensor(np.ascontiguousarray(faces, np.int32)).to(dev)
        self.bmin, self.bmax = mesh_bounds(vertices, faces)
        self.n_faces = int(self.f.shape[0])
        self.bins = default_bin_entries(self.n_faces)


def default_bin_entries(n_faces, W=WIDTH, H=HEIGHT):
    """the starting capacity of the bin list: 4 (primitive, tile) entries per face plus 64 per tile; it grows to what a render
    reports it needed"""
    return int(min(4 * n_faces + 64 * ((W + 15) // 16) * ((H + 15) // 16), 0x7FFFFFFF))


def _raster(mesh, model_view, out, cull, fx, fy, znear, sync, ok=()):
    H, W = out.shape
    nbytes = _lib.lib().cppf_raster_workspace_bytes(mesh.n_faces, W, H, mesh.bins)
    if nbytes == 0:
        raise ValueError(f"render of {mesh.n_faces} faces at {W}x{H}: outside the rasteriser's limits (include/cppf.h)")
    ws = workspace(nbytes, out.device, "raster")
    mv = np.ascontiguousarray(np.asarray(model_view, np.float64)[:3, :4])
    rc = call("cppf_raster_depth", out.device, mesh.v, mesh.v.shape[0], mesh.f, mesh.n_faces, mv, fx, fy, W, H, znear, bool(cull), out,
              mesh.bins, bool(sync), scratch(ws), ok=ok)
    return rc, ws


def _render(mesh, model_view, out, cull=True, fx=FX, fy=FY, znear=ZNEAR, sync=True):
    """render into `out`; a bin list that was too small is grown to what the render needed and the render repeated once"""
    rc, ws = _raster(mesh, model_view, out, cull, fx, fy, znear, sync, ok=(_lib.ECAPACITY,))
    if rc == _lib.ECAPACITY:                                         # the status words hold the entries needed
        mesh.bins = int(min(int(ws[:8].view(torch.int32)[1].item()) * 5 // 4 + 1024, 0x7FFFFFFF))   # (headroom for the next pose)
        _, ws = _raster(mesh, model_view, out, cull, fx, fy, znear, True)
    return ws


def render_depth(vertices, faces, pose, cull=True, fx=FX, fy=FY, width=WIDTH, height=HEIGHT, znear=ZNEAR, device=None,
                 max_bin_entries=None):
    """Depth image f32[height, width] (device) of a mesh under the model-view matrix `pose` (4x4; the camera looks down -z):
    pyrender's DEPTH_ONLY render through the dataset's PinholeCamera, background 0 (include/cppf.h: cppf_raster_depth).
    vertices f64[V,3] / faces i32[F,3], numpy or device tensors.  cull=False renders both sides.  max_bin_entries: a fixed
    bin-list capacity (a render that needs more raises CppfError); None sizes it by itself."""
    require_cuda()
    dev = device or (vertices.device if isinstance(vertices, torch.Tensor) and vertices.is_cuda else torch.device("cuda", 0))
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else vertices
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else faces
    mesh = _Mesh(v, f, dev)
    out = torch.empty((height, width), dtype=torch.float32, device=dev)
    if max_bin_entries is not None:
        mesh.bins = int(max_bin_entries)
        _raster(mesh, pose, out, cull, fx, fy, znear, True)
    else:
        _render(mesh, pose, out, cull, fx, fy, znear)
    return out


class _MeshSet:
    """several meshes on the device in the form cppf_raster_instances reads: vertices and faces concatenated (face indices local
    to their mesh), the host offset tables, and the bin-list capacity the renders of the set have needed so far"""

    def __init__(self, meshes, dev):
        vs, fs = [], []
        for k, m in enumerate(meshes):
            v, f = (m.v, m.f) if isinstance(m, _Mesh) else m
            if isinstance(v, torch.Tensor):                          # (device tensors included: the caller's own form)
                vs.append(canon(v, torch.float64, v.device, f"meshes[{k}] vertices", tail=(3,)).to(dev))
                fs.append(canon(f, torch.int32, f.device, f"meshes[{k}] faces", tail=(3,)).to(dev))
            else:
                vs.append(torch.as_tensor(np.ascontiguousarray(v, np.float64).reshape(-1, 3)).to(dev))
                fs.append(torch.as_tensor(np.ascontiguousarray(f, np.int32).reshape(-1, 3)).to(dev))
        if not vs:
            raise ValueError("no meshes")
        self.n = len(vs)
        self.vert_off = np.concatenate([[0], np.cumsum([v.shape[0] for v in vs])]).astype(np.int64)
        self.face_off = np.concatenate([[0], np.cumsum([f.shape[0] for f in fs])]).astype(np.int64)
        self.v = torch.cat(vs).contiguous()
        self.f = torch.cat(fs).contiguous()
        self.bins = {}                                               # (W, H) -> capacity


def _instanced_faces(ms, inst_mesh):
    """the faces all instances draw together (an entry that names no mesh of the set counts nothing: the call refuses it)"""
    known = (inst_mesh >= 0) & (inst_mesh < ms.n)
    return int((ms.face_off[1:] - ms.face_off[:-1])[inst_mesh[known]].sum())


def _raster_instances(ms, inst_mesh, mvs, depth, labels, bins, cull, fx, fy, znear, ok=()):
    H, W = depth.shape
    K, Q = int(inst_mesh.shape[0]), _instanced_faces(ms, inst_mesh)
    nbytes = _lib.lib().cppf_raster_instances_workspace_bytes(K, max(Q, 1), ms.n, W, H, bins)
    if nbytes == 0:
        raise ValueError(f"render of {K} instances with {Q} faces at {W}x{H}: outside the rasteriser's limits (include/cppf.h)")
    ws = workspace(nbytes, depth.device, "raster_instances")
    rc = call("cppf_raster_instances", depth.device, ms.v, ms.f, ms.vert_off, ms.face_off, ms.n, inst_mesh, mvs, K, fx, fy, W, H, znear,
              bool(cull), depth, labels, bins, True, scratch(ws), ok=ok)
    return rc, ws


def render_instances(meshes, inst_mesh, model_views, cull=True, fx=FX, fy=FY, width=WIDTH, height=HEIGHT, znear=ZNEAR, device=None,
                     max_bin_entries=None, out=None):
    """Several posed meshes in ONE depth image with the instance that owns each pixel (include/cppf.h: cppf_raster_instances;
    one binned pass over all instances' triangles): (depth f32[height, width], labels i32[height, width]) device tensors.
    meshes: a list of (vertices f64[V,3], faces i32[F,3]) pairs (numpy or tensors) or a set loaded before (`mesh_set`);
    inst_mesh i32[K]: the mesh each instance draws; model_views f64[K,4,4] (or [K,3,4]): each instance's model-view matrix, as
    render_depth takes its one.  A pixel keeps the nearest fragment of all instances and the index of the instance it came from
    (equal depth: the lowest index); background: depth 0, label -1.  max_bin_entries: a fixed bin-list capacity (a render that
    needs more raises CppfError); None sizes it by itself and repeats a render that needed more once.  out: (depth, labels)
    tensors to render into."""
    require_cuda()
    dev = device or torch.device("cuda", 0)
    ms = meshes if isinstance(meshes, _MeshSet) else _MeshSet(meshes, dev)
    inst = np.ascontiguousarray(np.asarray(inst_mesh).reshape(-1), np.int32)
    mvs = np.asarray(model_views, np.float64)
    if mvs.ndim != 3 or mvs.shape[0] != inst.shape[0] or mvs.shape[1] not in (3, 4) or mvs.shape[2] != 4:
        raise ValueError(f"model_views must be [K,4,4] or [K,3,4] with one matrix per instance, got {mvs.shape} for {inst.shape[0]}")
    mvs = np.ascontiguousarray(mvs[:, :3, :])
    if out is None:
        depth = torch.empty((height, width), dtype=torch.float32, device=dev)
        labels = torch.empty((height, width), dtype=torch.int32, device=dev)
    else:
        depth = canon(out[0], torch.float32, dev, "out depth", tail=(height, width))
        labels = canon(out[1], torch.int32, dev, "out labels", tail=(height, width))
        if depth is not out[0] or labels is not out[1]:
            raise ValueError("out: contiguous f32 / i32 [height, width] tensors on the device")
    if max_bin_entries is not None:
        _raster_instances(ms, inst, mvs, depth, labels, int(max_bin_entries), cull, fx, fy, znear)
        return depth, labels
    bins = max(ms.bins.get((width, height), 0), default_bin_entries(_instanced_faces(ms, inst), width, height))
    rc, ws = _raster_instances(ms, inst, mvs, depth, labels, bins, cull, fx, fy, znear, ok=(_lib.ECAPACITY,))
    if rc == _lib.ECAPACITY:                                         # the status words hold the entries needed
        bins = int(min(int(ws[:8].view(torch.int32)[1].item()) * 5 // 4 + 1024, 0x7FFFFFFF))
        _raster_instances(ms, inst, mvs, depth, labels, bins, cull, fx, fy, znear)
    ms.bins[(width, height)] = bins
    return depth, labels


def mesh_set(meshes, device=None):
    """meshes ((vertices, faces) pairs) uploaded once for many render_instances calls"""
    require_cuda()
    return _MeshSet(meshes, device or torch.device("cuda", 0))


def depth_points(depth, intrinsics=DATASET_K):
    """The covered pixels of a rendered depth image as the dataset's cloud (utils/dataset.py:203-207): (pts f64[H*W,3], count
    i32[1]) device tensors, the first count rows valid, in row-major pixel order (include/cppf.h: cppf_depth_points)."""
    depth = canon(depth, torch.float32, depth.device, "depth")      # (a strided view or another float type: a converted copy)
    if depth.dim() != 2:
        raise ValueError(f"depth must be [H,W], got {tuple(depth.shape)}")
    H, W = depth.shape
    pts = torch.empty((H * W, 3), dtype=torch.float64, device=depth.device)
    pix = torch.empty(H * W, dtype=torch.int32, device=depth.device)
    count = torch.zeros(1, dtype=torch.int32, device=depth.device)
    ws = workspace(_lib.lib().cppf_depth_points_workspace_bytes(H, W), depth.device, "depth_points")
    kinv = np.ascontiguousarray(np.linalg.inv(np.asarray(intrinsics, np.float64)))
    call("cppf_depth_points", depth.device, depth, H, W, kinv, pts, pix, count, scratch(ws))
    return pts, count


# ----------------------------------------------------------------------------------------------------------------- samples
def draw_pose(rng, is_nocs):
    """utils/dataset.py:143-159: (R f64[3,3], t f64[3]) of the mesh, drawn from the numpy Generator `rng` in the reference's order"""
    if is_nocs:
        y = rng.uniform(0, 2 * np.pi)
        x = rng.uniform(25 / 180 * np.pi, 65 / 180 * np.pi)
        yy = rng.uniform(-15 / 180 * np.pi, 15 / 180 * np.pi)
        R = roty(yy)[:3, :3] @ rotx(x)[:3, :3] @ roty(y)[:3, :3]
        t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -rng.uniform(0.6, 2.0)])
    else:
        y = rng.uniform(0, 2 * np.pi)
        x = np.clip(rng.normal(40, 10), 10, 70) / 180 * np.pi
        R = rotx(x)[:3, :3] @ roty(y)[:3, :3]
        t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), -rng.uniform(1.0, 5.0)])
    return R, t


def apply_rotation(pc, A):
    """rows of pc (f64 device [N,3]) times the host matrix A (f64 3x3): out_r = (A[r,0] x + A[r,1] y) + A[r,2] z, in that order
    (a fixed sequence of fp64 operations, so tests/mesh_ref.py restates it bit for bit)"""
    A = np.asarray(A, np.float64)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    return torch.stack([(float(A[r, 0]) * x + float(A[r, 1]) * y) + float(A[r, 2]) * z for r in range(3)], -1)


def model_matrix(R, t, scale, bmin, bmax):
    """:162-170: pose . scale . translate(-(bmin + bmax) / 2)"""
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, t
    trans = np.eye(4)
    trans[:3, 3] = -(np.asarray(bmax) + np.asarray(bmin)) / 2
    sc = np.eye(4)
    sc[:3, :3] *= scale
    return pose @ sc @ trans


def view_half_extents(bmin, bmax, scale):
    """:244-248: (bmax - bmin) / 2 * scale with x and z swapped -- unconditionally, as the reference does"""
    b = np.asarray(bmax, np.float64) - np.asarray(bmin, np.float64)
    b[[0, 2]] = b[[2, 0]]
    return b / 2 * scale


class MeshViewSampler:
    """ShapeNetDataset.get_item_impl (utils/dataset.py:103-250) over a list of mesh files, on the device.

    sample() draws a mesh, a scale and a pose on the host (np.random.Generator seeded with `seed`), renders and back-projects on
    the device, and returns the tensors train.py's loop reads, under the reference's names: pc f32[N,3], normals f32[N,3],
    point_idxs i64[n_pairs,2], targets_tr / targets_rot / targets_rot_aux / targets_scale (cppf_amd.training.targets), plus the
    draws (mesh, path, R, t, scale, model, jitter_state = the torch generator's state the jitter was drawn from) and the views
    drawn and refused on the way (skipped).  Jitter and
    pairs come from a seeded torch generator on the device: the same seed gives the same samples bit for bit.
    canonical=False stops before the move to the object frame and returns a held-out object in the camera frame in the form
    training.infer / training.pose_errors read (pc / normals numpy f32, center, R (columns: the object's axes), half_extents, cfg)."""

    def __init__(self, mesh_paths, category, device=None, seed=0, n_pairs=200000, max_attempts=100, cfg=None, meshes=None):
        require_cuda()
        self.paths = list(mesh_paths) if meshes is None else [f"<mesh {k}>" for k in range(len(meshes))]
        if not self.paths:
            raise ValueError("no meshes")
        self.cfg = cfg or CATEGORIES[category]
        if self.cfg.scale_range is None:
            raise ValueError(f"category {category}: no scale_range in its config")
        self.category = category
        self.is_nocs = category in NOCS_CATEGORIES
        self.dev = device or torch.device("cuda", 0)
        self.rng = np.random.default_rng(seed)
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(seed)
        self.n_pairs = n_pairs
        self.max_attempts = max_attempts
        self._meshes = {}
        for k, (v, f) in enumerate(meshes or []):                  # meshes: (vertices, faces) pairs given in place of files
            self._meshes[k] = _Mesh(v, f, self.dev)
        self._depth = torch.empty((HEIGHT, WIDTH), dtype=torch.float32, device=self.dev)

    def mesh(self, i):
        m = self._meshes.get(i)
        if m is None:
            m = self._meshes[i] = _Mesh(*load_obj(self.paths[i]), self.dev)
        return m

    def sample(self, canonical=True, mesh_index=None):
        from .training import targets
        from .utils.util import estimate_normals, sparse_quantize
        cfg, skipped = self.cfg, []
        i = int(self.rng.integers(len(self.paths))) if mesh_index is None else int(mesh_index)
        for _ in range(self.max_attempts):
            m = self.mesh(i)
            R, t = draw_pose(self.rng, self.is_nocs)
            scale = self.rng.uniform(cfg.scale_range[0], cfg.scale_range[1])
            model = model_matrix(R, t, scale, m.bmin, m.bmax)
            ws = _render(m, model, self._depth, sync=False)
            pts, count = depth_points(self._depth)
            n_px, code, _ = torch.cat([count, ws[:8].view(torch.int32)]).tolist()       # one host read: count + render status
            if code == _lib.ECAPACITY:                                                                  # the bin list grew: render again
                ws = _render(m, model, self._depth)
                pts, count = depth_points(self._depth)
                n_px = int(count.item())
            else:
                _lib.check(code, "cppf_raster_depth")
            pc = pts[:n_px]
            if canonical:
                pc = pc - torch.as_tensor(t, device=self.dev)                               # :208
                pc = apply_rotation(pc, np.linalg.inv(R))                                   # :209
                if self.is_nocs:
                    pc = apply_rotation(pc, FLIP2NOCS)                                      # :210-212
            gen_state = self.gen.get_state()                                                # (what the jitter was drawn from)
            if n_px > 0:
                jit = torch.randn(pc.shape, generator=self.gen, device=self.dev, dtype=torch.float64)
                pc = pc + torch.clamp(cfg.res / 4 * jit, -cfg.res / 2, cfg.res / 2)        # :215
                _, keep = sparse_quantize(pc.float(), return_index=True, quantization_size=cfg.res)   # :217-218
                pc = pc[keep]
            n = int(pc.shape[0])
            if 100 <= n <= cfg.npoint_max:                                                  # :221-222
                break
            skipped.append(dict(mesh=i, n_points=n))
            i = int(self.rng.integers(len(self.paths)))
        else:
            raise RuntimeError(f"{self.max_attempts} views in a row had fewer than 100 or more than {cfg.npoint_max} points")
        pc = pc.float().contiguous()
        normals = estimate_normals(pc, cfg.knn)                                             # :224-227
        half = view_half_extents(m.bmin, m.bmax, scale)
        out = dict(mesh=i, path=self.paths[i], R=R, t=t, scale=scale, model=model, skipped=skipped, cfg=cfg, category=self.category,
                   half_extents=half, jitter_state=gen_state)
        if not canonical:
            Robj = R @ FLIP2NOCS.T if self.is_nocs else R
            out.update(pc=pc.cpu().numpy(), normals=normals.cpu().numpy(), center=np.asarray(t, np.float64), R=Robj, R_mesh=R)
            return out
        idx = torch.randint(0, n, (self.n_pairs, 2), device=self.dev, generator=self.gen)   # :25 (generate_target's draw)
        tr, rot, aux, sc = targets(pc, normals, idx, np.zeros(3), np.eye(3), half, cfg)     # :229-248
        out.update(pc=pc, normals=normals, point_idxs=idx, targets_tr=tr, targets_rot=rot, targets_rot_aux=aux, targets_scale=sc)
        return out


def mesh_paths(spec, shapenet_root=None):
    """`spec` = a directory: every *.obj under it, recursively (a ShapeNet synset directory gives its
    <model>/models/model_normalized.obj files); or a names file in the format of data/shapenet_names/*.txt (one
    `<synset>/<model>` per line), resolved against `shapenet_root` (default: the file's directory) as train.py:22-29 and
    utils/dataset.py:160 do.  Returns the sorted list of paths."""
    if os.path.isdir(spec):
        out = []
        for d, _, files in os.walk(spec):
            out += [os.path.join(d, f) for f in files if f.lower().endswith(".obj")]
        return sorted(out)
    root = shapenet_root or os.path.dirname(os.path.abspath(spec))
    names = [ln.strip() for ln in open(spec) if ln.strip()]
    return sorted(os.path.join(root, n, "models", "model_normalized.obj") for n in names)
