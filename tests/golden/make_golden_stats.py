#!/usr/bin/env python3
"""Voting statistics and right_sym targets from the reference itself (run in the build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stats.py <reference checkout>

  * utils/dataset.py:generate_target and utils/util.py:real2prob are executed from their own source (FunctionDef extracted with
    `ast`, exec'd with the real numpy / torch), with right_sym False and True, on fixed points;
  * gen_stats.py's `if __name__ == '__main__':` body is executed from its own source too, with stand-ins for what is not installed:
    Open3D's read_triangle_mesh / sample_points_uniformly return fixed point sets (one per mesh directory), estimate_normals
    returns zeros (gen_stats.py discards target_rot_aux, the only consumer of the normals), tqdm is the identity, and the
    category's meshes are empty directories of a temporary ShapeNet-style root.  generate_target is the real one, drawing its
    pairs from np.random seeded below; what the body printed and its scale_range / vote_range / scale_mean are recorded;
  * the reference's 12 config/category/*.yaml and config/config.yaml (settings only) are copied to tests/golden/config/.
Only data is written (stats.npz and the YAML copies)."""
import argparse
import ast
import contextlib
import hashlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

ref = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
if ref is None:
    raise SystemExit("usage: make_golden_stats.py <reference checkout> [--trust-modified-reference]")
out_dir = os.path.dirname(os.path.abspath(__file__))

# Trust: code below is exec'd from the reference checkout with this user's privileges.  The checkout is untrusted content, so the
# files are pinned by hash -- the versions that were read -- and a modified checkout is refused (--trust-modified-reference
# overrides, for a reviewed upgrade of the reference).
PINNED = {"utils/dataset.py": "5abbd20c0b137c9c5bf35997cda5eb210ab6e8017baba2537bb96d400c7035a6",
          "utils/util.py": "d6b3854a81d35c3eb0139899f0e2a687095ba37e3294bcb084ec8f4e8d4dddf0",
          "gen_stats.py": "567ef1e11b359bcbda6be0780be834409bf623c4d7791421403450cf75b275d7"}


def source(rel):
    path = os.path.join(ref, rel)
    text = open(path, "rb").read()
    digest = hashlib.sha256(text).hexdigest()
    if digest != PINNED[rel] and "--trust-modified-reference" not in sys.argv:
        raise SystemExit(f"{rel}: sha256 {digest} is not the pinned version; refusing to exec code from it")
    return path, ast.parse(text.decode())


def extract(rel, name, env):
    path, tree = source(rel)
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), env)
            return env[name]
    raise KeyError(name)


def main_body(rel):
    """the statements of `if __name__ == '__main__':`"""
    path, tree = source(rel)
    for node in tree.body:
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and getattr(node.test.left, "id", "") == "__name__":
            return path, ast.Module(body=node.body, type_ignores=[])
    raise KeyError("__main__ block")


gt = extract("utils/dataset.py", "generate_target", {"np": np})
real2prob = extract("utils/util.py", "real2prob", {"np": np, "torch": torch})
out = {}

# ---- generate_target with right_sym False / True (float32-representable fp64 points, as gen_stats.py passes fp64)
NP = 400
rng = np.random.default_rng(21)
n = 300
th = rng.uniform(0, 2 * np.pi, n)
pc = np.stack([rng.uniform(-0.12, 0.12, n), 0.04 * np.cos(th), 0.04 * np.sin(th)], -1) + rng.normal(0, 1e-3, (n, 3))
nrm = rng.normal(0, 1, (n, 3))
nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
pc = pc.astype(np.float32).astype(np.float64)
nrm = nrm.astype(np.float32).astype(np.float64)
out.update(pc=pc, nrm=nrm)
tr_bins, rot_bins, vote_range = 32, 36, [0.25, 0.25]
for tag, (up_sym, right_sym, z_right) in (("plain", (False, False, False)), ("rightsym", (False, True, False)),
                                          ("rightsym_zright_upsym", (True, True, True))):
    np.random.seed(11)
    tr, rot, aux, pidx = gt(pc, nrm.copy(), up_sym=up_sym, right_sym=right_sym, z_right=z_right, subsample=NP)
    tr_soft = np.stack([real2prob(np.clip(tr[:, 0] + vote_range[0], 0, 2 * vote_range[0]), 2 * vote_range[0], tr_bins, circular=False),
                        real2prob(np.clip(tr[:, 1], 0, vote_range[1]), vote_range[1], tr_bins, circular=False)], 1)   # :232-237
    rot_soft = np.stack([real2prob(rot[:, 0], np.pi, rot_bins, circular=False),
                         real2prob(rot[:, 1], np.pi, rot_bins, circular=False)], 1)                                   # :239-243
    out.update({f"{tag}.point_idxs": pidx, f"{tag}.targets_tr": tr, f"{tag}.targets_rot": rot, f"{tag}.aux": aux,
                f"{tag}.tr_soft": tr_soft.astype(np.float32), f"{tag}.rot_soft": rot_soft.astype(np.float32),
                f"{tag}.flags": np.array([up_sym, right_sym, z_right])})

# ---- gen_stats.py's body on fixed point sets
SEED = 5
shapes = []
rng = np.random.default_rng(3)
for k, (hx, hy, hz) in enumerate([(0.05, 0.15, 0.05), (0.08, 0.11, 0.06), (0.04, 0.2, 0.045)]):
    m = 256 + 32 * k
    p = rng.uniform(-1, 1, (m, 3)) * np.array([hx, hy, hz]) + rng.uniform(-0.02, 0.02, 3)
    shapes.append(p)
root = tempfile.mkdtemp()
try:
    synset = "01234567"
    names = [f"mesh{k}" for k in range(len(shapes))]
    for nm in names:
        os.makedirs(os.path.join(root, synset, nm, "models"))
    by_path = {os.path.join(root, f"{synset}/{nm}/models/model_normalized.obj"): p for nm, p in zip(names, shapes)}

    class _Mesh:
        def __init__(self, path):
            self.path = path

        def sample_points_uniformly(self, number_of_points):
            assert number_of_points == 2048
            return types.SimpleNamespace(points=by_path[self.path].copy())

    o3d = types.SimpleNamespace(io=types.SimpleNamespace(read_triangle_mesh=_Mesh))
    listdir_real = os.listdir
    env = {"argparse": argparse, "generate_target": gt, "typename2shapenetid": {"mycat": synset}, "os": os, "o3d": o3d, "np": np,
           "tqdm": lambda x: x, "estimate_normals": lambda pc, k: np.zeros_like(pc)}
    path, body = main_body("gen_stats.py")
    argv = sys.argv
    sys.argv = ["gen_stats.py", "--category", "mycat", "--shapenet_root", root]
    cwd = os.getcwd()
    os.chdir(root)                                   # data/shapenet_names/mycat.txt does not exist there: the listdir branch
    buf = io.StringIO()
    try:
        os.listdir = lambda d: sorted(listdir_real(d))      # a fixed mesh order
        np.random.seed(SEED)
        with contextlib.redirect_stdout(buf):
            exec(compile(body, path, "exec"), env)
    finally:
        os.listdir = listdir_real
        os.chdir(cwd)
        sys.argv = argv
finally:
    shutil.rmtree(root)
for k, p in enumerate(shapes):
    out[f"gen.points{k}"] = p
out["gen.n_meshes"] = np.int64(len(shapes))
out["gen.seed"] = np.int64(SEED)
out["gen.n_pairs"] = np.int64(100000)
out["gen.scale_range"] = np.array(env["scale_range"], np.float64)
out["gen.vote_range"] = np.array(env["vote_range"], np.float32)
out["gen.scale_mean"] = np.asarray(env["scale_mean"], np.float64)
out["gen.printed"] = np.array(buf.getvalue())
# the first pairs each mesh's generate_target drew (np.random.seed(SEED), then one randint per mesh): the test regenerates all of
# them from the legacy RandomState stream and checks them against these
np.random.seed(SEED)
for k, p in enumerate(shapes):
    out[f"gen.first_pairs{k}"] = np.random.randint(0, p.shape[0], size=[100000, 2])[:64]
out["reference_sha256"] = np.array([f"{k}:{v}" for k, v in sorted(PINNED.items())])
np.savez_compressed(os.path.join(out_dir, "stats.npz"), **out)

# ---- the reference's category files (settings only)
cdir = os.path.join(out_dir, "config")
os.makedirs(os.path.join(cdir, "category"), exist_ok=True)
shutil.copyfile(os.path.join(ref, "config", "config.yaml"), os.path.join(cdir, "config.yaml"))
for f in sorted(os.listdir(os.path.join(ref, "config", "category"))):
    if f.endswith(".yaml"):
        shutil.copyfile(os.path.join(ref, "config", "category", f), os.path.join(cdir, "category", f))
print("stats.npz and config/ written;", buf.getvalue().strip().replace("\n", " | "))
