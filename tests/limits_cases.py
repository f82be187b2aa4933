"""Seeded case builders and known answers for the kernels run at their caps and on the second trip of their grid-stride loops
(tests/test_gpu_limits.py); the conditions the cases must meet are asserted without a device in tests/test_limits_cpu.py.

Every expected value here is a closed form, an fp64 / numpy reference, or a documented invariance -- never the output of the
kernel under test.  The limits quoted from the device code:

  csrc/raster.hip     rs_inst_scan_kernel: one workgroup of 1024 lanes, ceil(K / 1024) instances per lane; RS_MAX_INST = 65 536
  csrc/box_nms.hip    NMS_CAP = CPPF_BOX_NMS_GROUP_CAP = 1024 boxes per group: 16 words per bit-matrix row
  csrc/pose_eval.hip  PE_MAX_BLOCKS = 8192 workgroups of 64 lanes; a swept pair is PE_SYM = 20 work items
  csrc/scene.hip      SCN_MAX_RADIUS = 32, SCN_MAX_MARGIN = 64, SCN_TILE = 8; pair kernels: 16 384 workgroups of 256 lanes"""
import functools

import numpy as np

import mesh_frames_ref as FR
import mesh_ref as R
import zero_shot_ref as Z
from cppf_amd import meshes as M

SCAN_LANES = 1024                       # rs_inst_scan_kernel's workgroup
RS_MAX_INST = 65536
NMS_GROUP_CAP = 1024                    # include/cppf.h CPPF_BOX_NMS_GROUP_CAP
PE_LANES_TOTAL = 8192 * 64              # pe_pairs_kernel: PE_MAX_BLOCKS workgroups of PE_LANES lanes
PE_SYM = 20
SCN_MAX_RADIUS, SCN_MAX_MARGIN, SCN_TILE = 32, 64, 8
SCENE_LANES_TOTAL = 16384 * 256         # scene.hip grid_blocks(): the pair kernels' grid

INT32_MAX, INT64_MAX = 2 ** 31 - 1, 2 ** 63 - 1


# ------------------------------------------------------------------------------------------------ 1. instances
INST_W, INST_H, INST_CELL = 320, 240, 4
INST_FX, INST_FY = M.FX / 2, M.FY / 2
INST_COLS, INST_ROWS = INST_W // INST_CELL, INST_H // INST_CELL          # an 80 x 60 grid of 4 x 4-pixel cells
INST_KS = (1024, 1025, 2049, 3100)      # ceil(K / 1024) = 1, 2, 3, 4 instances per lane; the last lanes hold fewer
INST_K_MAX = max(INST_KS)


def instance_meshes():
    """a 2-face quad, the 12-face box and a 7-face partial box (its last seven faces: the +z front among them), all of half
    width 1 in x and y: the model matrix scales them"""
    quad = (np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    v, f, _ = R.box(1.0, 1.0, 0.02)
    return [quad, (v, f), (v, f[5:].copy())]


@functools.lru_cache(maxsize=None)
def instances_case():
    """(meshes, inst_mesh i32[3100], model_views f64[3100,4,4]): instance k is fronto-parallel over the centre of cell k (row-major
    in the 80 x 60 grid), at its own depth, with a projected half width of 1.1 .. 1.65 pixels: it covers the 2 x 2 pixel centres
    in the middle of its cell and stays inside the cell.  The case for K instances is the first K of these."""
    rng = np.random.default_rng(1024)
    meshes = instance_meshes()
    assert [m[1].shape[0] for m in meshes] == [2, 12, 7]
    inst = rng.integers(0, 3, INST_K_MAX).astype(np.int32)                # non-periodic: irregular prefix sums
    d = rng.uniform(0.8, 1.6, INST_K_MAX)
    half_px = rng.uniform(1.1, 1.65, INST_K_MAX)
    mvs = np.empty((INST_K_MAX, 4, 4))
    for k in range(INST_K_MAX):
        u, v = (k % INST_COLS) * INST_CELL + 0.5 * INST_CELL, (k // INST_COLS) * INST_CELL + 0.5 * INST_CELL
        t = [(u - 0.5 * INST_W) / INST_FX * d[k], -(v - 0.5 * INST_H) / INST_FY * d[k], -d[k]]
        mvs[k] = FR.model(t, scale=half_px[k] * d[k] / INST_FX)
    return meshes, inst, mvs


def cell_of_pixels(rows, cols):
    return (rows // INST_CELL) * INST_COLS + cols // INST_CELL


@functools.lru_cache(maxsize=None)
def instances_ref():
    """{K: (depth, labels)} of the restatement for every K of INST_KS, from one streaming pass over the 3100 instances"""
    meshes, inst, mvs = instances_case()
    return FR.raster_instances_ref(meshes, inst, mvs, INST_FX, INST_FY, INST_W, INST_H, at=INST_KS)


def instance_windows(K, pad=8):
    """per instance, the pixel window (c0, r0, c1, r1), inclusive, of its cell with `pad` pixels around it"""
    k = np.arange(K)
    c0, r0 = (k % INST_COLS) * INST_CELL, (k // INST_COLS) * INST_CELL
    return np.stack([np.maximum(c0 - pad, 0), np.maximum(r0 - pad, 0), np.minimum(c0 + INST_CELL - 1 + pad, INST_W - 1),
                     np.minimum(r0 + INST_CELL - 1 + pad, INST_H - 1)], -1)


# ------------------------------------------------------------------------------------------------ 2. NMS
NMS_THRESH = 0.3
NMS_SIZES = (960, 961, 1023, 1024)      # 15 full words; one bit in word 15; word 15 short of one bit; the cap
NMS_EDGES = (0.8, 1.0, 1.25)
NMS_MANY_GROUPS, NMS_MANY_SIZES = 3000, (0, 0, 1, 1, 2, 3, 65)
# the largest |evaluation.compute_3d_iou - closed form| measured over 40 000 pairs of the four single-group cases below (10 000 each,
# nine in ten of them overlapping); test_limits_cpu.py re-measures a sample against it, test_gpu_limits.py allows the device 4 x this
NMS_HOST_IOU_DEVIATION = 7.3e-16         # (measured: 7.22e-16)
NMS_PITCH = (0.3, 0.8, 1.0)             # of the lattice of centres: neighbours overlap around the threshold


def aligned_boxes(rng, m, levels=7):
    """m axis-aligned boxes (RT = identity rotation + translation), edges from NMS_EDGES, centres on a jittered lattice whose
    pitch along x makes neighbours overlap around the threshold; scores on `levels` levels"""
    nx = max(1, int(np.ceil(m ** (1 / 3) * 1.6)))
    ny = max(1, int(np.ceil(np.sqrt(m / nx))))
    cell = np.arange(m)
    lattice = np.stack([cell % nx, (cell // nx) % ny, cell // (nx * ny)], -1).astype(np.float64)
    centres = lattice * np.array(NMS_PITCH) + rng.uniform(-0.12, 0.12, (m, 3))
    centres = centres[rng.permutation(m)]
    RT = np.tile(np.eye(4), (m, 1, 1))
    RT[:, :3, 3] = centres
    scales = rng.choice(NMS_EDGES, (m, 3))
    scores = rng.integers(0, levels, m).astype(np.float64)
    return RT, scales, scores


def aligned_iou(RT, scales, i=None, j=None):
    """closed-form IoU of axis-aligned boxes: the full [m, m] matrix (diagonal 0), or the vector for the index arrays (i, j).
    An intersection of at most 1e-9 of the smaller volume is 0 (evaluation._iou_frames' rule, include/cppf.h)."""
    c, h = RT[:, :3, 3], 0.5 * scales
    lo, hi = c - h, c + h
    if i is None:
        ov = np.clip(np.minimum(hi[:, None], hi[None]) - np.maximum(lo[:, None], lo[None]), 0, None).prod(-1)
        vol = scales.prod(-1)
        va, vb = vol[:, None], vol[None]
    else:
        ov = np.clip(np.minimum(hi[i], hi[j]) - np.maximum(lo[i], lo[j]), 0, None).prod(-1)
        va, vb = scales[i].prod(-1), scales[j].prod(-1)
    iou = np.where(ov <= 1e-9 * np.minimum(va, vb), 0.0, ov / (va + vb - ov))
    if i is None:
        np.fill_diagonal(iou, 0.0)
    return iou


def greedy_pick(scores, over):
    """the header's rule on a boolean `IoU > thresh` matrix: descending score, equal scores the higher index first"""
    order = np.argsort(scores, kind="stable")[::-1]
    alive, pick = np.ones(len(scores), bool), []
    for b in order:
        if alive[b]:
            pick.append(int(b))
            alive &= ~over[b]
    return pick


def pack_bits(over):
    """an [m, m] boolean matrix as the device's bit matrix: m rows of ceil(m / 64) little-endian 64-bit words, flat"""
    m = over.shape[0]
    wpr = (m + 63) // 64
    rows = np.zeros((m, wpr * 64), bool)
    rows[:, :m] = over
    return np.packbits(rows.reshape(m, wpr, 64), axis=-1, bitorder="little").view(np.uint64).reshape(-1)


@functools.lru_cache(maxsize=None)
def nms_group(m):
    """(RT, scales, scores, closed-form IoU matrix) of the single-group case of m boxes: the first seed at which the LAST box is
    suppressed, so that the last word of the removed set decides the answer even where it holds one bit (m = 961)"""
    for seed in range(5000 + m, 5000 + m + 64 * 2000, 2000):
        RT, scales, scores = aligned_boxes(np.random.default_rng(seed), m)
        iou = aligned_iou(RT, scales)
        if m - 1 not in greedy_pick(scores, iou > NMS_THRESH):
            return RT, scales, scores, iou
    raise AssertionError(m)


@functools.lru_cache(maxsize=None)
def nms_many_groups():
    """(RT, scales, scores, sizes, [closed-form IoU matrix per group]): 3000 groups in one call, sizes from NMS_MANY_SIZES, groups
    without pairs at the front, in the middle and as the last"""
    rng = np.random.default_rng(3000)
    sizes = rng.choice(NMS_MANY_SIZES, NMS_MANY_GROUPS)
    sizes[[0, 1]], sizes[[1499, 1500, 1501]], sizes[-1] = (0, 1), (0, 1, 0), 0
    sizes[2], sizes[-2] = 65, 65
    parts = [aligned_boxes(rng, int(m)) for m in sizes]
    RT, scales, scores = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return RT, scales, scores, sizes, [aligned_iou(p[0], p[1]) for p in parts]


def coincident_boxes():
    """(RT[6,4,4], scales[6,3], pairs, closed-form IoU): two identical boxes (1), two that share a face (0), one inside another
    (the ratio of the volumes)"""
    at = lambda x, y, z: FR.model([x, y, z])
    RT = np.stack([at(0.3, -0.2, 0.9), at(0.3, -0.2, 0.9), at(0.0, 0.0, 0.0), at(1.0, 0.0, 0.0), at(0.1, 0.05, -0.05), at(0.0, 0.0, 0.0)])
    scales = np.array([[0.8, 1.0, 1.25]] * 2 + [[1.0, 0.8, 1.25]] * 2 + [[0.5, 0.25, 0.5], [1.0, 1.0, 1.25]])
    pairs = np.array([[0, 1], [2, 3], [4, 5]])
    return RT, scales, pairs, np.array([1.0, 0.0, 0.5 * 0.25 * 0.5 / 1.25])


# ------------------------------------------------------------------------------------------------ 3. pose-eval pairs
PE_CHUNK = 20000                        # pairs of one single-trip call: at most 400 000 work items
PE_N_BOXES = 300


def random_boxes(rng, m, side):
    """the generator of test_gpu_box_nms._random_boxes: random rotations, centres in a cube of `side`, extents 0.5 .. 1.5"""
    from scipy.spatial.transform import Rotation
    RT = np.tile(np.eye(4), (m, 1, 1))
    RT[:, :3, :3] = Rotation.random(m, random_state=int(rng.integers(1 << 30))).as_matrix()
    RT[:, :3, 3] = rng.uniform(-0.5 * side, 0.5 * side, (m, 3))
    return RT, rng.uniform(0.5, 1.5, (m, 3))


def pose_eval_case(n_plain, n_swept, seed):
    """dict(pred RT / scales, gt RT / scales, up-symmetry flags, pairs i32[M,2], sweep i32[M], item_off i64[M+1]): random boxes,
    random pairs, the swept pairs scattered among the plain ones"""
    rng = np.random.default_rng(seed)
    a, sa = random_boxes(rng, PE_N_BOXES, 2.5)
    b, sb = random_boxes(rng, PE_N_BOXES, 2.5)
    M_ = n_plain + n_swept
    sweep = np.zeros(M_, np.int32)
    sweep[rng.permutation(M_)[:n_swept]] = 1
    pairs = rng.integers(0, PE_N_BOXES, (M_, 2)).astype(np.int32)
    item_off = np.concatenate([[0], np.cumsum(np.where(sweep != 0, PE_SYM, 1))]).astype(np.int64)
    return dict(pred_RT=a, pred_scales=sa, gt_RT=b, gt_scales=sb, up_sym=(rng.random(PE_N_BOXES) < 0.5).astype(np.int32), pairs=pairs,
                sweep=sweep, item_off=item_off)


def straddling_pair(item_off):
    """the pair whose work items hold item PE_LANES_TOTAL - 1, the last of the first trip"""
    return int(np.searchsorted(item_off, PE_LANES_TOTAL - 1, side="right") - 1)


# ------------------------------------------------------------------------------------------------ 4. smoothing and proposals
SMOOTH_GRIDS = ((1, 1, 1), (2, 2, 2), (33, 7, 70), (65, 64, 9))           # lines shorter than the radius: reflect repeats
# (sigma, truncate, radius): the radii 0, 31 and 32 through `truncate` at sigma 1, and 31 / 32 again with a sigma at which the
# outermost weights still reach the float32 result
SMOOTH_PARAMS = ((1.0, 0.0, 0), (1.0, 31.0, 31), (1.0, 32.0, 32), (7.75, 4.0, 31), (8.0, 4.0, 32))


def smooth_grid_case(shape):
    return (np.random.default_rng(sum(shape)).random(shape) * 500).astype(np.float32)


MARGIN_GRID = (140, 137, 131)           # no dimension a multiple of 8; 2 * 64 = 128 < every dimension
MARGIN_PEAKS = ((0, 0, 0), (70, 0, 65), (70, 68, 65), (139, 136, 130))   # a corner, a face, the interior, the opposite corner


@functools.lru_cache(maxsize=None)
def margin_grid():
    """noise below 1 and four single-cell peaks; smoothed (sigma 1, reflect) they come out near 527 (corner), 403 (face), 413
    (interior) and 395 (opposite corner): a peak on the last planes is never suppressed -- the notebook's half-open box -- so it is
    the lowest and comes last"""
    g = np.random.default_rng(64).random(MARGIN_GRID).astype(np.float32)
    for p, a in zip(MARGIN_PEAKS, (2000.0, 3950.0, 6500.0, 1500.0)):
        g[p] = a
    return g


@functools.lru_cache(maxsize=None)
def margin_grid_smoothed():
    return Z.smooth(margin_grid())


PLATEAU_GRID = (90, 85, 83)             # 12 x 11 x 11 = 1452 tiles: more than the loop kernel's 1024 lanes
# the same maximum in five cells of five tiles; ascending flat index is NOT ascending tile index: (1, 9, 4) lies in tile (0, 1, 0),
# (0, 17, 4) in tile (0, 2, 0)
PLATEAU_CELLS = ((1, 9, 4), (0, 17, 4), (40, 83, 81), (88, 3, 40), (47, 40, 7))


def plateau_grid():
    g = np.random.default_rng(5).integers(0, 4, PLATEAU_GRID).astype(np.float32)
    for c in PLATEAU_CELLS:
        g[c] = 1000.0
    return g


def plateau_order():
    """the five cells by flat index: np.argmax returns the first of equal maxima"""
    return sorted(PLATEAU_CELLS, key=lambda c: (c[0] * PLATEAU_GRID[1] + c[1]) * PLATEAU_GRID[2] + c[2])


# ------------------------------------------------------------------------------------------------ 5. pair filter, segmentation
SCENE_P, SCENE_N = SCENE_LANES_TOTAL + 333, 5000          # every lane takes a second trip or is in the ragged tail
SCENE_MIN_CONTRIB = 50


def _bad_positions(rng):
    """about 1000 positions: 720 in the first trip, 200 in the second trip's full workgroup, and the whole ragged tail behind it
    (77 pairs), the first and last pair of each trip among them"""
    first = rng.choice(SCENE_LANES_TOTAL, 720, replace=False)
    second = SCENE_LANES_TOTAL + rng.choice(256, 200, replace=False)
    tail = np.arange(SCENE_LANES_TOTAL + 256, SCENE_P)
    return np.unique(np.concatenate([first, second, tail, [0, SCENE_LANES_TOTAL - 1, SCENE_LANES_TOTAL, SCENE_P - 1]]))


@functools.lru_cache(maxsize=None)
def scene_cloud():
    """the cloud of test_gpu_zero_shot's pair-filter test: half of the points coplanar with parallel normals"""
    rng = np.random.default_rng(21)
    pc = rng.standard_normal((SCENE_N, 3)).astype(np.float32)
    nrm = rng.standard_normal((SCENE_N, 3)).astype(np.float32)
    nrm[:SCENE_N // 2] = [0, 0, 1]
    pc[:SCENE_N // 2, 2] = 0.25
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return pc, nrm


@functools.lru_cache(maxsize=None)
def scene_pairs(bad):
    """idx i64[P,2] over N points.  bad: no / 'i32' / 'i64' -- about 1000 pairs get one endpoint at -1, N, or the largest value of
    the index type (for 'i64' also 2^32 + 7, which a truncation to 32 bits would turn into a valid index); returns (idx, the
    positions of the bad pairs, which endpoint is bad)"""
    rng = np.random.default_rng(55)
    idx = rng.integers(0, SCENE_N, (SCENE_P, 2))
    if not bad:
        return idx, np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = _bad_positions(rng)
    values = [-1, SCENE_N, INT32_MAX] if bad == "i32" else [-1, SCENE_N, INT64_MAX, 2 ** 32 + 7]
    side = rng.integers(0, 2, len(pos))
    idx[pos, side] = np.asarray(values, np.int64)[np.arange(len(pos)) % len(values)]
    return idx, pos, side


@functools.lru_cache(maxsize=None)
def scene_distinct(bad):
    """Z.distinct_mask of scene_pairs(bad) over scene_cloud()"""
    return Z.distinct_mask(*scene_cloud(), scene_pairs(bad)[0])


@functools.lru_cache(maxsize=None)
def scene_survivors():
    """about 3 % of the pairs, and every second pair with a bad endpoint"""
    surv = np.random.default_rng(56).random(SCENE_P) < 0.03
    surv[scene_pairs("i32")[1][::2]] = True
    return surv
