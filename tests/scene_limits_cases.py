"""Seeded case builders for csrc/instances.hip, csrc/segments.hip and csrc/scene_train.hip at their caps, on the second trips of
their loops and on lists that break their promises (tests/test_gpu_scene_limits.py); that every case reaches the trip or branch it
is named for is shown from the restatements alone in tests/test_scene_limits_cpu.py.  tests/limits_cases.py does the same for the
older kernels.

The limits quoted from the device code:
  csrc/instances.hip    a chunk is CPPF_GATHER_CHUNK = 1024 dense points = 16 waves; gi_scatter_kernel's wave w sums rows w, w + 16
                        of counts[k][chunk], 64 columns per trip; CPPF_GATHER_MAX_CHUNKS = 8192
  csrc/segments.hip     CPPF_SEGMENTS_MAX = 1024 listed segments, staged into LDS 256 per trip (SEG_BLOCK); depth, tol_mm <= 65535,
                        slope_permille <= 1000, H W <= 2^24; pr_count_kernel: at most 512 workgroups of 256 lanes per trip
  csrc/scene_train.hip  st_draw_kernel's four guards; tr_bins / rot_bins in 2..256"""
import functools

import numpy as np

import instances_ref as IR
import scene_training_ref as TR
import segments_ref as SR

F32 = np.float32

# ------------------------------------------------------------------------------------------------ A. instance gather
CHUNK, TABLE_LANES, GI_WAVES, MAX_CHUNKS = 1024, 64, 16, 8192
FAR_START = TABLE_LANES * CHUNK                     # the first dense point of chunk 64: the table sum's second trip
EDGE_MS = (63, 64, 65, 1023, 1024, 1025)            # a wave and a chunk, one short, exact, one over
FAR_MS = (64 * CHUNK, 64 * CHUNK + 1, 65 * CHUNK + 7)      # 64 chunks (one full trip), 65 (one point in chunk 64), 66 (7 in chunk 65)
FAR_KS = (16, 17, 32)                               # one trip of the row loop, a ragged second trip, two full trips
N_SPARSE = 400
S_BOTH, S_NEAR, S_FAR = (0, 200), (200, 300), (300, 400)   # sparse points owned from both sides / from chunks < 64 / >= 64 only
S_STAR = 399                                        # the owner of the first and of the last far point, in every mask but the near-only one
FAR_ONLY_ROWS, NEAR_ONLY_ROW = (1, 20), 2


def far_rows(K):
    return tuple(r for r in FAR_ONLY_ROWS if r < K)


@functools.lru_cache(maxsize=None)
def gather_far_case(M, K):
    """(hi, nrm, owner, masks) with M dense points over more than 64 chunks (exactly 64 at M = 65 536) and K masks: rows far_rows(K)
    have members in chunks >= 64 only, row 2 in chunks < 64 only, every other row on both sides; the first point of chunk 64 and the last
    point belong to every row but row 2; 8 points have no owner.  Read-only: the arrays are shared."""
    rng = np.random.default_rng(M + K)
    hi, nrm = rng.standard_normal((M, 3)).astype(F32), rng.standard_normal((M, 3)).astype(F32)
    owner = rng.integers(0, S_NEAR[1], M).astype(np.int32)
    n_far = max(M - FAR_START, 0)
    if n_far:
        far = rng.integers(0, S_BOTH[1] + S_FAR[1] - S_FAR[0], n_far)
        owner[FAR_START:] = np.where(far < S_BOTH[1], far, far - S_BOTH[1] + S_FAR[0])
        owner[FAR_START] = owner[M - 1] = S_STAR
    owner[rng.permutation(FAR_START)[:8]] = -1
    masks = (rng.random((K, N_SPARSE)) < 0.3).astype(np.uint8) * np.uint8(3)
    masks[:, S_STAR] = 1
    for r in far_rows(K):
        masks[r, :S_FAR[0]] = 0
    masks[NEAR_ONLY_ROW, :S_NEAR[0]] = 0
    masks[NEAR_ONLY_ROW, S_FAR[0]:] = 0
    return hi, nrm, owner, masks


@functools.lru_cache(maxsize=None)
def gather_far_ref(M, K):
    """the roomy restatement of gather_far_case(M, K) and its total"""
    hi, nrm, owner, masks = gather_far_case(M, K)
    total = int(IR.gather_ref(hi, nrm, owner, masks, capacity=0)["offsets"][K])
    return IR.gather_ref(hi, nrm, owner, masks, capacity=total + 5), total


CAP_M = MAX_CHUNKS * CHUNK                          # 8 388 608 dense points: the largest cloud one pass takes
CAP_N_SPARSE, CAP_MEMBERS_OF = 16, (3, 7, 15)


@functools.lru_cache(maxsize=None)
def gather_cap_case():
    """(hi, nrm, owner, masks) at 8192 chunks, K = 1: about 70 points have an owner, half of them in the mask -- the first and the
    last point of the cloud, the points around the first chunk's end and around chunk 64's start among them.  Coordinates are distinct
    bit patterns of normal floats (the gather copies words)."""
    M = CAP_M
    rng = np.random.default_rng(8192)
    hi = (np.arange(3 * M, dtype=np.int32) + np.int32(0x3F000000)).view(F32).reshape(M, 3)
    nrm = (np.arange(3 * M, dtype=np.int32) + np.int32(0x40800000)).view(F32).reshape(M, 3)
    owner = np.full(M, -1, np.int32)
    fixed = np.array([0, CHUNK - 1, CHUNK, FAR_START - 1, FAR_START, M - CHUNK, M - 1])
    other = np.setdiff1d(rng.choice(M, 64, replace=False), fixed)
    owner[fixed] = np.resize(CAP_MEMBERS_OF, fixed.size)
    owner[other[::2]] = np.resize(CAP_MEMBERS_OF, other[::2].size)
    owner[other[1::2]] = np.resize((0, 1, 2), other[1::2].size)           # an owner outside the mask
    masks = np.zeros((1, CAP_N_SPARSE), np.uint8)
    masks[0, list(CAP_MEMBERS_OF)] = 1
    return hi, nrm, owner, masks


# ------------------------------------------------------------------------------------------------ B. depth segments
SEG_MAX, SEG_STAGE = 1024, 256                      # CPPF_SEGMENTS_MAX; seg_label_kernel stages `first` 256 entries per trip
SEG_PIXELS_MAX = 1 << 24


def cap_image(n):
    """n one-pixel components for n in 1023 / 1024 / 1025: the 32 x 64 checkerboard (1024), with one pixel killed, or with an isolated
    pixel in an added row"""
    d = SR.checkerboard(32, 64)
    if n == SEG_MAX - 1:
        d[17, 31] = 0
    elif n == SEG_MAX + 1:
        d = np.concatenate([d, np.zeros((1, 64), np.uint16)])
        d[32, 0] = 1000                             # (31, 0) is dead: nothing links it
    else:
        assert n == SEG_MAX
    return d


STAGING_FILTER = dict(min_pixels=3, max_pixels=6)
STAGING_WIDTH = 131                                 # no multiple of 64: runs cross wave and workgroup boundaries


@functools.lru_cache(maxsize=None)
def staging_image(n_kept):
    """runs of 2..7 live pixels along the rows of a 131-wide image, a dead pixel between two runs and a dead row between two rows of
    runs: sizes 3..6 pass STAGING_FILTER, 2 and 7 do not, in random order -- until n_kept runs pass, then a few more that do not"""
    rng = np.random.default_rng(n_kept)
    sizes, kept = [], 0
    while kept < n_kept:
        s = int(rng.choice([2, 3, 4, 5, 6, 7], p=[0.25, 0.125, 0.125, 0.125, 0.125, 0.25]))
        sizes.append(s)
        kept += 3 <= s <= 6
    sizes += [7, 2, 7]
    rows, cur = [], []
    for s in sizes:
        if len(cur) + s > STAGING_WIDTH:
            rows += [cur + [0] * (STAGING_WIDTH - len(cur)), [0] * STAGING_WIDTH]
            cur = []
        cur += [900 + 7 * s] * s + [0] * min(1, STAGING_WIDTH - len(cur) - s)
    rows.append(cur + [0] * (STAGING_WIDTH - len(cur)))
    return np.array(rows, np.uint16)


# (row, tol_mm, slope_permille, components): the link rule |dz| <= tol + slope min(z) / 1000 at the ends of its accepted ranges
LINK_ENDS = (((1, 65535), 65534, 0, 1), ((1, 65535), 65533, 0, 2), ((30000, 60000), 0, 1000, 1), ((30000, 60001), 0, 1000, 2),
             ((65535, 65535), 0, 1000, 1), ((65535, 1), 65535, 1000, 1))
LONG_ROW = 65537                                    # 1025 waves of one flat run, the last of one pixel

# (keyword, value) of the five refusals; every other argument is acceptable
SEG_REFUSALS = (("W", SEG_PIXELS_MAX + 1), ("cap", SEG_MAX + 1), ("slope", 1001), ("tol", 65536), ("mn", 0))


# ------------------------------------------------------------------------------------------------ C. plane RANSAC
PR_TRIP = 512 * 256                                 # points per trip of pr_count_kernel's capped launch
PLANE_NS = (PR_TRIP, PR_TRIP + 1, PR_TRIP + 65, 2 * PR_TRIP + 1)
PLANE_HYP, PLANE_THRESH, PLANE_TAIL = 64, 0.01, 65


@functools.lru_cache(maxsize=None)
def plane_case(N):
    """test_gpu_segments._plane_cloud(N): 60 % of the points on one plane, shuffled -- with a point of the plane in the LAST place
    (exchanged with the last point where that is an outlier): at N = 131 073 it is the whole second trip"""
    from test_gpu_segments import _plane_cloud
    pts, n = _plane_cloud(N, N % 1000)
    on = np.abs(pts.astype(np.float64) @ n - 1.2) < 0.004
    if not on[-1]:
        j = int(np.nonzero(on)[0][-1])
        pts[[j, N - 1]] = pts[[N - 1, j]]
    return pts


# ------------------------------------------------------------------------------------------------ D. scene training: the draw
DRAW_P, DRAW_N, DRAW_K, DRAW_SEED = 257, 300, 4, 0xD0A5
DRAW_FLAGS = np.array([1, 0, 1, 1], np.int32)       # instance 1 is of another category: an empty segment
DRAW_BREAKS = ("cap", "member_n", "member_neg", "label_K", "label_neg", "seg_neg", "empty_seg", "seg_past_M")
M_OFF, S_OFF, I_OFF = 64, 16, 64                    # where the arrays start inside their allocations


def _draw_base():
    inst = np.random.default_rng(77).integers(-1, DRAW_K, DRAW_N).astype(np.int32)
    members, seg_off = TR.members_ref(inst, DRAW_FLAGS)
    return inst, members, seg_off


@functools.lru_cache(maxsize=None)
def draw_case(name):
    """One broken promise.  dict(members_buf, seg_buf, inst_buf: the allocations, filled with junk that is IN RANGE (a point of the
    cloud, an offset in [0, M], a label in [0, K)) around the arrays, which start at M_OFF / S_OFF / I_OFF -- a guard that failed
    would read a wrong index, never outside an allocation; cap: the members capacity handed to the kernel; M: the well-formed list's
    length; bad: the value an altered member holds, or None).  name None: the well-formed lists."""
    inst, members, seg_off = _draw_base()
    M = int(members.shape[0])
    rng = np.random.default_rng(5)
    members_buf = rng.integers(0, DRAW_N, M_OFF + M + 256).astype(np.int32)
    seg_buf = rng.integers(0, M + 1, S_OFF + DRAW_K + 1 + 16).astype(np.int32)
    inst_buf = rng.integers(0, DRAW_K, I_OFF + DRAW_N + 64).astype(np.int32)
    m, s, i = members_buf[M_OFF:M_OFF + M], seg_buf[S_OFF:S_OFF + DRAW_K + 1], inst_buf[I_OFF:I_OFF + DRAW_N]
    m[:], s[:], i[:] = members, seg_off, inst
    bad, every = None, slice(0, None, 5)
    if name == "cap":
        s[DRAW_K] = M + 1                           # one more than the capacity handed over (M): members[M] is junk inside the buffer
    elif name in ("member_n", "member_neg"):
        bad = DRAW_N if name == "member_n" else -1
        m[every] = bad
    elif name in ("label_K", "label_neg"):
        i[members[every]] = DRAW_K if name == "label_K" else -1
    elif name == "seg_neg":
        s[2] = -1
    elif name == "empty_seg":
        bad = int(np.nonzero(inst == 1)[0][3])      # a point of instance 1, whose segment is empty
        m[every] = bad
    elif name == "seg_past_M":
        s[3] = M + 1
    else:
        assert name is None
    return dict(members_buf=members_buf, seg_buf=seg_buf, inst_buf=inst_buf, cap=M, M=M, bad=bad)


def draw_views(c):
    """(members from M_OFF to the end of its buffer, seg_off[K+1], inst[N]) of a draw_case, as the restatement reads them"""
    return c["members_buf"][M_OFF:], c["seg_buf"][S_OFF:S_OFF + DRAW_K + 1], c["inst_buf"][I_OFF:I_OFF + DRAW_N]


def draw_want(name, P=DRAW_P):
    """(idx, kept) of the lenient restatement on draw_case(name), every pair in the positive stratum"""
    c = draw_case(name)
    m, s, i = draw_views(c)
    return TR.draw_ref_lenient(m, c["cap"], s, i, DRAW_N, P, P, DRAW_SEED)


# ------------------------------------------------------------------------------------------------ D. scene training: the targets
EXACT_RANGE = (0.5, 0.5)                            # v0 = v1 = 0.5: mu is clamped to [0, 1], nu to [0, 0.5]
EXACT_BINS = ((3, 3), (2, 2))                       # bin widths 0.5 / 0.25 / fl(pi / 2), and 1 / 0.5 / fl(pi): exact quotients
_REL = [(0, 3, 0), (0, 1, 0), (0, 0.5, 0), (0, 2.5, 0), (0, -1.5, 0), (2, 2, 0), (2, 0, 0), (0.5, 2, 0), (0.5, 0, 0), (3, 0, 0), (1, 0, 0),
        (0, 0.25, 0), (np.nan, 0, 0), (np.inf, 1, 0), (0, -np.inf, 0)]
_NRM = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 1, 0), (1, 0, 0), (0, -1, 0), (1, 0, 0), (0, 1, 0), (1, 0, 0),
        (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0)]
EXACT_N_REL = len(_REL)
# name -> (a, b) among the points of one instance; every |a - b| is 2 (fl(2 + 1e-7) = 2: u is exactly an axis) or 0
EXACT_PAIRS = dict(mu_above=(0, 1), mu_below=(1, 0), mu_at_0=(2, 3), mu_at_top=(2, 4), nu_above=(5, 6), nu_at_top=(7, 8), right_par=(9, 10),
                   right_anti=(10, 9), coincident=(11, 11), nan_a=(12, 0), nan_b=(0, 12), inf_a=(13, 1), inf_b=(1, 14))
EXACT_CENTRES = ((0.5, -1.0, 2.0), (8.5, 1.0, 4.0), (-4.0, 0.0, 1.0))
EXACT_FLAGS = np.array([1, 7, 0], np.int32)         # a target; a target with both symmetry bits; another category


@functools.lru_cache(maxsize=None)
def exact_scene():
    """Three instances of the same 15 points around their centres (up = +y, right = +x), every coordinate a small multiple of 1/4.
    dict(pc, nrm, inst, table, flags, idx i32[P,2], names: per pair (name, instance)).  Pairs: EXACT_PAIRS inside instance 0, inside
    instance 1 (the symmetric one) and inside instance 2 (no target: negatives), then two pairs across instances."""
    pc = np.concatenate([np.asarray(_REL, F32) + np.asarray(c, F32) for c in EXACT_CENTRES])
    nrm = np.tile(np.asarray(_NRM, F32), (3, 1))
    inst = np.repeat(np.arange(3, dtype=np.int32), EXACT_N_REL)
    table = np.zeros((3, 12), F32)
    table[:, 0:3], table[:, 3:6], table[:, 6:9] = np.asarray(EXACT_CENTRES, F32), (0, 1, 0), (1, 0, 0)
    idx, names = [], []
    for k in range(3):
        for name, (a, b) in EXACT_PAIRS.items():
            idx.append((k * EXACT_N_REL + a, k * EXACT_N_REL + b))
            names.append((name, k))
    idx += [(0, EXACT_N_REL + 1), (EXACT_N_REL, 2 * EXACT_N_REL)]
    names += [("across", -1)] * 2
    return dict(pc=pc, nrm=nrm, inst=inst, table=table, flags=EXACT_FLAGS, idx=np.asarray(idx, np.int32), names=names)


def exact_want(tr_bins, rot_bins):
    s = exact_scene()
    return TR.targets_ref(s["pc"], s["nrm"], s["inst"], s["idx"], s["table"], s["flags"], EXACT_RANGE, tr_bins, rot_bins, dtype=F32)


# (low, w_low) per head of the named pairs at 3 x 3 bins, by hand: x = value / width, low = min(floor x, 1), w = 1 - (x - low); the
# angle heads are (plain instance, instance with both symmetry bits)
EXACT_BY_HAND = dict(
    mu_above=dict(mu=(1, 0.0), nu=(0, 1.0), up=((0, 1.0), (0, 1.0)), right=((1, 1.0), (1, 1.0))),      # 3.5 -> 1: x = 2; u = +up
    mu_below=dict(mu=(0, 1.0), nu=(0, 1.0), up=((1, 0.0), (0, 1.0)), right=((1, 1.0), (1, 1.0))),      # -0.5 -> 0; u = -up: pi, or 0
    mu_at_0=dict(mu=(0, 1.0), nu=(0, 1.0), up=((1, 0.0), (0, 1.0)), right=((1, 1.0), (1, 1.0))),       # exactly 0
    mu_at_top=dict(mu=(1, 0.0), nu=(0, 1.0), up=((0, 1.0), (0, 1.0)), right=((1, 1.0), (1, 1.0))),     # exactly 1 = 2 v0
    nu_above=dict(mu=(1, 0.0), nu=(1, 0.0), up=((0, 1.0), (0, 1.0)), right=((1, 1.0), (1, 1.0))),      # proj 2; |o| = 2 -> 0.5: x = 2
    nu_at_top=dict(mu=(1, 0.0), nu=(1, 0.0), up=((0, 1.0), (0, 1.0)), right=((1, 1.0), (1, 1.0))),     # |o| = 0.5 = v1
    right_par=dict(mu=(1, 0.0), nu=(0, 1.0), up=((1, 1.0), (1, 1.0)), right=((0, 1.0), (0, 1.0))),     # u = +right
    right_anti=dict(mu=(0, 1.0), nu=(0, 1.0), up=((1, 1.0), (1, 1.0)), right=((1, 0.0), (0, 1.0))),    # u = -right, proj = -1
    coincident=dict(mu=(1, 1.0), nu=(1, 1.0), up=((1, 1.0), (1, 1.0)), right=((1, 1.0), (1, 1.0))))    # u = 0: proj 0, |o| = |a| = 0.25
