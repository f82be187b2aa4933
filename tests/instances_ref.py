"""What cppf_amd.scene_stage.voxel_owner and cppf_gather_instances (csrc/instances.hip) are held to, in numpy, with a plain Python loop
beside each for the restatement itself (tests/test_instances_cpu.py), and the clouds of both test files.

  voxel of a point      floor((double)p / q) per axis, a TRUE division (cppf_voxel_dedupe's arithmetic, utils/util.py:117-121)
  owner[i]              the position in the sparse cloud hi[pc_index] of the point with dense point i's voxel, -1 where there is none
                        (the first such position where a caller's subset names a voxel twice)
  member[i] bit k       owner[i] >= 0 and masks[k][owner[i]] != 0
  offsets               exclusive prefix of the proposals' member counts; all zero with offsets[K] = -1 when an owner is >= N
  pts / nrm / src       proposal k's members in increasing dense index at rows offsets[k]:offsets[k+1]; rows >= capacity dropped"""
import numpy as np

F32 = np.float32
POISON_F, POISON_I = F32(-7.5), np.int32(-77)


def voxels(p, q):
    """i64[M,3]: floor(p / q) in fp64 by true division"""
    p64 = np.asarray(p, F32).astype(np.float64)
    return np.floor(p64 / np.full_like(p64, float(q))).astype(np.int64)


def voxels_reciprocal(p, q):
    """the mistake: floor(p * (1 / q)) -- what dividing a device tensor by a Python number computes"""
    p64 = np.asarray(p, F32).astype(np.float64)
    return np.floor(p64 * (1.0 / float(q))).astype(np.int64)


def _keys(v):
    v = v + (1 << 20)
    assert ((v >= 0) & (v < (1 << 21))).all()
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def owner_ref(hi, pc_index, q, voxel_fn=voxels):
    """i32[M]"""
    hi = np.asarray(hi, F32).reshape(-1, 3)
    pc_index = np.asarray(pc_index, np.int64).reshape(-1)
    if pc_index.size == 0:
        return np.full(hi.shape[0], -1, np.int32)
    key = _keys(voxel_fn(hi, q))
    sk = key[pc_index]
    order = np.argsort(sk, kind="stable")
    pos = np.searchsorted(sk[order], key)
    pos_c = np.minimum(pos, sk.size - 1)
    hit = (pos < sk.size) & (sk[order][pos_c] == key)
    return np.where(hit, order[pos_c], -1).astype(np.int32)


def owner_loop(hi, pc_index, q):
    """the same by a dictionary and a loop"""
    hi = np.asarray(hi, F32).reshape(-1, 3)
    first = {}
    for j, i in enumerate(np.asarray(pc_index).reshape(-1)):
        v = tuple(int(np.floor(float(c) / float(q))) for c in hi[int(i)])
        first.setdefault(v, j)
    return np.array([first.get(tuple(int(np.floor(float(c) / float(q))) for c in p), -1) for p in hi], np.int32).reshape(-1)


def gather_ref(hi, nrm, owner, masks, capacity=None, poison=True):
    """-> dict(member u32[M], offsets i32[K+1], pts f32[cap,3], nrm f32[cap,3], src i32[cap], bad).  Rows the call leaves alone hold
    POISON_F / POISON_I (what the device test fills its buffers with beforehand)."""
    hi, nrm = np.asarray(hi, F32).reshape(-1, 3), np.asarray(nrm, F32).reshape(-1, 3)
    owner, masks = np.asarray(owner, np.int32).reshape(-1), np.asarray(masks, np.uint8)
    K, N = masks.shape
    M = hi.shape[0]
    cap = M if capacity is None else int(capacity)
    out = dict(pts=np.full((cap, 3), POISON_F, F32), nrm=np.full((cap, 3), POISON_F, F32), src=np.full(cap, POISON_I, np.int32))
    if (owner >= N).any():
        return dict(out, member=None, offsets=np.array([0] * K + [-1], np.int32), bad=True)
    has = owner >= 0
    member = np.zeros(M, np.uint32)
    for k in range(K):
        inside = np.zeros(M, bool)
        inside[has] = masks[k][owner[has]] != 0
        member |= inside.astype(np.uint32) << np.uint32(k)
    counts = [int(((member >> np.uint32(k)) & 1).sum()) for k in range(K)]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    for k in range(K):
        rows = np.nonzero((member >> np.uint32(k)) & 1)[0]
        dst = offsets[k] + np.arange(rows.size)
        ok = dst < cap
        out["pts"][dst[ok]], out["nrm"][dst[ok]], out["src"][dst[ok]] = hi[rows[ok]], nrm[rows[ok]], rows[ok]
    return dict(out, member=member, offsets=offsets, bad=False)


def chunk_counts_ref(member, K, chunk=1024):
    """i64[K, ceil(M / chunk)]: the members of proposal k among the dense points [c chunk, (c + 1) chunk) -- the table
    gi_count_kernel writes and every workgroup of gi_scatter_kernel sums"""
    member = np.asarray(member, np.uint32)
    n_chunks = (member.shape[0] + chunk - 1) // chunk
    padded = np.zeros(n_chunks * chunk, np.uint32)
    padded[:member.shape[0]] = member
    return np.stack([((padded >> np.uint32(k)) & 1).reshape(n_chunks, chunk).sum(-1) for k in range(K)]).astype(np.int64)


def gather_loop(hi, nrm, owner, masks):
    """member, offsets and the packed rows by plain loops (roomy capacity, owners in range)"""
    K, N = np.asarray(masks).shape
    member, lists = [], [[] for _ in range(K)]
    for i, o in enumerate(owner):
        w = 0
        for k in range(K):
            if o >= 0 and masks[k][o] != 0:
                w |= 1 << k
                lists[k].append(i)
        member.append(w)
    offsets = [0]
    for k in range(K):
        offsets.append(offsets[-1] + len(lists[k]))
    flat = [i for l in lists for i in l]
    return (np.array(member, np.uint32), np.array(offsets, np.int32), np.asarray(hi, F32)[flat].reshape(-1, 3),
            np.asarray(nrm, F32)[flat].reshape(-1, 3), np.array(flat, np.int32))


# the quantisation sizes of the face clouds: 4 res of the configs with res = 0.03 and 0.004
FACE_Q = (0.12, 0.016)


def face_cloud(q, m_max=4100):
    """coordinates ON voxel faces at both signs: x = float32(m q) for m in -m_max..m_max (the float32 nearest to the face), y and z
    inside voxel 0.  -> (cloud f32[2 m_max + 1, 3], m)"""
    m = np.arange(-m_max, m_max + 1)
    p = np.zeros((m.size, 3), F32)
    p[:, 0] = (m.astype(np.float64) * float(q)).astype(F32)
    p[:, 1:] = F32(0.25 * q)
    return p, m


def small_face_cloud():
    """about 50 points for the loops: the faces m = -4075..-3950 step 25 and their mirror images at q = 0.12 (the negative ones are
    where floor(p * (1 / q)) and floor(p / q) part), each face three times (twice inside the same voxel), and a few interior points"""
    q = FACE_Q[0]
    m = np.concatenate([np.arange(-4075, -3949, 25), np.arange(3950, 4076, 25)])
    x = (m.astype(np.float64) * q).astype(F32)
    rng = np.random.default_rng(3)
    pts = []
    for v in x:
        for dy in (0.1, 0.6, 1.3):
            pts.append([v, F32(dy * q), F32(0.5 * q)])
    pts += (rng.uniform(-2, 2, (12, 3)) * q).tolist()
    return np.array(pts, F32), q


def case(M, K, N=300, seed=0, lone=8):
    """a gather case: M dense points, N sparse points, K masks.  Mask 0 is empty and mask K - 1 owns every sparse point (K >= 2; K = 1:
    a random mask), masks 1 and 2 share points, `lone` dense points (fewer when M is small) have owner -1."""
    rng = np.random.default_rng(seed)
    hi = rng.standard_normal((M, 3)).astype(F32)
    nrm = rng.standard_normal((M, 3)).astype(F32)
    owner = rng.integers(0, N, M).astype(np.int32)
    owner[rng.permutation(M)[:min(lone, M // 2)]] = -1
    masks = (rng.random((K, N)) < 0.3).astype(np.uint8) * np.uint8(1 + seed % 200)      # (any non-zero byte is membership)
    if K >= 2:
        masks[0] = 0
        masks[K - 1] = 1
    if K >= 3:
        masks[2, :N // 4] = masks[1, :N // 4] = 1
    return hi, nrm, owner, masks
