"""Yardstick of the fixed-radius search (csrc/radius.hip, scream_amd/overlap.py): a brute-force float64 numpy restatement of the
contract in include/scream_hip.h -- every source point against every target point, no grid -- and the seeded pairs the host and
GPU tests share.  Nothing here imports scream_amd or touches a GPU.

Why bit for bit.  Every step of the contract is one IEEE float64 operation with one rounding, in a stated order (numpy does not
contract a * b + c), so two faithful implementations are the same sequence:
    a_k = ((M[k][0]*x0 + M[k][1]*x1) + M[k][2]*x2) + M[k][3]       x the fp32 source point, converted exactly
    d_k = a_k - float64(b_k)                                       b the fp32 target point
    d2  = (d0*d0 + d1*d1) + d2*d2
    j is a neighbour of i  iff  d2 < radius * radius               strict
    the neighbours of i in ascending (d2, j), the first K of them
"""
import numpy as np

CHUNK = 512  # source rows per block of the dense comparison


def transform64(src, T):
    """float64 [N,3]: the contract's a_k for every source row."""
    x = np.asarray(src, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    M = np.asarray(T, dtype=np.float64)
    return np.stack([((M[k, 0] * x[:, 0] + M[k, 1] * x[:, 1]) + M[k, 2] * x[:, 2]) + M[k, 3] for k in range(3)], axis=1)


def radius_ref(src, tgt, T, radius, K=None):
    """src [N,3], tgt [M,3] (used as fp32), T float64 4x4, radius a float -> (count int32 [N], pairs int64 [n,2]): count before
    any K; pairs (i, j) in ascending i, the neighbours of one i in ascending (d2, j), at most K of them (None: all)."""
    a = transform64(src, T)
    b = np.asarray(tgt, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    R2 = np.float64(radius) * np.float64(radius)
    count = np.zeros(a.shape[0], dtype=np.int32)
    blocks = []
    for s in range(0, a.shape[0], CHUNK):
        d0 = a[s:s + CHUNK, None, 0] - b[None, :, 0]
        d1 = a[s:s + CHUNK, None, 1] - b[None, :, 1]
        d2 = a[s:s + CHUNK, None, 2] - b[None, :, 2]
        sq = (d0 * d0 + d1 * d1) + d2 * d2
        i, j = np.nonzero(sq < R2)
        count[s:s + CHUNK] = np.bincount(i, minlength=sq.shape[0])
        order = np.lexsort((j, sq[i, j], i))  # the last key is the most significant
        i, j = i[order], j[order]
        if K is not None and i.size:
            first = np.searchsorted(i, i, side="left")  # where the run of every row begins
            keep = np.arange(i.size) - first < K
            i, j = i[keep], j[keep]
        blocks.append(np.stack([i + s, j], axis=1).astype(np.int64))
    pairs = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, 2), np.int64)
    return count, pairs.reshape(-1, 2)


def count_fp32(src, tgt, T, radius):
    """The same search with every step in fp32 (matrix, transform, differences, squares, radius): what the contract is NOT."""
    x = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    b = np.asarray(tgt, dtype=np.float32).reshape(-1, 3)
    M = np.asarray(T, dtype=np.float32)
    a = np.stack([((M[k, 0] * x[:, 0] + M[k, 1] * x[:, 1]) + M[k, 2] * x[:, 2]) + M[k, 3] for k in range(3)], axis=1)
    assert a.dtype == np.float32
    R2 = np.float32(radius) * np.float32(radius)
    count = np.zeros(a.shape[0], dtype=np.int32)
    for s in range(0, a.shape[0], CHUNK):
        d = a[s:s + CHUNK, None, :] - b[None, :, :]
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        count[s:s + CHUNK] = (sq < R2).sum(axis=1)
    return count


def rotation(rng, max_deg=180.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.radians(max_deg) * rng.uniform(-1, 1)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def room_points(rng, n, size=3.0):
    """Points on the walls of a size^3 room, a few millimetres thick: most points of an indoor scan lie on planes."""
    p = rng.uniform(0, size, size=(n, 3))
    wall = rng.integers(0, 3, size=n)
    p[np.arange(n), wall] = np.where(rng.random(n) < 0.5, 0.0, size) + rng.normal(0, 0.004, size=n)
    return p


def room_pair(seed, n_src=4096, n_tgt=4096, transform="identity", size=3.0, noise=0.02):
    """(src fp32 [n_src,3], tgt fp32 [n_tgt,3], T float64 4x4): a target on the walls of a room; half of the source points are
    target points moved by N(0, noise) (neighbours at every distance up to and beyond 0.03), the rest lie elsewhere on the walls.
    transform: "identity"; "rigid" a general rotation and a translation of about a metre; "far" the same with the translation
    at 1000 -- the source is stored in its own frame, R^T (world - t), so its fp32 coordinates are about 1000."""
    rng = np.random.default_rng(seed)
    world_t = room_points(rng, n_tgt, size)
    half = min(n_src // 2, n_tgt)
    near = world_t[rng.permutation(n_tgt)[:half]] + rng.normal(0, noise, size=(half, 3))
    world_s = np.concatenate([near, room_points(rng, n_src - half, size)], axis=0)[rng.permutation(n_src)]
    T = np.eye(4)
    if transform != "identity":
        T[:3, :3] = rotation(rng)
        T[:3, 3] = rng.uniform(-1.5, 1.5, size=3) + (1000.0 if transform == "far" else 0.0)
    src = (world_s - T[:3, 3]) @ T[:3, :3]  # rows R^T (w - t)
    return np.ascontiguousarray(src, dtype=np.float32), np.ascontiguousarray(world_t, dtype=np.float32), T


LATTICE_RADIUS = 0.625
LATTICE_ANCHORS = np.asarray([[-8, -8, -8], [16, 16, 16]], dtype=np.float32)


def lattice_pair(k):
    """Target and queries on the multiples of 1/8 in [0, 1.25]^3 (11^3 nodes; every coordinate, difference, square and sum is
    exact), shifted as a whole by k/16.  At radius 5/8 a query has neighbours at offsets like (3, 4, 0)/8 and (5, 0, 0)/8 with
    d2 == R2 exactly: excluded.  Two target rows at -8 and 16 are NOT shifted: they fix the kernel's grid (1 333 rows give 32
    cells per axis, 24 / 32 = 0.75 = six lattice steps from -8), so at k = 0 every sixth lattice plane is a cell border and the
    shifts move the scene against the borders.  The anchors are out of every query's reach."""
    g = np.stack(np.meshgrid(*[np.arange(11)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 0.125 + k / 16.0
    rng = np.random.default_rng(300 + k)
    tgt = np.concatenate([g[rng.permutation(g.shape[0])].astype(np.float32), LATTICE_ANCHORS], axis=0)
    return g.astype(np.float32), tgt, np.eye(4)


BOX_DIRECTIONS = np.asarray([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=np.float64)


def outside_pair(radius, seed=40):
    """A target in the unit cube holding the 26 face centres, edge midpoints and corners of the cube; the source: behind each of
    them, outward along its direction, one point at 0.99 of the radius (within reach of it), one at 1.01 (beyond reach of
    everything), one ten radii away.  Returns (src [78,3], tgt, T, within bool [78], beyond bool [78])."""
    rng = np.random.default_rng(seed)
    border = 0.5 + 0.5 * BOX_DIRECTIONS
    tgt = np.concatenate([rng.uniform(0.0, 1.0, size=(500, 3)), border], axis=0)
    unit = BOX_DIRECTIONS / np.linalg.norm(BOX_DIRECTIONS, axis=1, keepdims=True)
    src = np.concatenate([border + unit * radius * f for f in (0.99, 1.01, 10.0)], axis=0)
    within = np.arange(78) < 26
    return src.astype(np.float32), tgt.astype(np.float32), np.eye(4), within, ~within


def degenerate_pairs(seed=50):
    """[(name, src, tgt)]: targets with no extent on three, two or one axes, one-point clouds, empty clouds."""
    rng = np.random.default_rng(seed)
    z = lambda n: np.zeros((n, 3), np.float32)
    q = rng.uniform(-0.1, 0.1, size=(200, 3))
    point = np.tile([[0.25, -1.5, 3.0]], (300, 1))
    line = np.stack([rng.uniform(0, 2, size=300), np.full(300, 0.5), np.full(300, -0.5)], axis=1)
    plane = np.stack([rng.uniform(0, 2, size=300), rng.uniform(0, 2, size=300), np.full(300, 1.0)], axis=1)
    near = lambda t: t[rng.integers(0, t.shape[0], size=200)] + rng.normal(0, 0.02, size=(200, 3))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return [("coincident", f(point[:200] + q * 0.5), f(point)), ("line", f(near(line)), f(line)), ("plane", f(near(plane)), f(plane)),
            ("one target", f(point[:200] + q * 0.4), f(point[:1])), ("one source", f(point[:1] + 0.01), f(point + rng.normal(0, 0.02, size=(300, 3)))),
            ("one and one", f([[0, 0, 0]]), f([[0.01, 0.01, 0.01]])), ("no target", f(q), z(0)), ("no source", z(0), f(plane))]
