"""Yardstick of voxel_down_sample (csrc/voxel.hip, scream_amd/voxel.py): a float64 numpy restatement of the contract in
include/scream_hip.h, and the seeded clouds the host and GPU tests share.  Nothing here imports scream_amd or touches a GPU;
tests/test_voxel_host.py pins it to scream_amd.evaluate_open_gf.voxel_down_sample, which predates the kernels, before
tests/test_gpu_voxel.py holds the kernels to it bit for bit.

Why bit for bit.  Every step of the contract is one IEEE operation with one rounding, in a stated order, so two faithful
implementations are the same sequence:
    origin = float64(min fp32 coordinate) - voxel * 0.5                        one multiply (exact: x 0.5), one subtract
    index  = floor((float64(p) - origin) / voxel)                              subtract, DIVIDE (not x 1/voxel), floor
    sum    = (((0.0 + p_a) + p_b) + ...) over the voxel's points, ascending ROW INDEX, in float64
    row    = float32(sum / float64(count))                                     one divide, one rounding to fp32
    order  = ascending (i, j, k), i most significant
It is written independently of the product's restatement: a stable lexsort and run boundaries instead of np.unique(axis=0),
np.bincount (a plain loop over the rows in index order, float64 weights) instead of np.add.at.
"""
import numpy as np

AXIS_CELLS = 1 << 21  # a cloud needing more cells than this on an axis is refused by the kernels (length -1)


def voxel_ref(points, voxel):
    """points [N,3] (any float type; used as float64), voxel a float -> (keys int64 [M,3], counts int64 [M], centroids float64
    [M,3]) in ascending (i, j, k).  Cast the centroids with .astype(np.float32) to compare with the kernels."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    if n == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
    voxel = float(voxel)
    origin = pts.min(axis=0) - voxel * 0.5
    idx = np.floor((pts - origin) / voxel).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < AXIS_CELLS, "outside the kernels' grid: such a cloud is refused, not down-sampled"
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))  # stable; the last key is the most significant
    s = idx[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    keys = s[head]
    ordinal = np.empty(n, dtype=np.int64)
    ordinal[order] = np.cumsum(head) - 1  # the voxel of every ORIGINAL row
    m = keys.shape[0]
    counts = np.bincount(ordinal, minlength=m).astype(np.int64)
    sums = np.stack([np.bincount(ordinal, weights=pts[:, a], minlength=m) for a in range(3)], axis=1)
    return keys, counts, sums / counts[:, None].astype(np.float64)


def ref32(points, voxel):
    """(keys, counts, fp32 centroids) of an fp32 cloud: what the kernels must return, bit for bit."""
    k, c, x = voxel_ref(np.asarray(points, dtype=np.float32).astype(np.float64), voxel)
    return k, c, x.astype(np.float32)


def seeded_cloud(kind, n, seed):
    """fp32 [n,3] clouds scaled like the datasets the reference down-samples:
    "3dmatch" an indoor fragment, ~3 m of walls and clutter (voxel 0.0625); "kitti" a LiDAR sweep, 120 m across and 4 m high
    (voxels 0.3 and 0.7); "opengf" a 500 m terrain tile with smooth relief (voxel 20); "uniform" the unit cube."""
    rng = np.random.default_rng(seed)
    if kind == "3dmatch":
        p = rng.uniform(-1.5, 1.5, size=(n, 3))
        wall = rng.integers(0, 3, size=n)
        p[np.arange(n), wall] = np.where(rng.random(n) < 0.5, -1.5, 1.5) + rng.normal(0, 0.004, size=n)  # most points lie on planes
    elif kind == "kitti":
        r = rng.uniform(2.0, 60.0, size=n)
        a = rng.uniform(0, 2 * np.pi, size=n)
        p = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 2.0, size=n)], axis=1)
    elif kind == "opengf":
        xy = rng.uniform(0, 500, size=(n, 2))
        p = np.concatenate([xy, (8 * np.sin(0.01 * xy[:, :1]) + 6 * np.cos(0.015 * xy[:, 1:]))], axis=1)
    elif kind == "uniform":
        p = rng.random(size=(n, 3))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=np.float32)
