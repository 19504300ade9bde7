"""Yardstick of the DSM extraction (csrc/dsm.hip, scream_amd/dsm.py): a float64 numpy restatement of the contract in
include/scream_hip.h, and the seeded tiles the host and GPU tests share.  Nothing here imports scream_amd or touches a GPU;
tests/test_dsm_host.py pins it to the reference's literal fp32 statement before tests/test_gpu_dsm.py holds the kernels to it
bit for bit.

Why bit for bit.  Every step of the contract is one IEEE operation with one rounding:
    R  = float64(float32(radius)),  R2 = R * R                     (exact: the square of a 24-bit number)
    dx = float32(p.x - q.x), dy = float32(p.y - q.y)               fp32 subtractions
    d2 = float64(dx) * float64(dx) + float64(dy) * float64(dy)     exact products, one rounding of the sum
    candidate iff d2 <= R2;  winner: largest z, then lowest row;  none: the ground point itself, index -1
It is written independently of the product: one brute-force pass over the whole window per ground point, no grid.
"""
import numpy as np


def dsm_ref(patch, dem, radius=0.8):
    """patch [M,3], dem [N,3] (used as fp32) -> (dsm fp32 [N,3], idx int32 [N]): what the kernels must return, bit for bit."""
    p = np.ascontiguousarray(patch, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(dem, dtype=np.float32).reshape(-1, 3)
    R = np.float64(np.float32(radius))
    R2 = R * R
    out, idx = q.copy(), np.full(q.shape[0], -1, dtype=np.int32)
    px, py, pz = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    for j in range(q.shape[0]):
        dx = (px - q[j, 0]).astype(np.float64)  # the subtraction itself is fp32
        dy = (py - q[j, 1]).astype(np.float64)
        cand = np.nonzero(dx * dx + dy * dy <= R2)[0]
        if cand.size:
            w = cand[np.argmax(pz[cand])]  # the first maximum in ascending row order
            out[j], idx[j] = p[w], w
    return out, idx


def centre_ref(dsm, dem):
    """process_open_gf.py:234-242 on fp32 arrays, as numpy does it: -> (dsm_dem fp32 [n,6], centre fp32 [1,3])."""
    dsm, dem = np.asarray(dsm, dtype=np.float32), np.asarray(dem, dtype=np.float32)
    both = np.concatenate([dsm, dem], axis=0)
    centre = ((both.min(axis=0) + both.max(axis=0)) / np.float32(2)).reshape(1, 3)
    assert centre.dtype == np.float32
    return np.concatenate([dsm - centre, dem - centre], axis=1), centre


def windows_ref(kind):
    """The window ranges of the three splits, written out from their description: 100 m windows; train every 25 m up to
    [400, 500] on both axes, val side by side over 500 m, test side by side over 2 600 m x 2 500 m."""
    step, nx, ny = {"train": (25, 17, 17), "val": (100, 5, 5), "test": (100, 26, 25)}[kind]
    return [[i * step, i * step + 100] for i in range(nx)], [[i * step, i * step + 100] for i in range(ny)]


def seeded_tile(seed, n, side, offset=0.0):
    """(xyz fp32 [n,3], cls int64 [n]): xy uniform on [0, side)^2 plus offset, ground 8 sin(0.01 x) + 6 cos(0.015 y), 30 % of
    the points 'vegetation' lifted by uniform(1, 12) metres; class 1 = ground, 2 = the rest."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, side, size=(n, 2)) + offset
    z = 8 * np.sin(0.01 * xy[:, 0]) + 6 * np.cos(0.015 * xy[:, 1])
    veg = rng.random(n) < 0.3
    z = z + np.where(veg, rng.uniform(1.0, 12.0, size=n), 0.0)
    xyz = np.ascontiguousarray(np.concatenate([xy, z[:, None]], axis=1), dtype=np.float32)
    return xyz, np.where(veg, 2, 1).astype(np.int64)
