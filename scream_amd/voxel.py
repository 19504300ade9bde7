"""voxel_down_sample on the MI355X (csrc/voxel.hip): the step that turns a raw scan into the cloud the models see.

    coarse = voxel_down_sample(points, 0.0625)                         # [N,3] fp32 on the GPU -> [M,3]
    outs = voxel_down_sample_batch([a, b, c], [0.0625, 0.3, 0.7])      # one launch sequence for the whole list
    outs, counts = voxel_down_sample_batch(clouds, 20.0, return_counts=True)

The rules are open3d's legacy ``voxel_down_sample`` as scream_amd/evaluate_open_gf.py restates it (grid origin at
min_bound - voxel / 2, one centroid per occupied voxel), made exact: float64 indices and sums from the fp32 coordinates, sums in
ascending row index, rows in ascending (i, j, k) -- the order of ``np.unique(axis=0)``.  The result is a pure function of the
cloud (bitwise repeatable, independent of what else is in the batch; include/scream_hip.h states the contract).  Parity with
open3d itself is not pinned: it is not installed here, and its output order is that of a hash map.  There is no CPU path.
"""
from __future__ import annotations

from typing import List, Sequence, Union

import torch

from . import ops
from .clouds import check_clouds, check_radius, pack_clouds

__all__ = ["voxel_down_sample", "voxel_down_sample_batch"]


def voxel_down_sample_batch(clouds: Sequence[torch.Tensor], voxel: Union[float, Sequence[float]], return_counts: bool = False):
    """Down-sample every cloud ([N_i,3] fp32 on the GPU, N_i >= 0) at its voxel size (one float for all, or one per cloud).
    Returns the list of [M_i,3] centroids, or (that list, the list of int32 [M_i] point counts) with return_counts.  The clouds
    are packed and share every launch; the lengths come back in ONE device-to-host copy (the caller needs them to size what
    follows).  A cloud the kernels refuse -- more than 2^21 cells on an axis, a non-finite coordinate -- raises ValueError."""
    clouds = list(clouds)
    B = len(clouds)
    voxels = [float(v) for v in voxel] if isinstance(voxel, (list, tuple)) else [float(voxel)] * B
    if len(voxels) != B:
        raise ValueError("%d voxel sizes for %d clouds" % (len(voxels), B))
    if B == 0:
        return ([], []) if return_counts else []
    check_clouds(clouds, "cloud", op="voxel_down_sample", builtin_errors=True)
    for i, v in enumerate(voxels):
        check_radius(v, "cloud %d: voxel size" % i, ValueError)
    dev = clouds[0].device
    xyz, row0, lens = pack_clouds(clouds)
    meta = torch.tensor([row0, lens], dtype=torch.int32).to(dev)
    vox = torch.tensor(voxels, dtype=torch.float64).to(dev)
    out, out_len, out_cnt = ops.voxel_down_sample_packed(xyz, meta[0], meta[1], max(lens), vox, want_counts=return_counts)
    n_out = out_len.cpu().tolist()  # the one synchronising copy
    for i, m in enumerate(n_out):
        if m < 0:
            raise ValueError("voxel_down_sample: cloud %d (%d points, voxel %g) cannot be gridded: it holds a non-finite coordinate or "
                             "spans more than 2^21 voxels on an axis" % (i, lens[i], voxels[i]))
    pts: List[torch.Tensor] = [out[r:r + m].clone() for r, m in zip(row0, n_out)]
    if not return_counts:
        return pts
    return pts, [out_cnt[r:r + m].clone() for r, m in zip(row0, n_out)]


def voxel_down_sample(points: torch.Tensor, voxel: float) -> torch.Tensor:
    """[N,3] fp32 on the GPU -> [M,3]: the centroid of the points of every occupied voxel, rows in ascending (i, j, k)."""
    return voxel_down_sample_batch([points], voxel)[0]
