"""OpenGF preprocessing on the MI355X (csrc/dsm.hip): from a window of a raw tile to the [n,6] sample DEMTransformer reads.

    dsm = extract_dsm(patch, dem)                                  # [M,3], [N,3] fp32 on the GPU -> [N,3]
    dsm, idx = extract_dsm(patch, dem, return_index=True)          # idx int32 [N]: the chosen patch row, or -1
    dsm_dem, centre = make_dsm_dem(window_xyz, window_cls)         # raw window -> ([n,6] fp32, [1,3] fp32)
    xr, yr = tile_windows("train")                                 # the window ranges of the three splits

The rules are the reference's ``split_dataset_as_patch`` (process_open_gf.py:193-263): window and ground points down-sampled
at 1 m, for every ground point the highest window point within 0.8 m in the xy plane (the point itself when there is none),
both centred on the middle of their common bounding box.  The cylinder search is exact (include/scream_hip.h states the
contract; tests/dsm_ref.py restates it); the result is a pure function of the cloud.  There is no CPU path.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .clouds import PackedPairs, check_clouds, check_radius
from .voxel import voxel_down_sample_batch

__all__ = ["extract_dsm", "extract_dsm_batch", "make_dsm_dem", "make_dsm_dem_batch", "tile_windows", "window_mask"]


def extract_dsm_batch(patches: Sequence[torch.Tensor], dems: Sequence[torch.Tensor], radius: float = 0.8, return_index: bool = False):
    """For every pair (patch [M_i,3], dem [N_i,3]; fp32 on the GPU, M_i, N_i >= 0): the [N_i,3] DSM rows of the dem rows -- per
    ground point the highest patch point within `radius` in the xy plane (equal heights: the lowest patch row), the ground point
    itself when there is none.  With return_index also the int32 [N_i] patch rows (-1: none).  The clouds are packed and share
    every launch; nothing is copied back to the host."""
    patches, dems = list(patches), list(dems)
    if len(patches) != len(dems):
        raise _lib.ScreamHipError("%d patches for %d dems" % (len(patches), len(dems)))
    check_clouds(patches, "patch", op="extract_dsm")
    check_clouds(dems, "dem", op="extract_dsm")
    radius = check_radius(radius, "extract_dsm: the radius")
    if not patches:
        return ([], []) if return_index else []
    pk = PackedPairs(patches, dems, dems[0].device)
    out, idx = _extract(pk, radius)
    return (pk.split_tgt(out), pk.split_tgt(idx)) if return_index else pk.split_tgt(out)


def _extract(pk: PackedPairs, radius: float):
    """The packed call: the patches are the pairs' sources, the dems their targets."""
    m = pk.meta
    return ops.dsm_extract_packed(pk.src, m[0], m[1], pk.max_s_len, pk.tgt, m[2], m[3], pk.max_t_len, radius)


def extract_dsm(patch: torch.Tensor, dem: torch.Tensor, radius: float = 0.8, return_index: bool = False):
    """[M,3], [N,3] fp32 on the GPU -> [N,3] (and the int32 [N] patch rows with return_index): see extract_dsm_batch."""
    r = extract_dsm_batch([patch], [dem], radius, return_index)
    return (r[0][0], r[1][0]) if return_index else r[0]


def _to_device_f32(xyz, origin, dev) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(xyz) if not isinstance(xyz, torch.Tensor) else xyz).to(dev)
    if origin is not None:
        x = x.double() - torch.as_tensor(np.asarray(origin, dtype=np.float64)).to(dev).reshape(1, 3)
    return x.float().contiguous()


def make_dsm_dem_batch(patches_raw: Sequence, classes: Sequence, resolution: float = 1.0, radius: float = 0.8, ground_class: int = 1,
                       origin=None) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """A list of raw windows (xyz [N_i,3], class [N_i]; numpy arrays or tensors on any device) -> (list of [n_i,6] fp32 samples,
    list of [1,3] fp32 centres), on the current GPU: one batched call of each kernel for the whole list.

    Per window: the ground points are those with class == ground_class; window and ground are down-sampled at `resolution`
    (voxel_down_sample_batch: all 2 B clouds in one call), every ground voxel gets its DSM row (the packed scream_dsm_extract), and both are
    centred on float32(min + max) / 2 of their common bounding box: row = dsm - centre | dem - centre.
    `origin` (float64 [3]) is subtracted in float64 before the cast to fp32 -- UTM-sized coordinates have an fp32 spacing of
    3 cm; None casts the coordinates as they are, as the reference does.

    Known difference from the reference: it averages the points of a voxel in float64 and then rounds to fp32 (torch.Tensor of
    open3d's float64 centroids); here the coordinates are rounded to fp32 first and then averaged in float64 -- half an fp32
    ulp per point.  coarse_dems (evaluate_open_gf.py) documents the same caveat.  Parity with open3d itself is not pinned."""
    patches_raw, classes = list(patches_raw), list(classes)
    if len(patches_raw) != len(classes):
        raise _lib.ScreamHipError("%d windows for %d class arrays" % (len(patches_raw), len(classes)))
    radius = check_radius(radius, "make_dsm_dem: the radius")
    B = len(patches_raw)
    if B == 0:
        return [], []
    dev = torch.device("cuda", torch.cuda.current_device())
    clouds = []
    for xyz, cls in zip(patches_raw, classes):
        w = _to_device_f32(xyz, origin, dev)
        c = torch.as_tensor(np.asarray(cls) if not isinstance(cls, torch.Tensor) else cls).to(dev).reshape(-1)
        if w.dim() != 2 or w.shape[1] != 3 or c.shape[0] != w.shape[0]:
            raise _lib.ScreamHipError("expected xyz [N,3] and class [N], got %s and %s" % (tuple(w.shape), tuple(c.shape)))
        clouds.append((w, w[c == ground_class]))
    down = voxel_down_sample_batch([w for w, _ in clouds] + [g for _, g in clouds], float(resolution))
    pk = PackedPairs(down[:B], down[B:], dev)
    dsm, _ = _extract(pk, radius)
    out, centre = ops.dsm_dem_assemble_packed(dsm, pk.tgt, pk.meta[2], pk.meta[3], pk.max_t_len)
    return pk.split_tgt(out), [centre[i:i + 1].clone() for i in range(B)]


def make_dsm_dem(patch_raw, cls, resolution: float = 1.0, radius: float = 0.8, ground_class: int = 1,
                 origin=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One raw window -> (dsm_dem [n,6] fp32, centre [1,3] fp32) on the GPU: see make_dsm_dem_batch."""
    out, centre = make_dsm_dem_batch([patch_raw], [cls], resolution, radius, ground_class, origin)
    return out[0], centre[0]


def tile_windows(kind: str) -> Tuple[List[List[int]], List[List[int]]]:
    """(x ranges, y ranges) of the windows a tile of the split is cut into, [lo, hi] in metres from the tile's minimum corner:
    "train" 17 x 17 windows of 100 m every 25 m, "val" 5 x 5 side by side, "test" 26 x 25 side by side.  Window i of a tile is
    x range i % len(x ranges), y range i // len(x ranges)."""
    if kind == "train":
        r = [[lo, lo + 100] for lo in range(0, 401, 25)]
        return r, [list(w) for w in r]
    if kind == "val":
        r = [[lo, lo + 100] for lo in range(0, 500, 100)]
        return r, [list(w) for w in r]
    if kind == "test":
        return [[lo, lo + 100] for lo in range(0, 2600, 100)], [[lo, lo + 100] for lo in range(0, 2500, 100)]
    raise ValueError("tile_windows: kind must be 'train', 'val' or 'test', got %r" % (kind,))


def window_mask(xyz: torch.Tensor, coor_min: torch.Tensor, x: Sequence[int], y: Sequence[int]) -> torch.Tensor:
    """Rows of xyz ([N,>=2], on the device) inside window x = [lo, hi], y = [lo, hi]: (shift >= lo) & (shift < hi) per axis with
    shift = xyz - coor_min, evaluated in float64."""
    shift = xyz[:, :2].double() - coor_min.double().reshape(-1)[:2].to(xyz.device)
    return (shift[:, 0] >= x[0]) & (shift[:, 0] < x[1]) & (shift[:, 1] >= y[0]) & (shift[:, 1] < y[1])
