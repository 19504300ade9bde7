"""3DMatch pair preparation on the MI355X (csrc/radius.hip): the overlap of a pair and everything process_3d_match.py derives
from it.

    counts = radius_count_batch(srcs, tgts, Ts, 0.03)                   # int32 [N_i]: target points within 0.03 m of T src_i
    pairs = radius_pairs_batch(srcs, tgts, Ts, 0.03, K=None)            # int64 [n_i,2]: (i, j), i ascending, then (d2, j)
    masks, n_overlap = overlap_batch(srcs, tgts, Ts)                    # bool [N_i], Python ints
    items = prepare_3dmatch_batch(srcs, tgts, rots, transs)             # src / tgt / src_zero down-sampled, T, overlap_ratio
    select_outputs("test_3dlomatch", n_overlap, n_src)                  # [("3DLoMatch_test", "src"), ("3DZeroMatch_test", "src_zero")]

The rules are the reference's: ``utils.get_correspondences`` (utils.py:94-108) as ``ThreeDMatchDataset_PREDATOR`` calls it at
0.03 m (datasets/three_d_match.py:106-113), and the ratio tests of process_3d_match.py.  The search is exact under the
contract of include/scream_hip.h (float64 transform and distance, j a neighbour of i iff d2 < radius^2, STRICT; neighbours in
ascending (d2, j), equal distances to the lowest target row -- that tie rule is ours); tests/radius_ref.py restates it.  Parity
with open3d's KD-tree itself is not pinned (it is not installed here): the two rules can differ only for points exactly at
the radius.  There is no CPU path.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .clouds import PackedPairs, check_clouds, check_radius, pose_stack
from .voxel import voxel_down_sample_batch

__all__ = ["radius_count_batch", "radius_pairs_batch", "overlap_batch", "prepare_3dmatch_batch", "select_outputs",
           "get_correspondences"]

SETS = {"train": "3DMatch_train", "val": "3DMatch_val", "test_3dmatch": "3DMatch_test", "test_3dlomatch": "3DLoMatch_test"}
ZERO_SET = "3DZeroMatch_test"


class _RadiusCall(PackedPairs):
    """A call's checked clouds packed, with its transforms and radius, as scream_radius_count / _pairs read them."""

    def __init__(self, srcs, tgts, Ts, radius):
        srcs, tgts = list(srcs), list(tgts)
        if len(srcs) != len(tgts):
            raise _lib.ScreamHipError("%d sources for %d targets" % (len(srcs), len(tgts)))
        check_clouds(srcs, "source", op="the radius search")
        check_clouds(tgts, "target", op="the radius search")
        self.radius = check_radius(radius)
        self.B = len(srcs)
        if not self.B:
            return
        super().__init__(srcs, tgts, srcs[0].device)
        self.T = pose_stack(Ts, self.B, self.dev)

    def args(self):
        m = self.meta
        return (self.src, m[0], m[1], self.max_s_len, self.tgt, m[2], m[3], self.max_t_len, self.T, self.radius)

    def count(self):
        return ops.radius_count_packed(*self.args())

    def bounds(self) -> torch.Tensor:
        """int64 [B + 1] on the device: the first source row of every pair, and the total."""
        return torch.tensor(self.s_row0 + [self.s_rows], dtype=torch.int64).to(self.dev)


def radius_count_batch(srcs: Sequence[torch.Tensor], tgts: Sequence[torch.Tensor], Ts, radius: float) -> List[torch.Tensor]:
    """For every pair (src [N_i,3], tgt [M_i,3]; fp32 on the GPU, N_i, M_i >= 0; T_i a float64 4x4, numpy or tensor): the int32
    [N_i] number of target points within `radius` of every transformed source point.  The pairs are packed and share every
    launch; nothing is copied back to the host."""
    pk = _RadiusCall(srcs, tgts, Ts, radius)
    if not pk.B:
        return []
    count, _ = pk.count()
    return pk.split_src(count)


def radius_pairs_batch(srcs: Sequence[torch.Tensor], tgts: Sequence[torch.Tensor], Ts, radius: float,
                       K: Optional[int] = None) -> List[torch.Tensor]:
    """For every pair the int64 [n_i,2] rows (i, j): target point j lies within `radius` of transformed source point i.  Rows in
    ascending i, the neighbours of one i in ascending (d2, j) -- nearest first, equal distances to the lowest j -- and at most K
    of them (None: all).  One count launch, a prefix sum, ONE host read (the per-pair totals) and the fill launch."""
    pk = _RadiusCall(srcs, tgts, Ts, radius)
    if K is not None and int(K) < 1:
        raise _lib.ScreamHipError("K must be None or at least 1, got %r" % (K,))
    if not pk.B:
        return []
    count, workspace = pk.count()
    kept = count.to(torch.int64) if K is None else count.to(torch.int64).clamp(max=int(K))
    offset = torch.zeros(count.shape[0] + 1, device=pk.dev, dtype=torch.int64)
    torch.cumsum(kept, dim=0, out=offset[1:])
    ends = offset[pk.bounds()].cpu().tolist()  # the one synchronising copy
    total = ends[-1]
    pair_j = ops.radius_pairs_packed(*pk.args(), workspace, 0 if K is None else int(K), offset, total)
    rows = torch.repeat_interleave(torch.arange(count.shape[0], device=pk.dev, dtype=torch.int64), kept, output_size=total)
    out = []
    for p in range(pk.B):
        a, b = ends[p], ends[p + 1]
        out.append(torch.stack([rows[a:b] - pk.s_row0[p], pair_j[a:b].to(torch.int64)], dim=1))
    return out


def get_correspondences(src_pcd, tgt_pcd, trans, search_voxel_size: float, K: Optional[int] = None) -> torch.Tensor:
    """The reference's utils.get_correspondences (utils.py:94-108) with [N,3] tensors or arrays in place of open3d clouds (taken
    as fp32, moved to the GPU if they are not there): a LongTensor [n,2] of (i, j), target point j within `search_voxel_size` of
    source point i transformed by the 4x4 `trans`.  Rows in ascending i; the neighbours of one i nearest first, equal distances
    to the lowest j, at most K of them.  Membership is d2 < radius^2 in float64 (strict).  Parity with open3d's KD-tree is not
    pinned: it can differ only for points exactly at the radius, and in the order of equally distant neighbours."""
    dev = torch.device("cuda", torch.cuda.current_device())
    cloud = lambda a: torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(device=dev, dtype=torch.float32).contiguous()
    return radius_pairs_batch([cloud(src_pcd)], [cloud(tgt_pcd)], [trans], search_voxel_size, K)[0]


def overlap_batch(srcs: Sequence[torch.Tensor], tgts: Sequence[torch.Tensor], Ts, radius: float = 0.03) -> Tuple[List[torch.Tensor], List[int]]:
    """(masks, n_overlap): per pair the boolean [N_i] mask of the source points that have a target point within `radius` once
    transformed -- the set ``src_overlap_ind`` of datasets/three_d_match.py:113 -- and its size as a Python int (one host copy
    per batch)."""
    pk = _RadiusCall(srcs, tgts, Ts, radius)
    if not pk.B:
        return [], []
    count, _ = pk.count()
    mask = count > 0
    run = torch.zeros(count.shape[0] + 1, device=pk.dev, dtype=torch.int64)
    torch.cumsum(mask.to(torch.int64), dim=0, out=run[1:])
    ends = run[pk.bounds()].cpu().tolist()
    return pk.split_src(mask), [ends[p + 1] - ends[p] for p in range(pk.B)]


def _f32(a) -> np.ndarray:
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float32)


def prepare_3dmatch_batch(srcs: Sequence[torch.Tensor], tgts: Sequence[torch.Tensor], rots: Sequence, transs: Sequence,
                          overlap_radius: float = 0.03, voxel: float = 0.0625) -> List[Dict]:
    """What process_3d_match.py computes for every pair before it saves (lines 13-32), for a batch: one dict per pair with
      T              float64 4x4 numpy, built as line 18 does from the float32 rot [3,3] | trans [3] or [3,1]
      n_overlap      source points with a target point within `overlap_radius` of T src (overlap_batch), n_src their number
      overlap_ratio  n_overlap / n_src, a Python division of two ints: exactly the reference's value, so its comparisons with
                     0.3 and 0.1 are the reference's
      src, tgt       the clouds down-sampled at `voxel`;  src_zero  src[~mask] (order preserving, as np.setdiff1d is) down-sampled
    The clouds are fp32 [N,3] on the GPU and stay there; the 3 B clouds are down-sampled in ONE voxel_down_sample_batch call.
    An empty source raises ScreamHipError (the reference divides by zero).

    Known difference from the reference: it averages the points of a voxel in float64 from float64 copies of the fp32 points
    and keeps float64; here the fp32 points are averaged in float64 and the mean is rounded once to fp32 -- half an fp32 ulp
    per coordinate.  make_dsm_dem_batch documents the same caveat.  Parity with open3d itself is not pinned."""
    srcs, tgts, rots, transs = list(srcs), list(tgts), list(rots), list(transs)
    B = len(srcs)
    if not (len(tgts) == len(rots) == len(transs) == B):
        raise _lib.ScreamHipError("%d sources, %d targets, %d rotations, %d translations" % (B, len(tgts), len(rots), len(transs)))
    for i, s in enumerate(srcs):
        if isinstance(s, torch.Tensor) and s.dim() == 2 and s.shape[0] == 0:
            raise _lib.ScreamHipError("pair %d: the source cloud is empty, its overlap ratio is undefined" % i)
    Ts = []
    for rot, trans in zip(rots, transs):
        rot, trans = _f32(rot).reshape(3, 3), _f32(trans).reshape(3, 1)
        Ts.append(np.concatenate([np.concatenate([rot, trans], axis=1), np.array([[0, 0, 0, 1]])], axis=0))
    masks, n_overlap = overlap_batch(srcs, tgts, Ts, overlap_radius)
    if B == 0:
        return []
    down = voxel_down_sample_batch(srcs + tgts + [s[~m] for s, m in zip(srcs, masks)], float(voxel))
    out = []
    for p in range(B):
        n_src = int(srcs[p].shape[0])
        out.append(dict(src=down[p], tgt=down[B + p], src_zero=down[2 * B + p], T=Ts[p], n_overlap=n_overlap[p], n_src=n_src,
                        overlap_ratio=n_overlap[p] / n_src))
    return out


def select_outputs(kind: str, n_overlap: int, n_src: int) -> List[Tuple[str, str]]:
    """Which split folders a pair is written to, and with which source cloud, by the reference's rules (process_3d_match.py:43,
    87, 125, 166, 173): a list of (folder, "src" | "src_zero") in the order the reference writes them.
      "train", "val"     the full pair always; the zero-overlap pair as well when ratio <= 0.3
      "test_3dmatch"     the full pair when ratio > 0.3
      "test_3dlomatch"   3DLoMatch_test with the full pair when ratio > 0.1; 3DZeroMatch_test with src_zero when ratio <= 0.3
    ratio = n_overlap / n_src, the Python division of the reference.  A pure host function."""
    if kind not in SETS:
        raise ValueError("select_outputs: kind must be one of %s, got %r" % (sorted(SETS), kind))
    if n_src <= 0:
        raise ValueError("select_outputs: an empty source has no overlap ratio")
    ratio = n_overlap / n_src
    folder = SETS[kind]
    if kind in ("train", "val"):
        return [(folder, "src")] + ([(folder, "src_zero")] if ratio <= 0.3 else [])
    if kind == "test_3dmatch":
        return [(folder, "src")] if ratio > 0.3 else []
    return ([(folder, "src")] if 0.1 < ratio else []) + ([(ZERO_SET, "src_zero")] if ratio <= 0.3 else [])
