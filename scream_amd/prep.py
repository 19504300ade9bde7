"""Training batches on the MI355X (csrc/prep.hip): augmentation, normalisation and packing of B pairs in one call, and the L1
loss of a packed prediction with its gradient.

    perturb, side = sample_perturbations(B, 0.1, rng)                           # host, numpy: B small SE(3) matrices
    prep = prepare_3dmatch_train(srcs, tgts, Ts, rng=rng, seed=epoch, sample_ids=ids)    # everything stays on the device
    pred = net.forward_packed_train(prep.batch)
    loss = net.loss_packed(pred, prep)                                          # one scalar with a grad_fn
    loss.backward()

The rules are the reference's: ``augment`` (datasets/three_d_match.py:129-153, datasets/kitti.py:233-265: a small SE(3)
perturbation about the centroid of the perturbed cloud, then 3 mm Gaussian noise on 3DMatch), the unit-ball / bounding-box
normalisation behind it (three_d_match.py:183-190, kitti.py:268-273) and the L1 point loss (models/pointnet.py:93-99, 163-167).
The arithmetic is the float64 contract of include/scream_hip.h, restated in numpy by tests/prep_ref.py.  The reference draws
from numpy's global stream; here the perturbations come from a seeded Generator and the noise from Philox4x32-10 keyed by
(seed, sample_id): the same distribution, not the same bits, and a sample's noise does not depend on what else is in its batch.
There is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .clouds import check_clouds, pose_stack
from .packing import PackedBatch

__all__ = ["sample_perturbations", "prepare_pairs", "PreparedPairs", "prepare_3dmatch_train", "prepare_3dmatch_val",
           "prepare_kitti_train", "prepare_kitti_val", "packed_l1_loss"]

MODES = {"ball": 0, "bbox": 1}
CENTER_RULES = {"mean": 0, "trans": 1, "neg_rt_trans": 2}


def sample_perturbations(B: int, std: float = 0.1, rng=None, side: str = "random") -> Tuple[np.ndarray, np.ndarray]:
    """B small rigid perturbations and the cloud each one moves: (perturb float64 [B,4,4], side int32 [B]; 0 source, 1 target).
    What the reference's SE3.sample_small(std) draws (lie/numpy/so3.py:31-38, se3.py:38-44, so3_common.py:185-210), written
    out: the axis uniform on the sphere (azimuth U(0, 2 pi), cos of the polar angle U(-1, 1)), the angle N(0, 1) std pi / sqrt 3,
    the rotation by Rodrigues' formula I + sin(angle) K + (1 - cos(angle)) K^2, the translation N(0, 1) std / sqrt 3 per axis.
    side "random": source or target with equal odds (three_d_match.py:131); "source": always the source (kitti.py:235).
    rng: a numpy Generator or a seed."""
    if side not in ("random", "source"):
        raise ValueError("side must be 'random' or 'source', got %r" % (side,))
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    B = int(B)
    phi = rng.uniform(0.0, 2.0 * math.pi, size=B)
    cos_t = rng.uniform(-1.0, 1.0, size=B)
    sin_t = np.sqrt(1.0 - cos_t * cos_t)
    axis = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], axis=1)
    angle = rng.standard_normal(B) * (std * math.pi / math.sqrt(3.0))
    trans = rng.standard_normal((B, 3)) * (std / math.sqrt(3.0))
    K = np.zeros((B, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    P = np.zeros((B, 4, 4))
    P[:, :3, :3] = np.eye(3)[None] + np.sin(angle)[:, None, None] * K + (1.0 - np.cos(angle))[:, None, None] * (K @ K)
    P[:, :3, 3] = trans
    P[:, 3, 3] = 1.0
    which = (rng.random(B) <= 0.5).astype(np.int32) if side == "random" else np.zeros(B, dtype=np.int32)
    return P, which


@dataclass
class PreparedPairs:
    """A training batch on the device: the packed clouds and the ground truth in their normalised frame."""
    batch: PackedBatch
    rot: torch.Tensor     # fp32 [B,3,3]
    trans: torch.Tensor   # fp32 [B,3,1]
    s: torch.Tensor       # float64 [B]      normalised = s * (metric - c)
    c: torch.Tensor       # float64 [B,3]
    T_aug: torch.Tensor   # float64 [B,4,4]  registers the augmented metric source onto the augmented metric target


def prepare_pairs(srcs: Sequence[torch.Tensor], tgts: Sequence[torch.Tensor], T, *, mode: str, center: str, perturb=None, side=None,
                  noise_std: float = 0.0, seed: int = 0, sample_ids=None) -> PreparedPairs:
    """B raw pairs (srcs[i] [N_i,3], tgts[i] [M_i,3] on the GPU, all float32 or all float64, metric frame; T the float64 4x4
    transforms that register each source onto its target: [B,4,4] numpy, a sequence, or a tensor, which may be on the device)
    -> one PreparedPairs.
      mode      "ball" (3DMatch) | "bbox" (KITTI): the normalisation
      center    the source centre the embedding subtracts: "mean" (of the normalised source), "trans" (train_3d_match.py:172)
                or "neg_rt_trans" (-R^T trans, train_kitti.py:156)
      perturb   float64 [B,4,4] (sample_perturbations), None: none;  side int [B]: 0 moves the source, 1 the target
      noise_std metric Gaussian noise on both clouds, from (seed, sample_ids[i], cloud, row); sample_ids default to 0 .. B - 1
    Lengths come from the tensor shapes: four small uploads (the integers, the ids, T, perturb), nothing is copied to the host
    and nothing synchronises."""
    srcs, tgts = list(srcs), list(tgts)
    B = len(srcs)
    if B == 0 or len(tgts) != B:
        raise _lib.ScreamHipError("prepare_pairs: %d sources for %d targets" % (B, len(tgts)))
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    if center not in CENTER_RULES:
        raise ValueError("center must be one of %s, got %r" % (sorted(CENTER_RULES), center))
    clouds = srcs + tgts
    check_clouds(clouds, "cloud", (torch.float32, torch.float64), op="batch preparation")
    dev = clouds[0].device
    src_len, tgt_len = [int(t.shape[0]) for t in srcs], [int(t.shape[0]) for t in tgts]
    lens, row0, rows_src, rows_total, tile_cloud, max_chunks = PackedBatch.layout(src_len, tgt_len)
    raw_row0 = np.concatenate([[0], np.cumsum(lens.astype(np.int64))[:-1]])
    if int(lens.astype(np.int64).sum()) >= 2 ** 31:
        raise ValueError("batch too large for int32 row indices")
    Tm = pose_stack(T, B, dev, "T").reshape(-1)
    Pm = pose_stack(np.broadcast_to(np.eye(4), (B, 4, 4)) if perturb is None else perturb, B, dev, "perturb").reshape(-1)
    sd = np.zeros(B, dtype=np.int64) if side is None else np.asarray(side, dtype=np.int64).reshape(-1)
    ids = np.arange(B, dtype=np.int64) if sample_ids is None else np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    if sd.shape[0] != B or ids.shape[0] != B:
        raise _lib.ScreamHipError("prepare_pairs: side / sample_ids must have one entry per pair")
    # one upload for the integers (raw_row0 | cloud_row0 | cloud_len | side | tile_cloud), one for the ids, one per matrix set
    i32 = torch.from_numpy(np.concatenate([raw_row0, row0, lens, sd, tile_cloud]).astype(np.int32)).to(dev)
    ids_d = torch.from_numpy(ids).to(dev)
    raw = torch.cat(clouds, dim=0).contiguous()
    raw_row0_d, cloud_row0, cloud_len, side_d = i32[:2 * B], i32[2 * B:4 * B], i32[4 * B:6 * B], i32[6 * B:7 * B]
    xyz, cen, rot, trans, s, c, T_aug = ops.prep_pairs_packed(raw, raw_row0_d, cloud_len, int(lens.max()), Tm, Pm, side_d, noise_std, seed,
                                                              ids_d, MODES[mode], CENTER_RULES[center], cloud_row0, rows_total)
    batch = PackedBatch(B, src_len, tgt_len, row0, lens, rows_src, rows_total, max_chunks, xyz, cen, i32[7 * B:], cloud_row0, cloud_len)
    return PreparedPairs(batch, rot, trans, s, c, T_aug)


def prepare_3dmatch_train(srcs, tgts, T, *, rng=None, seed: int = 0, sample_ids=None, std: float = 0.1,
                          noise_std: float = 0.003) -> PreparedPairs:
    """ThreeDMatchTrain.__getitem__ (three_d_match.py:175-192) for a batch: a perturbation of a random side, 3 mm noise, the unit
    ball, and the centre train_3d_match.py:172 passes (trans)."""
    perturb, side = sample_perturbations(len(srcs), std, rng, "random")
    return prepare_pairs(srcs, tgts, T, mode="ball", center="trans", perturb=perturb, side=side, noise_std=noise_std, seed=seed,
                         sample_ids=sample_ids)


def prepare_3dmatch_val(srcs, tgts, T) -> PreparedPairs:
    """ThreeDMatchVal.__getitem__: the unit ball, no augmentation."""
    return prepare_pairs(srcs, tgts, T, mode="ball", center="trans")


def prepare_kitti_train(srcs, tgts, T, *, rng=None, std: float = 0.1) -> PreparedPairs:
    """KITTI_Train.__getitem__ (kitti.py:233-265, 340-346): the source perturbed, no noise, the bounding box, and the centre
    train_kitti.py:156 passes (-R^T trans)."""
    perturb, side = sample_perturbations(len(srcs), std, rng, "source")
    return prepare_pairs(srcs, tgts, T, mode="bbox", center="neg_rt_trans", perturb=perturb, side=side)


def prepare_kitti_val(srcs, tgts, T) -> PreparedPairs:
    """KITTI_Val.__getitem__: the bounding box, no augmentation."""
    return prepare_pairs(srcs, tgts, T, mode="bbox", center="neg_rt_trans")


class _PackedL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, batch, xyz, rot, trans, target):
        pred = pred.contiguous()
        max_len = max(batch.src_len)
        loss, loss_pair = ops.l1_pairs_fwd(pred, xyz, rot, trans, target, batch.cloud_row0, batch.cloud_len, batch.n_pairs, max_len)
        ctx.batch, ctx.max_len = batch, max_len
        ctx.save_for_backward(pred, *(t for t in (xyz, rot, trans, target) if t is not None))
        ctx.has_target = target is not None
        ctx.mark_non_differentiable(loss_pair)
        return loss, loss_pair

    @staticmethod
    def backward(ctx, dout, _dpair):
        saved = ctx.saved_tensors
        pred = saved[0]
        xyz, rot, trans, target = (None, None, None, saved[1]) if ctx.has_target else (saved[1], saved[2], saved[3], None)
        b = ctx.batch
        dpred = ops.l1_pairs_bwd(dout.to(torch.float32).contiguous(), pred, xyz, rot, trans, target, b.cloud_row0, b.cloud_len, b.n_pairs,
                                 ctx.max_len)
        return dpred, None, None, None, None, None


def packed_l1_loss(pred: torch.Tensor, prepared, target: Optional[torch.Tensor] = None, return_pairs: bool = False):
    """The reference's L1 loss of a packed prediction [rows_src,3] (forward_packed_train's), one launch pair forward and one
    backward for the whole batch:
        packed_l1_loss(pred, prepared)               mean_p mean_i sum_k |pred - (rot_p x + trans_p)|      (pointnet.py:93-99)
        packed_l1_loss(pred, batch, target=packed)   the same against a packed [rows_src,3] target        (pointnet.py:163-167)
    Sums in float64 in a fixed order (include/scream_hip.h); the fp32 scalar carries a grad_fn when `pred` does.
    return_pairs: also the float64 [B] per-pair losses (no gradient)."""
    if isinstance(prepared, PreparedPairs):
        batch = prepared.batch
        args = (None, None, None, target) if target is not None else (batch.xyz, prepared.rot, prepared.trans, None)
    elif isinstance(prepared, PackedBatch):
        if target is None:
            raise _lib.ScreamHipError("packed_l1_loss(pred, batch) needs target=: a PackedBatch carries no ground truth")
        batch, args = prepared, (None, None, None, target)
    else:
        raise TypeError("expected a PreparedPairs or a PackedBatch, got %s" % type(prepared).__name__)
    if tuple(pred.shape) != (batch.rows_src, 3):
        raise _lib.ScreamHipError("the packed prediction is [%d,3], got %s" % (batch.rows_src, tuple(pred.shape)))
    if args[3] is not None:
        args = (None, None, None, args[3].detach().to(torch.float32).contiguous())
    loss, loss_pair = _PackedL1.apply(pred, batch, *args)
    return (loss, loss_pair) if return_pairs else loss
