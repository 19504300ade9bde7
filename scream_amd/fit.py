"""The training loops of the reference's three drivers (train_3d_match.py:156-233, train_kitti.py:138-233, train_open_gf.py:79-146)
on the packed path: batch preparation on the GPU (scream_amd/prep.py), forward_packed_train, the packed L1 loss, the HIP backward
and one optimiser step (scream_amd/optim.py), with nothing read back inside an epoch.

    opt = FusedAdam(net.parameters(), lr=2e-4)
    prepare_train, prepare_val = pair_preparer("3dmatch", True, dev), pair_preparer("3dmatch", False, dev)
    fit(net, opt, train_loader, val_loader, prepare_train, prepare_val, epochs=45, save_path="params/point-generator.pth")

A loader yields batches (lists of raw items, ``collate_fn=list``); ``prepare(batch)`` turns one into what the step consumes: a
PreparedPairs (PointTransformer: the loss is net.loss_packed(pred, prepared)) or a (PackedBatch, packed target) pair
(DEMTransformer: net.loss_packed(pred, batch, target)).  The per-step losses of an epoch are written into a device vector and
copied to the host once, when the epoch ends; its mean is taken in float64 on the host.  The mean is over steps, as in the
reference (which runs batch_size = 1): with a short last batch it is the mean of the batch means.
"""
from __future__ import annotations

import os
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np
import torch

from .packing import PackedBatch
from .prep import PreparedPairs, prepare_3dmatch_train, prepare_3dmatch_val, prepare_kitti_train, prepare_kitti_val

__all__ = ["lr_after_epoch", "train_epoch", "val_loss", "fit", "pair_preparer", "dem_preparer"]


def lr_after_epoch(lr: float, epoch: int, gamma: float = 0.5, every: int = 15, floor: float = 1e-5) -> float:
    """The reference's update_lr behind its `if epoch % lr_update_epoch == 0` (train_3d_match.py:46-51,232-233; the other two
    drivers are identical): the rate to use after `epoch`."""
    return max(lr * gamma, floor) if epoch % every == 0 else lr


class _LossLog:
    """The per-step losses of an epoch in one device vector; `host()` is the epoch's only copy to the host."""

    def __init__(self, batches):
        self.capacity = len(batches) if hasattr(batches, "__len__") else 64
        self.buf, self.n = None, 0

    def add(self, loss: torch.Tensor) -> None:
        if self.buf is None:
            self.buf = torch.empty(max(self.capacity, 1), device=loss.device, dtype=torch.float32)
        elif self.n == self.buf.shape[0]:
            self.buf = torch.cat([self.buf, torch.empty_like(self.buf)])
        self.buf[self.n].copy_(loss.detach())
        self.n += 1

    def host(self) -> np.ndarray:
        return np.zeros(0, dtype=np.float32) if self.buf is None else self.buf[:self.n].cpu().numpy()


def _mean(losses: np.ndarray) -> float:
    return float(losses.astype(np.float64).mean()) if losses.size else float("nan")


def _loss(net, pred, prepared):
    if isinstance(prepared, PreparedPairs):
        return net.loss_packed(pred, prepared)
    batch, target = prepared
    return net.loss_packed(pred, batch, target)


def _batch_of(prepared) -> PackedBatch:
    return prepared.batch if isinstance(prepared, PreparedPairs) else prepared[0]


def train_epoch(net, opt, batches: Iterable, prepare: Callable, scaler=None) -> Tuple[float, np.ndarray]:
    """One pass over `batches`: prepare, forward_packed_train, loss_packed, zero_grad, backward, step (through `scaler`, a
    torch.amp.GradScaler, when one is given).  Returns (the float64 mean of the per-step losses, the fp32 losses)."""
    net.train()
    log = _LossLog(batches)
    for raw in batches:
        prepared = prepare(raw)
        loss = _loss(net, net.forward_packed_train(_batch_of(prepared)), prepared)
        opt.zero_grad()
        if scaler is None:
            loss.backward()
            opt.step()
        else:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        log.add(loss)
    losses = log.host()
    return _mean(losses), losses


def val_loss(net, batches: Iterable, prepare: Callable) -> Tuple[float, np.ndarray]:
    """The same loss on the inference forward, in eval() under no_grad.  Returns (float64 mean, the fp32 per-batch losses)."""
    net.eval()
    log = _LossLog(batches)
    with torch.no_grad():
        for raw in batches:
            prepared = prepare(raw)
            log.add(_loss(net, net.forward_packed(_batch_of(prepared)), prepared))
    losses = log.host()
    return _mean(losses), losses


def fit(net, opt, train_batches: Iterable, val_batches: Iterable, prepare_train: Callable, prepare_val: Callable, epochs: int,
        save_path: str, scaler=None, gamma: float = 0.5, every: int = 15, floor: float = 1e-5, log: Optional[Callable] = print) -> List[dict]:
    """The reference's train(): for epoch in range(1, epochs) -- as it writes it, epochs - 1 passes -- a training epoch, the
    validation loss, a checkpoint (net.state_dict(), what the reference's models load) whenever that loss improves on the best so
    far, then the learning-rate rule.  Returns one dict per epoch: epoch, train_loss, val_loss, saved, lr (the rate after the
    epoch)."""
    best = 1e8  # train_3d_match.py:157
    history = []
    for epoch in range(1, epochs):
        train_loss, _ = train_epoch(net, opt, train_batches, prepare_train, scaler)
        v, _ = val_loss(net, val_batches, prepare_val)
        saved = v < best
        if saved:
            best = v
            if os.path.dirname(save_path):
                os.makedirs(os.path.dirname(save_path), exist_ok=True)
            torch.save(net.state_dict(), save_path)
        for group in opt.param_groups:
            group["lr"] = lr_after_epoch(group["lr"], epoch, gamma, every, floor)
        history.append(dict(epoch=epoch, train_loss=train_loss, val_loss=v, saved=saved, lr=opt.param_groups[0]["lr"]))
        if log is not None:
            log("epoch: %d  loss: %.5f  val loss: %.5f  lr: %.6f%s" % (epoch, train_loss, v, opt.param_groups[0]["lr"], "  saved" if saved else ""))
    return history


def pair_preparer(kind: str, train: bool, device, seed: int = 0) -> Callable:
    """prepare(batch) for lists of raw (src, tgt, T) items (data.RawPairFiles / data.SyntheticRawPairs): the clouds go to
    `device` and through prepare_3dmatch_* (kind "3dmatch") or prepare_kitti_* (kind "kitti").  Training draws its perturbations
    from one numpy Generator seeded with `seed` and numbers the samples as they come, so no two draws share their noise."""
    if kind not in ("3dmatch", "kitti"):
        raise ValueError("kind must be '3dmatch' or 'kitti', got %r" % (kind,))
    rng = np.random.default_rng(seed)
    seen = [0]

    def prepare(items) -> PreparedPairs:
        srcs = [torch.as_tensor(it[0]).to(device, non_blocking=True) for it in items]
        tgts = [torch.as_tensor(it[1]).to(device, non_blocking=True) for it in items]
        Ts = np.stack([np.asarray(it[2], dtype=np.float64) for it in items])
        if not train:
            return (prepare_3dmatch_val if kind == "3dmatch" else prepare_kitti_val)(srcs, tgts, Ts)
        if kind == "kitti":
            return prepare_kitti_train(srcs, tgts, Ts, rng=rng)
        ids = list(range(seen[0], seen[0] + len(items)))
        seen[0] += len(items)
        return prepare_3dmatch_train(srcs, tgts, Ts, rng=rng, seed=seed, sample_ids=ids)

    return prepare


def dem_preparer(device) -> Callable:
    """prepare(batch) for lists of OpenGF samples (dsm, dem_coarse, dem, ...: evaluate_open_gf.make_sample): DEMTransformer has
    no pose, so the batch is PackedBatch.from_pairs(dsms, dem_coarses, zeros) and the ground truth is the DEMs packed like the
    prediction."""
    def prepare(items):
        dsms = [it[0].to(device, non_blocking=True) for it in items]
        coarse = [it[1].to(device, non_blocking=True) for it in items]
        zero = torch.zeros(3, device=device)
        batch = PackedBatch.from_pairs(dsms, coarse, [zero] * len(items))
        target = torch.zeros(batch.rows_src, 3, device=device)
        for t, it in zip(batch.unpack_src(target), items):
            t.copy_(it[2].to(device, non_blocking=True))
        return batch, target

    return prepare
