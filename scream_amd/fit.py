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

The reference's use_GAN = True is fit(..., gan=GanTraining(AdversarialLoss().to(dev), opt_d, pair_real_rows)): train_epoch_gan adds
the rendered images, the HIP discriminator of scream_amd/gan.py and its own optimiser step to every step, still with nothing read
back inside an epoch.

Driver is the text the three root scripts have in common (update_lr, the loaders, the body of train(), the GAN set-up, the command
line); each script hands it what differs: its model, data sets, preparers and real_rows.
"""
from __future__ import annotations

import argparse
import os
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import ops
from .packing import PackedBatch
from .prep import PreparedPairs, prepare_3dmatch_train, prepare_3dmatch_val, prepare_kitti_train, prepare_kitti_val
from .render import render_packed_train

__all__ = ["lr_after_epoch", "train_epoch", "train_epoch_gan", "val_loss", "fit", "pair_preparer", "dem_preparer", "render_rows",
           "pair_real_rows", "dem_real_rows", "GanTraining", "gan_training", "Driver"]


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


def _point_loss(net, pred, prepared, chamfer_weight: float, chamfer_rows: Optional[Callable]):
    """The point loss of a step: loss_packed, plus chamfer_weight times the Chamfer distance of the prediction against
    chamfer_rows(prepared) when the weight is positive (with weight 0 nothing of it is entered)."""
    loss = _loss(net, pred, prepared)
    if chamfer_weight > 0:
        if chamfer_rows is None:
            raise ValueError("chamfer_weight > 0 needs chamfer_rows (pair_real_rows or dem_real_rows)")
        loss = loss + chamfer_weight * net.chamfer_packed_loss(pred, _batch_of(prepared), chamfer_rows(prepared))
    return loss


def _step(loss, opt, scaler):
    """zero_grad, backward, step; through `scaler` (scale, step, update) when one is given."""
    opt.zero_grad()
    if scaler is None:
        loss.backward()
        opt.step()
    else:
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()


def train_epoch(net, opt, batches: Iterable, prepare: Callable, scaler=None, chamfer_weight: float = 0.0,
                chamfer_rows: Optional[Callable] = None) -> Tuple[float, np.ndarray]:
    """One pass over `batches`: prepare, forward_packed_train, loss_packed, zero_grad, backward, step (through `scaler`, a
    torch.amp.GradScaler, when one is given).  chamfer_weight > 0: the loss of a step is loss_packed + chamfer_weight *
    net.chamfer_packed_loss(pred, batch, chamfer_rows(prepared)), chamfer_rows being pair_real_rows or dem_real_rows (or any
    packed [rows_src,3] ground truth, row-paired or not).  Returns (the float64 mean of the per-step losses, the fp32 losses)."""
    net.train()
    log = _LossLog(batches)
    for raw in batches:
        prepared = prepare(raw)
        loss = _point_loss(net, net.forward_packed_train(_batch_of(prepared)), prepared, chamfer_weight, chamfer_rows)
        _step(loss, opt, scaler)
        log.add(loss)
    losses = log.host()
    return _mean(losses), losses


def val_loss(net, batches: Iterable, prepare: Callable, chamfer_weight: float = 0.0,
             chamfer_rows: Optional[Callable] = None) -> Tuple[float, np.ndarray]:
    """The same loss (train_epoch's, chamfer_weight included) on the inference forward, in eval() under no_grad.  Returns
    (float64 mean, the fp32 per-batch losses)."""
    net.eval()
    log = _LossLog(batches)
    with torch.no_grad():
        for raw in batches:
            prepared = prepare(raw)
            log.add(_point_loss(net, net.forward_packed(_batch_of(prepared)), prepared, chamfer_weight, chamfer_rows))
    losses = log.host()
    return _mean(losses), losses


def render_rows(net, rows: torch.Tensor, prepared) -> torch.Tensor:
    """The depth images of the packed source rows `rows` [rows_src,3] against the batch's target clouds, through net.generator's
    views: [B*V, 2, w, w], with a grad_fn into `rows` when they carry one (pointnet.py:62-65 for every pair of the batch)."""
    batch, gen = _batch_of(prepared), net.generator
    return render_packed_train(rows, batch.src_row0, batch.src_len_dev, batch.xyz, batch.tgt_row0, batch.tgt_len_dev, max(batch.src_len),
                               max(batch.tgt_len), gen.eulers, gen.w, gen.rho, rot=gen.view_matrices(rows.device))


def pair_real_rows(prepared: PreparedPairs) -> torch.Tensor:
    """real_rows of PointTransformer: the ground-truth source R x + t of every pair over the packed rows (train_3d_match.py:198),
    one launch."""
    b = prepared.batch
    return ops.pairs_transform(b.xyz, prepared.rot, prepared.trans, b.tile_cloud, b.n_pairs, b.rows_src)


def dem_real_rows(prepared) -> torch.Tensor:
    """real_rows of DEMTransformer: the packed ground-truth DEM as it is (train_open_gf.py's real = generator(dem, dem_coarse))."""
    return prepared[1]


@dataclass
class GanTraining:
    """What fit(gan=...) needs besides the generator's: the AdversarialLoss, the discriminator's optimiser, real_rows(prepared)
    (pair_real_rows / dem_real_rows), where to save the discriminator (whenever the generator checkpoint is written; None:
    nowhere) and the weight of g_loss (0.1, train_3d_match.py:189)."""
    loss: torch.nn.Module
    opt: torch.optim.Optimizer
    real_rows: Callable
    save_path: Optional[str] = None
    g_weight: float = 0.1


def gan_training(device, real_rows: Callable, lr_d: float = 1e-4, betas=(0.5, 0.999), save_path: Optional[str] = None) -> GanTraining:
    """What the reference's drivers build under use_GAN (train_3d_match.py:24-26,40-41): an AdversarialLoss on `device` and Adam
    at lr_d with betas (0.5, 0.999) over its parameters, here a FusedAdam."""
    from .gan import AdversarialLoss
    from .optim import FusedAdam
    loss = AdversarialLoss().to(device)
    return GanTraining(loss, FusedAdam(loss.parameters(), lr=lr_d, betas=betas), real_rows, save_path)


def train_epoch_gan(net, gan_loss, opt_g, opt_d, batches: Iterable, prepare: Callable, real_rows: Callable, scaler=None,
                    g_weight: float = 0.1, chamfer_weight: float = 0.0, chamfer_rows: Optional[Callable] = None) -> Tuple[float, np.ndarray]:
    """train_epoch with the adversarial loss, in the reference's order (train_3d_match.py:171-205), every step:
      1. forward_packed_train;
      2. the prediction's images through render_rows;
      3. loss = point_loss + g_weight * g_loss (point_loss: train_epoch's, chamfer_weight included), g_loss = gan_loss(imgs, None, 0); opt_g.zero_grad(), backward, opt_g.step();
      4. real = the images of real_rows(prepared), the ground-truth source rows, rendered under no_grad;
      5. d_loss = gan_loss(imgs.detach(), real, 1); opt_d.zero_grad(), backward, opt_d.step().
    With a `scaler` both updates go scale(loss).backward(), step(opt), update(), as train_kitti.py:185-204 writes them.
    With B pairs and V views the discriminator sees B * V images per call and its batch statistics run over all of them: the
    batch form of the reference's loop, which runs batch size 1 (V images per call); at B = 1 the two coincide.
    Returns (the float64 mean of the per-step generator losses -- point_loss + g_weight * g_loss, what the reference reports --
    and the fp32 losses [steps,3]: that loss, g_loss, d_loss), copied to the host once, when the epoch ends."""
    net.train()
    gan_loss.train()
    logs = [_LossLog(batches) for _ in range(3)]
    for raw in batches:
        prepared = prepare(raw)
        pred = net.forward_packed_train(_batch_of(prepared))
        imgs = render_rows(net, pred, prepared)
        g = gan_loss(imgs, None, 0)
        loss = _point_loss(net, pred, prepared, chamfer_weight, chamfer_rows) + g_weight * g
        _step(loss, opt_g, scaler)
        with torch.no_grad():
            real = render_rows(net, real_rows(prepared), prepared)
        d = gan_loss(imgs.detach(), real, 1)
        _step(d, opt_d, scaler)
        for lg, v in zip(logs, (loss, g, d)):
            lg.add(v)
    losses = np.stack([lg.host() for lg in logs], axis=1)
    return _mean(losses[:, 0]), losses


def fit(net, opt, train_batches: Iterable, val_batches: Iterable, prepare_train: Callable, prepare_val: Callable, epochs: int,
        save_path: str, scaler=None, gamma: float = 0.5, every: int = 15, floor: float = 1e-5, log: Optional[Callable] = print,
        gan: Optional[GanTraining] = None, chamfer_weight: float = 0.0, chamfer_rows: Optional[Callable] = None) -> List[dict]:
    """The reference's train(): for epoch in range(1, epochs) -- as it writes it, epochs - 1 passes -- a training epoch, the
    validation loss, a checkpoint (net.state_dict(), what the reference's models load) whenever that loss improves on the best so
    far, then the learning-rate rule.  Returns one dict per epoch: epoch, train_loss, val_loss, saved, lr (the rate after the
    epoch).  gan: a GanTraining turns the epoch into train_epoch_gan (the reference's use_GAN = True); the dicts then also carry
    g_loss and d_loss (epoch means), the discriminator is saved with the generator, and its rate is left alone, as the reference
    only ever updates optimizer_G's.  chamfer_weight / chamfer_rows: train_epoch's, for the training and the validation loss alike."""
    best = 1e8  # train_3d_match.py:157
    history = []
    for epoch in range(1, epochs):
        extra = {}
        if gan is None:
            train_loss, _ = train_epoch(net, opt, train_batches, prepare_train, scaler, chamfer_weight, chamfer_rows)
        else:
            train_loss, steps = train_epoch_gan(net, gan.loss, opt, gan.opt, train_batches, prepare_train, gan.real_rows, scaler, gan.g_weight,
                                                chamfer_weight, chamfer_rows)
            extra = dict(g_loss=_mean(steps[:, 1]), d_loss=_mean(steps[:, 2]))
        v, _ = val_loss(net, val_batches, prepare_val, chamfer_weight, chamfer_rows)
        saved = v < best
        if saved:
            best = v
            for path, module in ((save_path, net),) + (((gan.save_path, gan.loss.discriminator),) if gan is not None and gan.save_path else ()):
                if os.path.dirname(path):
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                torch.save(module.state_dict(), path)
        for group in opt.param_groups:
            group["lr"] = lr_after_epoch(group["lr"], epoch, gamma, every, floor)
        history.append(dict(epoch=epoch, train_loss=train_loss, val_loss=v, saved=saved, lr=opt.param_groups[0]["lr"], **extra))
        if log is not None:
            log("epoch: %d  loss: %.5f  val loss: %.5f  lr: %.6f%s%s" % (epoch, train_loss, v, opt.param_groups[0]["lr"],
                                                                       "".join("  %s: %.5f" % kv for kv in extra.items()),
                                                                       "  saved" if saved else ""))
    return history


class Driver:
    """What train_3d_match.py, train_kitti.py and train_open_gf.py share, written once and bound to one of them.  `mod` is the
    driver module: it keeps the reference's attributes (use_GAN, lr_g, lr_d, epochs, the save paths, ...), and every method reads
    them from it when it is called, so a caller that assigns one is obeyed.  real_rows: pair_real_rows / dem_real_rows, what
    use_GAN renders as the real images; batch_help: the --batch help text."""

    def __init__(self, mod, real_rows: Callable, batch_help: str):
        self.mod, self.real_rows, self.batch_help = mod, real_rows, batch_help

    def update_lr(self, optimizer, gamma=0.5):
        """The reference's update_lr (train_3d_match.py:46-51, train_kitti.py:55-60, train_open_gf.py:44-49)."""
        m = self.mod
        m.lr_g = max(m.lr_g * gamma, m.min_learning_rate)
        for param_group in optimizer.param_groups:
            param_group['lr'] = m.lr_g
        print("lr update finished  cur lr: %.5f" % m.lr_g)

    @staticmethod
    def evaluate(net, val_loader, prepare_val) -> float:
        """The validation loss: the reference's evaluate() without the open3d ICP and the columns that need it."""
        return val_loss(net, val_loader, prepare_val)[0]

    def gan(self, device) -> GanTraining:
        """What use_GAN adds: the driver's lr_d, ground-truth rows and discriminator_save_path."""
        return gan_training(device, self.real_rows, lr_d=self.mod.lr_d, save_path=self.mod.discriminator_save_path)

    def train(self, model, datasets: Callable, preparers: Callable, synthetic=0, batch=1, train_backend=None, layers=(6, 6),
              n_epochs=None, save_path=None, device=None, log=print, scaler=None, gan=None, chamfer_weight=None) -> List[dict]:
        """The body of the reference's train(): `model` (a class) on `device`, FusedAdam at lr_g, loaders over
        datasets(synthetic) -> (train_set, val_set), preparers(device) -> (prepare_train, prepare_val), then fit().  The torch
        global generator is consumed in this order: the model, the loaders, the GAN loss.  chamfer_weight: the weight of the
        Chamfer term against the driver's real_rows (None: the module's chamfer_weight, which --chamfer sets; 0 without one).
        Returns fit()'s history."""
        from .optim import FusedAdam
        m = self.mod
        device = torch.device(device if device is not None else "cuda:0")
        net = model(d_model=256, self_layer_num=layers[0], cross_layer_num=layers[1])
        if train_backend is not None:
            net.train_backend = train_backend
        net.to(device)
        optimizer_G = FusedAdam(params=net.parameters(), lr=m.lr_g)
        train_set, val_set = datasets(synthetic)
        train_loader = DataLoader(train_set, batch_size=batch, shuffle=True, collate_fn=list)
        val_loader = DataLoader(val_set, batch_size=batch, shuffle=False, collate_fn=list)
        prepare_train, prepare_val = preparers(device)
        return fit(net, optimizer_G, train_loader, val_loader, prepare_train, prepare_val, m.epochs if n_epochs is None else n_epochs,
                   save_path or m.generator_save_path, scaler=scaler, gamma=m.learning_rate_decay_gamma, every=m.lr_update_epoch,
                   floor=m.min_learning_rate, log=log, gan=m._gan(device) if (m.use_GAN if gan is None else gan) else None,
                   chamfer_weight=float(getattr(m, "chamfer_weight", 0.0) if chamfer_weight is None else chamfer_weight),
                   chamfer_rows=self.real_rows)

    def main(self, argv=None):
        from .model import PointTransformer
        m = self.mod
        ap = argparse.ArgumentParser()
        ap.add_argument("--batch", type=int, default=1, help=self.batch_help)
        ap.add_argument("--synthetic", type=int, default=0)
        ap.add_argument("--train-backend", choices=PointTransformer.TRAIN_BACKENDS, default=None)
        ap.add_argument("--epochs", type=int, default=m.epochs)
        ap.add_argument("--gan", action="store_true", help="train with the adversarial loss (use_GAN)")
        ap.add_argument("--chamfer", type=float, default=0.0, metavar="W",
                        help="add W times the HIP Chamfer distance against the ground-truth rows to the point loss (default 0: off)")
        a = ap.parse_args(argv)
        if a.chamfer < 0:
            ap.error("--chamfer must not be negative")
        m.use_GAN = m.use_GAN or a.gan
        m.chamfer_weight = a.chamfer
        m.train(a.synthetic, a.batch, a.train_backend, n_epochs=a.epochs)


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
