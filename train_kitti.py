"""Drop-in for the reference's ``train_kitti.py``: the same names (update_lr, evaluate, train), path and hyper-parameters, over
the loops of scream_amd/fit.py -- batches prepared on the GPU, the HIP forward / backward, FusedAdam under a GradScaler.

    python train_kitti.py [--batch 1] [--synthetic N] [--train-backend f32|split|bf16] [--gan] [--epochs 120]

With the reference's on-disk splits present (``KITTI_train/`` and ``KITTI_val/``: src%d.npy, tgt%d.npy, T%d.npy, raw metric
clouds) it trains on them; ``--synthetic N`` trains on N seeded synthetic pairs and validates on N / 4 others.  Nothing runs at
import.  The reference keeps the checkpoint with the best registration recall (train_kitti.py:223-229, open3d ICP inside the
loop); here, as in the other two drivers, it is the one with the best validation loss, and evaluate() returns that loss: pose
metrics with the GPU ICP are evaluate_kitti.py's.  ``--gan`` turns on use_GAN: the adversarial loss of
scream_amd/gan.py (a 2-channel HIP discriminator, FusedAdam at lr_d with betas (0.5, 0.999)) through fit(gan=...); the
discriminator is saved to discriminator_save_path whenever the generator is.
"""
import argparse
import os

import torch
from torch.utils import data

from scream_amd import FusedAdam
from scream_amd.data import RawPairFiles, SyntheticRawPairs
from scream_amd.fit import fit, gan_training, pair_preparer, pair_real_rows, val_loss
from scream_amd.model import PointTransformer

use_GAN = False
generator_save_path = "params/kitti-generator.pth"
discriminator_save_path = "params/discriminator.pth"

lr_g = 0.00032
lr_d = 0.0001
min_learning_rate = 0.00001
learning_rate_decay_gamma = 0.5
lr_update_epoch = 10
epochs = 120


def update_lr(optimizer, gamma=0.5):
    """train_kitti.py:55-60."""
    global lr_g
    lr_g = max(lr_g * gamma, min_learning_rate)
    for param_group in optimizer.param_groups:
        param_group['lr'] = lr_g
    print("lr update finished  cur lr: %.5f" % lr_g)


def _loaders(synthetic, batch):
    if synthetic:
        train_set, val_set = SyntheticRawPairs("kitti", synthetic, 0), SyntheticRawPairs("kitti", max(synthetic // 4, 1), 10 ** 6)
    else:
        for d in ("KITTI_train", "KITTI_val"):
            if not os.path.exists(os.path.join(d, "T0.npy")):
                raise FileNotFoundError("%s/ is not populated (process_kitti.py writes it); pass --synthetic N to train on seeded "
                                        "synthetic pairs" % d)
        train_set, val_set = RawPairFiles("KITTI_train"), RawPairFiles("KITTI_val")
    return (data.DataLoader(train_set, batch_size=batch, shuffle=True, collate_fn=list),
            data.DataLoader(val_set, batch_size=batch, shuffle=False, collate_fn=list))


def evaluate(net, val_loader, prepare_val):
    """The validation loss (train_kitti.py:63-135 without the open3d ICP and its recall)."""
    return val_loss(net, val_loader, prepare_val)[0]


def _gan(device):
    """What use_GAN adds: this driver's lr_d, ground-truth rows and discriminator_save_path."""
    return gan_training(device, pair_real_rows, lr_d=lr_d, save_path=discriminator_save_path)


def train(synthetic=0, batch=1, train_backend=None, layers=(6, 6), n_epochs=None, save_path=None, device=None, log=print, scaler=None, gan=None):
    """train_kitti.py:138-233.  Returns fit()'s history."""
    from models.pointnet import PointTransformer
    device = torch.device(device if device is not None else "cuda:0")
    net = PointTransformer(d_model=256, self_layer_num=layers[0], cross_layer_num=layers[1])
    if train_backend is not None:
        net.train_backend = train_backend
    net.to(device)
    optimizer_G = FusedAdam(params=net.parameters(), lr=lr_g)
    # train_kitti.py:52,186-188: scaler.scale(loss).backward(); scaler.step(optimizer_G); scaler.update().  The reference needs
    # the scaler because its forward runs under autocast.  Here the arithmetic of the matrix products is net.train_backend, not
    # a context manager: "f32" and "split" are fp32-accurate, and --train-backend bf16 is the mirror of the reference's autocast
    # (one 16-bit product per GEMM, fp32 accumulation; bf16 where the reference has fp16).  The split and the bf16 backend are
    # scale free, so the scaled gradients are the gradients times the scale.  FusedAdam takes the scale and the scaler's
    # found_inf on the device, so the step reads nothing back.
    scaler = scaler if scaler is not None else torch.amp.GradScaler("cuda")
    train_loader, val_loader = _loaders(synthetic, batch)
    return fit(net, optimizer_G, train_loader, val_loader, pair_preparer("kitti", True, device), pair_preparer("kitti", False, device),
               epochs if n_epochs is None else n_epochs, save_path or generator_save_path, scaler=scaler, gamma=learning_rate_decay_gamma,
               every=lr_update_epoch, floor=min_learning_rate, log=log,
               gan=_gan(device) if (use_GAN if gan is None else gan) else None)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1, help="pairs per step (the reference trains at 1)")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--train-backend", choices=PointTransformer.TRAIN_BACKENDS, default=None)
    ap.add_argument("--epochs", type=int, default=epochs)
    ap.add_argument("--gan", action="store_true", help="train with the adversarial loss (use_GAN)")
    a = ap.parse_args(argv)
    global use_GAN
    use_GAN = use_GAN or a.gan
    train(a.synthetic, a.batch, a.train_backend, n_epochs=a.epochs)


if __name__ == "__main__":
    main()
