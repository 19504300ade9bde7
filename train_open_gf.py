"""Drop-in for the reference's ``train_open_gf.py``: the same names (update_lr, evaluate, train), path and hyper-parameters, over
the loops of scream_amd/fit.py -- DEMTransformer on packed batches, the HIP forward / backward, FusedAdam.

    python train_open_gf.py [--batch 1] [--synthetic N] [--train-backend f32|split|bf16] [--gan] [--epochs 45]

With the reference's on-disk splits present (``OpenGF_train/`` and ``OpenGF_val/``: 1.npy, 2.npy, ... [N,6] DSM | DEM) it trains
on them; ``--synthetic N`` trains on N seeded synthetic terrain patches and validates on N / 4 others.  Nothing runs at import.
evaluate() returns the validation loss (the reference's "chamfer loss" is this L1 loss); its height-loss progress column is
evaluate_open_gf.py's.  ``--gan`` turns on use_GAN: the adversarial loss of
scream_amd/gan.py (a 2-channel HIP discriminator, FusedAdam at lr_d with betas (0.5, 0.999)) through fit(gan=...); the
discriminator is saved to discriminator_save_path whenever the generator is.
"""
import argparse
import os

import torch
from torch.utils import data

from scream_amd import FusedAdam
from scream_amd.evaluate_open_gf import OpenGFFiles, SyntheticDEM
from scream_amd.fit import dem_preparer, dem_real_rows, fit, gan_training, val_loss
from scream_amd.model import PointTransformer

use_GAN = False
generator_save_path = "params/dem-generator.pth"
discriminator_save_path = "params/discriminator.pth"

lr_g = 0.0002
lr_d = 0.0001
min_learning_rate = 0.00001
learning_rate_decay_gamma = 0.5
lr_update_epoch = 15
epochs = 45


def update_lr(optimizer, gamma=0.5):
    """train_open_gf.py:44-49."""
    global lr_g
    lr_g = max(lr_g * gamma, min_learning_rate)
    for param_group in optimizer.param_groups:
        param_group['lr'] = lr_g
    print("lr update finished  cur lr: %.5f" % lr_g)


def _count(root):
    n = 0
    while os.path.exists(os.path.join(root, "%d.npy" % (n + 1))):
        n += 1
    return n


def _loaders(synthetic, batch):
    if synthetic:
        train_set, val_set = SyntheticDEM(synthetic, 0), SyntheticDEM(max(synthetic // 4, 1), 10 ** 6)
    else:
        for d in ("OpenGF_train", "OpenGF_val"):
            if _count(d) == 0:
                raise FileNotFoundError("%s/ is not populated (process_open_gf.py writes it); pass --synthetic N to train on seeded "
                                        "synthetic terrain" % d)
        train_set, val_set = OpenGFFiles("OpenGF_train", _count("OpenGF_train")), OpenGFFiles("OpenGF_val", _count("OpenGF_val"))
    return (data.DataLoader(train_set, batch_size=batch, shuffle=True, collate_fn=list),
            data.DataLoader(val_set, batch_size=batch, shuffle=False, collate_fn=list))


def evaluate(net, val_loader, prepare_val):
    """The validation loss (train_open_gf.py:52-76)."""
    return val_loss(net, val_loader, prepare_val)[0]


def _gan(device):
    """What use_GAN adds: this driver's lr_d, ground-truth rows and discriminator_save_path."""
    return gan_training(device, dem_real_rows, lr_d=lr_d, save_path=discriminator_save_path)


def train(synthetic=0, batch=1, train_backend=None, layers=(6, 6), n_epochs=None, save_path=None, device=None, log=print, gan=None):
    """train_open_gf.py:79-146.  Returns fit()'s history."""
    from models.pointnet import DEMTransformer
    device = torch.device(device if device is not None else "cuda:0")
    net = DEMTransformer(d_model=256, self_layer_num=layers[0], cross_layer_num=layers[1])
    if train_backend is not None:
        net.train_backend = train_backend
    net.to(device)
    optimizer_G = FusedAdam(params=net.parameters(), lr=lr_g)
    train_loader, val_loader = _loaders(synthetic, batch)
    prepare = dem_preparer(device)
    return fit(net, optimizer_G, train_loader, val_loader, prepare, prepare, epochs if n_epochs is None else n_epochs,
               save_path or generator_save_path, gamma=learning_rate_decay_gamma, every=lr_update_epoch, floor=min_learning_rate, log=log,
               gan=_gan(device) if (use_GAN if gan is None else gan) else None)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1, help="samples per step (the reference trains at 1)")
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
