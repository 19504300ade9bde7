"""Drop-in for the reference's ``train_3d_match.py``: the same names (update_lr, evaluate, train), paths and hyper-parameters,
over the loops of scream_amd/fit.py -- batches prepared on the GPU, the HIP forward / backward, FusedAdam.

    python train_3d_match.py [--batch 1] [--synthetic N] [--train-backend f32|split|bf16] [--gan] [--epochs 45]

With the reference's on-disk splits present (``3DMatch_train/`` and ``3DMatch_val/``: src%d.npy, tgt%d.npy, T%d.npy, raw metric
clouds) it trains on them; ``--synthetic N`` trains on N seeded synthetic pairs and validates on N / 4 others (no dataset ships
with either repository).  Nothing runs at import.  Left out: the reference's look() (visualisation) and the RE / TE progress
columns with open3d ICP; evaluate() returns the validation loss, and RE / TE without ICP when asked.  ``--gan`` turns on use_GAN: the adversarial loss of
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
generator_save_path = "params/point-generator.pth"
discriminator_save_path = "params/discriminator.pth"

lr_g = 0.0002
lr_d = 0.0001
min_learning_rate = 0.00001
learning_rate_decay_gamma = 0.5
lr_update_epoch = 15
epochs = 45


def update_lr(optimizer, gamma=0.5):
    """train_3d_match.py:46-51."""
    global lr_g
    lr_g = max(lr_g * gamma, min_learning_rate)
    for param_group in optimizer.param_groups:
        param_group['lr'] = lr_g
    print("lr update finished  cur lr: %.5f" % lr_g)


def _loaders(synthetic, batch):
    if synthetic:
        train_set, val_set = SyntheticRawPairs("3dmatch", synthetic, 0), SyntheticRawPairs("3dmatch", max(synthetic // 4, 1), 10 ** 6)
    else:
        for d in ("3DMatch_train", "3DMatch_val"):
            if not os.path.exists(os.path.join(d, "T0.npy")):
                raise FileNotFoundError("%s/ is not populated (process_3d_match.py writes it); pass --synthetic N to train on seeded "
                                        "synthetic pairs" % d)
        train_set, val_set = RawPairFiles("3DMatch_train"), RawPairFiles("3DMatch_val")
    return (data.DataLoader(train_set, batch_size=batch, shuffle=True, collate_fn=list),
            data.DataLoader(val_set, batch_size=batch, shuffle=False, collate_fn=list))


def evaluate(net, val_loader, prepare_val, metrics_items=None):
    """train_3d_match.py:106-153 without the open3d ICP: the validation loss; with `metrics_items` (the reference's 9-tuples,
    scream_amd.data.SyntheticPairs / PairFileDataset) also the mean RE and TE of the pre-ICP pose: (loss, rre, rte)."""
    loss, _ = val_loss(net, val_loader, prepare_val)
    if metrics_items is None:
        return loss
    from scream_amd.evaluate import evaluate_items
    rows = evaluate_items(net, [metrics_items[i] for i in range(len(metrics_items))], list(range(len(metrics_items))), icp=None)
    return loss, float(rows[:, 4].mean()), float(rows[:, 5].mean())


def _gan(device):
    """What use_GAN adds: this driver's lr_d, ground-truth rows and discriminator_save_path."""
    return gan_training(device, pair_real_rows, lr_d=lr_d, save_path=discriminator_save_path)


def train(synthetic=0, batch=1, train_backend=None, layers=(6, 6), n_epochs=None, save_path=None, device=None, log=print, gan=None):
    """train_3d_match.py:156-233.  Returns fit()'s history."""
    from models.pointnet import PointTransformer
    device = torch.device(device if device is not None else "cuda:0")
    net = PointTransformer(d_model=256, self_layer_num=layers[0], cross_layer_num=layers[1])
    if train_backend is not None:
        net.train_backend = train_backend
    net.to(device)
    optimizer_G = FusedAdam(params=net.parameters(), lr=lr_g)
    train_loader, val_loader = _loaders(synthetic, batch)
    return fit(net, optimizer_G, train_loader, val_loader, pair_preparer("3dmatch", True, device), pair_preparer("3dmatch", False, device),
               epochs if n_epochs is None else n_epochs, save_path or generator_save_path, gamma=learning_rate_decay_gamma,
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
