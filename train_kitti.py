"""Drop-in for the reference's ``train_kitti.py``: the same names (update_lr, evaluate, train), path and hyper-parameters, over
the loops of scream_amd/fit.py -- batches prepared on the GPU, the HIP forward / backward, FusedAdam under a GradScaler.

    python train_kitti.py [--batch 1] [--synthetic N] [--train-backend f32|split|bf16] [--gan] [--chamfer W] [--epochs 120]

With the reference's on-disk splits present (``KITTI_train/`` and ``KITTI_val/``: src%d.npy, tgt%d.npy, T%d.npy, raw metric
clouds) it trains on them; ``--synthetic N`` trains on N seeded synthetic pairs and validates on N / 4 others.  Nothing runs at
import.  The reference keeps the checkpoint with the best registration recall (train_kitti.py:223-229, open3d ICP inside the
loop); here, as in the other two drivers, it is the one with the best validation loss, and evaluate() returns that loss: pose
metrics with the GPU ICP are evaluate_kitti.py's.  ``--gan`` turns on use_GAN: the adversarial loss of
scream_amd/gan.py (a 2-channel HIP discriminator, FusedAdam at lr_d with betas (0.5, 0.999)) through fit(gan=...); the
discriminator is saved to discriminator_save_path whenever the generator is.
"""
import os
import sys

import torch

from scream_amd.data import RawPairFiles, SyntheticRawPairs
from scream_amd.fit import Driver, pair_preparer, pair_real_rows

use_GAN = False
generator_save_path = "params/kitti-generator.pth"
discriminator_save_path = "params/discriminator.pth"

lr_g = 0.00032
lr_d = 0.0001
min_learning_rate = 0.00001
learning_rate_decay_gamma = 0.5
lr_update_epoch = 10
epochs = 120


def _datasets(synthetic):
    if synthetic:
        return SyntheticRawPairs("kitti", synthetic, 0), SyntheticRawPairs("kitti", max(synthetic // 4, 1), 10 ** 6)
    for d in ("KITTI_train", "KITTI_val"):
        if not os.path.exists(os.path.join(d, "T0.npy")):
            raise FileNotFoundError("%s/ is not populated (process_kitti.py writes it); pass --synthetic N to train on seeded "
                                    "synthetic pairs" % d)
    return RawPairFiles("KITTI_train"), RawPairFiles("KITTI_val")


def _preparers(device):
    return pair_preparer("kitti", True, device), pair_preparer("kitti", False, device)


_driver = Driver(sys.modules[__name__], pair_real_rows, "pairs per step (the reference trains at 1)")
update_lr, _gan, main = _driver.update_lr, _driver.gan, _driver.main
evaluate = _driver.evaluate  # the validation loss (train_kitti.py:63-135 without the open3d ICP and its recall)


def train(synthetic=0, batch=1, train_backend=None, layers=(6, 6), n_epochs=None, save_path=None, device=None, log=print, scaler=None, gan=None):
    """train_kitti.py:138-233.  Returns fit()'s history."""
    from models.pointnet import PointTransformer
    # train_kitti.py:52,186-188: scaler.scale(loss).backward(); scaler.step(optimizer_G); scaler.update().  The reference needs
    # the scaler because its forward runs under autocast.  Here the arithmetic of the matrix products is net.train_backend, not
    # a context manager: "f32" and "split" are fp32-accurate, and --train-backend bf16 is the mirror of the reference's autocast
    # (one 16-bit product per GEMM, fp32 accumulation; bf16 where the reference has fp16).  The split and the bf16 backend are
    # scale free, so the scaled gradients are the gradients times the scale.  FusedAdam takes the scale and the scaler's
    # found_inf on the device, so the step reads nothing back.
    scaler = scaler if scaler is not None else torch.amp.GradScaler("cuda")
    return _driver.train(PointTransformer, _datasets, _preparers, synthetic, batch, train_backend, layers, n_epochs, save_path, device,
                         log, scaler=scaler, gan=gan)


if __name__ == "__main__":
    main()
