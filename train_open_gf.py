"""Drop-in for the reference's ``train_open_gf.py``: the same names (update_lr, evaluate, train), path and hyper-parameters, over
the loops of scream_amd/fit.py -- DEMTransformer on packed batches, the HIP forward / backward, FusedAdam.

    python train_open_gf.py [--batch 1] [--synthetic N] [--train-backend f32|split|bf16] [--gan] [--chamfer W] [--epochs 45]

With the reference's on-disk splits present (``OpenGF_train/`` and ``OpenGF_val/``: 1.npy, 2.npy, ... [N,6] DSM | DEM) it trains
on them; ``--synthetic N`` trains on N seeded synthetic terrain patches and validates on N / 4 others.  Nothing runs at import.
evaluate() returns the validation loss (the reference's "chamfer loss" is this L1 loss); its height-loss progress column is
evaluate_open_gf.py's.  ``--chamfer W`` adds W times the Chamfer distance of scream_amd/chamfer.py against the ground-truth DEM to
the L1 loss of every step (fit(chamfer_weight=W)); that term needs no row pairing between prediction and ground truth.  ``--gan`` turns on use_GAN: the adversarial loss of
scream_amd/gan.py (a 2-channel HIP discriminator, FusedAdam at lr_d with betas (0.5, 0.999)) through fit(gan=...); the
discriminator is saved to discriminator_save_path whenever the generator is.
"""
import os
import sys

from scream_amd.evaluate_open_gf import OpenGFFiles, SyntheticDEM
from scream_amd.fit import Driver, dem_preparer, dem_real_rows

use_GAN = False
generator_save_path = "params/dem-generator.pth"
discriminator_save_path = "params/discriminator.pth"

lr_g = 0.0002
lr_d = 0.0001
min_learning_rate = 0.00001
learning_rate_decay_gamma = 0.5
lr_update_epoch = 15
epochs = 45


def _count(root):
    n = 0
    while os.path.exists(os.path.join(root, "%d.npy" % (n + 1))):
        n += 1
    return n


def _datasets(synthetic):
    if synthetic:
        return SyntheticDEM(synthetic, 0), SyntheticDEM(max(synthetic // 4, 1), 10 ** 6)
    for d in ("OpenGF_train", "OpenGF_val"):
        if _count(d) == 0:
            raise FileNotFoundError("%s/ is not populated (process_open_gf.py writes it); pass --synthetic N to train on seeded "
                                    "synthetic terrain" % d)
    return OpenGFFiles("OpenGF_train", _count("OpenGF_train")), OpenGFFiles("OpenGF_val", _count("OpenGF_val"))


def _preparers(device):
    return (dem_preparer(device),) * 2


_driver = Driver(sys.modules[__name__], dem_real_rows, "samples per step (the reference trains at 1)")
update_lr, _gan, main = _driver.update_lr, _driver.gan, _driver.main
evaluate = _driver.evaluate  # the validation loss (train_open_gf.py:52-76)


def train(synthetic=0, batch=1, train_backend=None, layers=(6, 6), n_epochs=None, save_path=None, device=None, log=print, gan=None):
    """train_open_gf.py:79-146.  Returns fit()'s history."""
    from models.pointnet import DEMTransformer
    return _driver.train(DEMTransformer, _datasets, _preparers, synthetic, batch, train_backend, layers, n_epochs, save_path, device,
                         log, gan=gan)


if __name__ == "__main__":
    main()
