"""Drop-in for the reference's ``train_3d_match.py``: the same names (update_lr, evaluate, train), paths and hyper-parameters,
over the loops of scream_amd/fit.py -- batches prepared on the GPU, the HIP forward / backward, FusedAdam.

    python train_3d_match.py [--batch 1] [--synthetic N] [--train-backend f32|split|bf16] [--gan] [--chamfer W] [--epochs 45]

With the reference's on-disk splits present (``3DMatch_train/`` and ``3DMatch_val/``: src%d.npy, tgt%d.npy, T%d.npy, raw metric
clouds) it trains on them; ``--synthetic N`` trains on N seeded synthetic pairs and validates on N / 4 others (no dataset ships
with either repository).  Nothing runs at import.  Left out: the reference's look() (visualisation) and the RE / TE progress
columns with open3d ICP; evaluate() returns the validation loss, and RE / TE without ICP when asked.  ``--gan`` turns on use_GAN: the adversarial loss of
scream_amd/gan.py (a 2-channel HIP discriminator, FusedAdam at lr_d with betas (0.5, 0.999)) through fit(gan=...); the
discriminator is saved to discriminator_save_path whenever the generator is.
"""
import os
import sys

from scream_amd.data import RawPairFiles, SyntheticRawPairs
from scream_amd.fit import Driver, pair_preparer, pair_real_rows

use_GAN = False
generator_save_path = "params/point-generator.pth"
discriminator_save_path = "params/discriminator.pth"

lr_g = 0.0002
lr_d = 0.0001
min_learning_rate = 0.00001
learning_rate_decay_gamma = 0.5
lr_update_epoch = 15
epochs = 45


def _datasets(synthetic):
    if synthetic:
        return SyntheticRawPairs("3dmatch", synthetic, 0), SyntheticRawPairs("3dmatch", max(synthetic // 4, 1), 10 ** 6)
    for d in ("3DMatch_train", "3DMatch_val"):
        if not os.path.exists(os.path.join(d, "T0.npy")):
            raise FileNotFoundError("%s/ is not populated (process_3d_match.py writes it); pass --synthetic N to train on seeded "
                                    "synthetic pairs" % d)
    return RawPairFiles("3DMatch_train"), RawPairFiles("3DMatch_val")


def _preparers(device):
    return pair_preparer("3dmatch", True, device), pair_preparer("3dmatch", False, device)


_driver = Driver(sys.modules[__name__], pair_real_rows, "pairs per step (the reference trains at 1)")
update_lr, _gan, main = _driver.update_lr, _driver.gan, _driver.main


def evaluate(net, val_loader, prepare_val, metrics_items=None):
    """train_3d_match.py:106-153 without the open3d ICP: the validation loss; with `metrics_items` (the reference's 9-tuples,
    scream_amd.data.SyntheticPairs / PairFileDataset) also the mean RE and TE of the pre-ICP pose: (loss, rre, rte)."""
    loss = _driver.evaluate(net, val_loader, prepare_val)
    if metrics_items is None:
        return loss
    from scream_amd.evaluate import evaluate_items
    rows = evaluate_items(net, [metrics_items[i] for i in range(len(metrics_items))], list(range(len(metrics_items))), icp=None)
    return loss, float(rows[:, 4].mean()), float(rows[:, 5].mean())


def train(synthetic=0, batch=1, train_backend=None, layers=(6, 6), n_epochs=None, save_path=None, device=None, log=print, gan=None):
    """train_3d_match.py:156-233.  Returns fit()'s history."""
    from models.pointnet import PointTransformer
    return _driver.train(PointTransformer, _datasets, _preparers, synthetic, batch, train_backend, layers, n_epochs, save_path, device,
                         log, gan=gan)


if __name__ == "__main__":
    main()
