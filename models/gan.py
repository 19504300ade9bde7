"""Drop-in for the reference's ``models/gan.py``: same import path and names (reference models/gan.py:6-65), backed by the
MI355X kernels in ``scream_amd`` (csrc/gan.hip).

    from models.gan import NLayerDiscriminator, weights_init
    dis = NLayerDiscriminator(input_nc=2, ndf=64, n_layers=3).apply(weights_init).to("cuda:0")
    logits = dis(imgs)                           # [n, 2, 64, 64] -> [n, 1, 6, 6], differentiable
"""
from scream_amd.gan import NLayerDiscriminator, weights_init  # noqa: F401

__all__ = ["NLayerDiscriminator", "weights_init"]
