"""Drop-in for the reference's ``loss.py``: same import path and names (reference loss.py:7-66), backed by the MI355X kernels in
``scream_amd`` (csrc/gan.hip).

    from loss import AdversarialLoss
    gan_loss = AdversarialLoss().to("cuda:0")    # a 2-channel discriminator: what RegistrationRender emits
    g_loss = gan_loss(imgs, None, 0)
    d_loss = gan_loss(imgs.detach(), real, 1)
"""
from scream_amd.gan import AdversarialLoss, weights_init  # noqa: F401

__all__ = ["AdversarialLoss", "weights_init"]
