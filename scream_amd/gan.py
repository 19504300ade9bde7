"""The adversarial rendering loss on the HIP kernels of csrc/gan.hip: the reference's PatchGAN discriminator (models/gan.py:15-65)
and AdversarialLoss (loss.py:16-66).

    gan_loss = AdversarialLoss().to(dev)                              # 2 input channels: what RegistrationRender emits
    opt_d = FusedAdam(gan_loss.discriminator.parameters(), lr=1e-4, betas=(0.5, 0.999))
    g_loss = gan_loss(imgs, None, 0)                                  # -mean D(fake); gradient into imgs only
    d_loss = gan_loss(imgs.detach(), real, 1)                         # hinge loss; two passes of D alive until its backward

``NLayerDiscriminator`` holds its parameters and buffers in the reference's own modules (``main.0.weight`` ... ``main.11.bias``,
``main.{3,6,9}.running_mean / running_var / num_batches_tracked``), so ``state_dict()`` interchanges with the reference both ways,
but it never calls them: one autograd.Function runs the whole network -- five implicit-GEMM convolutions on the fp32 matrix
cores, BatchNorm with float64 statistics, LeakyReLU -- and keeps the activations of its pass in one workspace.  Every sum has a
fixed order and there are no float atomics: a step repeats bit for bit.  There is no CPU path (ScreamHipError) and no fall-back
to torch's convolutions.

Differences from the reference, all stated:
  * the default is ``input_nc=2``: the reference builds its discriminator with 3 input channels while its renderer emits 2, so
    its use_GAN=True loop does not run as written.  1 to 4 channels are accepted, so a 3-channel state dict still loads and runs;
  * branch 0 (the generator update) computes the gradient with respect to the images only.  The reference also accumulates
    discriminator weight gradients there, but zeroes them (optimizer_D.zero_grad()) before their only use;
  * ``calculate_adaptive_weight`` is left out: in the reference it reads attributes that do not exist;
  * eval() is supported under no_grad only (BatchNorm is then the affine map of the running statistics); with grad mode on it
    raises NotImplementedError.
Supported: n_layers == 3, use_actnorm=False, ndf % 32 == 0, 1 <= input_nc <= 4, H and W >= 24 (at 23 the fourth convolution no
longer fits).
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib, ops

__all__ = ["weights_init", "NLayerDiscriminator", "AdversarialLoss", "g_loss", "hinge_d_loss", "MIN_SIZE"]

MIN_SIZE = 24
CONV_AT, BN_AT = (0, 2, 5, 8, 11), (3, 6, 9)


def weights_init(m):
    """The initialisation of models/gan.py:6-12, for ``module.apply``: convolution weights from N(0, 0.02), BatchNorm scales from
    N(1, 0.02) with zero shifts; every other module is left alone.  It draws from torch's global generator in the reference's
    order, so the same seed gives the reference's initial values."""
    with torch.no_grad():
        if isinstance(m, nn.Conv2d):
            m.weight.normal_(0.0, 0.02)
        elif isinstance(m, nn.BatchNorm2d):
            m.weight.normal_(1.0, 0.02)
            m.bias.zero_()


class _DiscFn(torch.autograd.Function):
    """logits of one pass.  tensors: 5 conv weights, the two biases, 3 gammas, 3 betas (differentiable), then 3 running means,
    3 running variances and 3 counters (updated in place by the kernels in training mode)."""

    @staticmethod
    def forward(ctx, x, ndf, training, *tensors):
        x = x.detach().contiguous()
        held = [t.detach() for t in tensors]
        params = ops.gan_params(held[0:5], held[5], held[6], held[7:10], held[10:13], held[13:16], held[16:19], held[19:22])
        n, cin, h, w = x.shape
        ws = ops.gan_workspace(n, cin, ndf, h, w, x.device)
        logits = ops.gan_forward(x, params, ndf, training, ws)
        ctx.ndf, ctx.training = ndf, training
        ctx.save_for_backward(x, ws, *held[:13])
        ctx.stats = held[13:]
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if not ctx.training:
            raise NotImplementedError("the discriminator's backward differentiates a training-mode pass only")
        x, ws = ctx.saved_tensors[:2]
        held = list(ctx.saved_tensors[2:])
        params = ops.gan_params(held[0:5], held[5], held[6], held[7:10], held[10:13], ctx.stats[0:3], ctx.stats[3:6], ctx.stats[6:9])
        want = any(ctx.needs_input_grad[3:16])
        grads = [torch.empty_like(t) for t in held] if want else None
        dx = ops.gan_backward(dlogits.to(torch.float32).contiguous(), x, params, ctx.ndf, ws, ctx.needs_input_grad[0], grads)
        return (dx, None, None) + (tuple(grads) if want else (None,) * 13) + (None,) * 9


class NLayerDiscriminator(nn.Module):
    """models/gan.py:15-65 with n_layers=3 and BatchNorm2d: conv(k4,s2,p1,bias) leaky | conv(k4,s2,p1) bn leaky, twice |
    conv(k4,s1,p1) bn leaky | conv(k4,s1,p1,bias) -> 1 channel.  forward(input [n,input_nc,h,w] on the GPU) -> logits."""

    def __init__(self, input_nc=2, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        if use_actnorm:
            raise NotImplementedError("NLayerDiscriminator: use_actnorm=True (ActNorm) is not implemented; only BatchNorm2d is")
        if n_layers != 3:
            raise NotImplementedError("NLayerDiscriminator: the HIP kernels are built for n_layers == 3, got %r" % (n_layers,))
        if int(ndf) != ndf or ndf <= 0 or ndf % 32:
            raise NotImplementedError("NLayerDiscriminator: ndf must be a positive multiple of 32 (ndf %% 32 == 0), got %r" % (ndf,))
        if int(input_nc) != input_nc or not 1 <= input_nc <= 4:
            raise NotImplementedError("NLayerDiscriminator: 1 <= input_nc <= 4 is supported, got %r" % (input_nc,))
        self.input_nc, self.ndf = int(input_nc), int(ndf)
        ndf = self.ndf
        # the reference's modules in the reference's order: they hold the parameters under the reference's names (and draw their
        # initial values as the reference does); forward never calls them
        seq = [nn.Conv2d(self.input_nc, ndf, kernel_size=4, stride=2, padding=1), nn.LeakyReLU(0.2, True)]
        for cin, cout, stride in ((ndf, 2 * ndf, 2), (2 * ndf, 4 * ndf, 2), (4 * ndf, 8 * ndf, 1)):
            seq += [nn.Conv2d(cin, cout, kernel_size=4, stride=stride, padding=1, bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.2, True)]
        seq += [nn.Conv2d(8 * ndf, 1, kernel_size=4, stride=1, padding=1)]
        self.main = nn.Sequential(*seq)

    def _tensors(self):
        m = self.main
        return ([m[i].weight for i in CONV_AT] + [m[0].bias, m[11].bias] + [m[i].weight for i in BN_AT] + [m[i].bias for i in BN_AT] +
                [m[i].running_mean for i in BN_AT] + [m[i].running_var for i in BN_AT] + [m[i].num_batches_tracked for i in BN_AT])

    def forward(self, input, weight_grads: bool = True):
        """weight_grads=False: the pass differentiates with respect to `input` only (AdversarialLoss's generator branch)."""
        if input.dim() != 4 or input.shape[1] != self.input_nc:
            raise ValueError("NLayerDiscriminator takes [n, %d, h, w] images, got %s" % (self.input_nc, tuple(input.shape)))
        if input.shape[0] < 1 or input.shape[2] < MIN_SIZE or input.shape[3] < MIN_SIZE:
            raise ValueError("NLayerDiscriminator needs at least one image with H and W >= %d (the fourth convolution no longer fits "
                             "below), got %s" % (MIN_SIZE, tuple(input.shape)))
        if input.dtype != torch.float32:
            raise TypeError("NLayerDiscriminator takes fp32 images, got %s" % input.dtype)
        if not self.training and torch.is_grad_enabled():
            raise NotImplementedError("NLayerDiscriminator in eval() mode runs under torch.no_grad() only: the backward through the "
                                      "running statistics is not implemented")
        if not input.is_cuda or not self.main[0].weight.is_cuda:
            raise _lib.ScreamHipError("NLayerDiscriminator needs its images and parameters on the MI355X (got %s, %s); there is no "
                                      "CPU path" % (input.device, self.main[0].weight.device))
        tensors = self._tensors()
        if not weight_grads:
            tensors = [t.detach() for t in tensors]
        return _DiscFn.apply(input, self.ndf, self.training, *tensors)


class _GLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        logits = logits.detach().contiguous()
        ctx.save_for_backward(logits)
        return ops.gan_loss_g(logits)

    @staticmethod
    def backward(ctx, dout):
        return ops.gan_loss_g_bwd(dout.to(torch.float32).contiguous(), ctx.saved_tensors[0])


class _DLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, real, fake):
        real, fake = real.detach().contiguous(), fake.detach().contiguous()
        ctx.save_for_backward(real, fake)
        return ops.gan_loss_d(real, fake)

    @staticmethod
    def backward(ctx, dout):
        return ops.gan_loss_d_bwd(dout.to(torch.float32).contiguous(), *ctx.saved_tensors)


def _check_logits(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.ScreamHipError("the GAN losses need logits on the MI355X (got %s); there is no CPU path" % t.device)
        if t.dtype != torch.float32 or t.numel() == 0:
            raise TypeError("the GAN losses take non-empty fp32 logits, got %s %s" % (t.dtype, tuple(t.shape)))


def g_loss(logits_fake):
    """-mean(logits_fake) (loss.py:56): a float64 sum in a fixed order, one fp32 scalar."""
    _check_logits(logits_fake)
    return _GLossFn.apply(logits_fake)


def hinge_d_loss(logits_real, logits_fake):
    """0.5 (mean relu(1 - logits_real) + mean relu(1 + logits_fake)) (loss.py:31-35); relu'(0) = 0."""
    _check_logits(logits_real, logits_fake)
    return _DLossFn.apply(logits_real, logits_fake)


class AdversarialLoss(nn.Module):
    """loss.py:16-66.  forward(fake, real, 0): the generator's loss (real is not read); forward(fake, real, 1): the
    discriminator's hinge loss on real.detach() and fake.detach()."""

    def __init__(self, input_nc=2, ndf=64):
        super().__init__()
        self.discriminator = NLayerDiscriminator(input_nc, ndf).apply(weights_init)

    def adopt_weight(self, weight, global_step, threshold=0, value=0.0):
        """loss.py:26-29: `value` until `global_step` reaches `threshold`, `weight` from then on."""
        return value if global_step < threshold else weight

    def hinge_d_loss(self, logits_real, logits_fake):
        return hinge_d_loss(logits_real, logits_fake)

    def forward(self, fake, real, optimizer_idx):
        if optimizer_idx == 0:
            return g_loss(self.discriminator(fake, weight_grads=False))
        if optimizer_idx == 1:
            logits_real = self.discriminator(real.detach())
            logits_fake = self.discriminator(fake.contiguous().detach())
            return self.hinge_d_loss(logits_real, logits_fake)
        raise ValueError("optimizer_idx must be 0 (generator) or 1 (discriminator), got %r" % (optimizer_idx,))
