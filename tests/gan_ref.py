"""A restatement of the adversarial loss of include/scream_hip.h ("The adversarial loss") in plain torch tensor algebra, in whatever
dtype and on whatever device its inputs have: float64 is the oracle of tests/test_gpu_gan.py and tests/test_gan_host.py, float32
on the CPU is the "fp32 expression" their bar is measured against.  Convolution is unfold + matmul (never nn.Conv2d / MIOpen),
its gradients are the transposed matmul + fold and the matmul against the unfolded input.

Like oracle/scream_ref.py with its relu masks, every kinked unit takes its mask from outside when `masks=` is given: the four
LeakyReLU layers (masks["leaky"]: four bool tensors, True where the unit passes its input unchanged) and the two hinge relus
(masks["real"], masks["fake"]: True where the relu is open).  Without `masks` the masks are the pass's own.

The state dict is the reference's (models/gan.py): main.{0,2,5,8,11}.weight, main.{0,11}.bias, main.{3,6,9}.weight / bias /
running_mean / running_var / num_batches_tracked.
"""
import torch
import torch.nn.functional as F

CONVS = ((0, 2), (2, 2), (5, 2), (8, 1), (11, 1))  # (index in main, stride)
BNS = (None, 3, 6, 9, None)
EPS, MOMENTUM, LEAK = 1e-5, 0.1, 0.2


def out_size(h, w, stride):
    return (h - 2) // stride + 1, (w - 2) // stride + 1


def conv(x, w, b, stride):
    n, _, h, wd = x.shape
    ho, wo = out_size(h, wd, stride)
    y = (w.reshape(w.shape[0], -1) @ F.unfold(x, 4, padding=1, stride=stride)).view(n, w.shape[0], ho, wo)
    return y if b is None else y + b.view(1, -1, 1, 1)


def conv_dgrad(dy, w, h, wd, stride):
    n, co = dy.shape[:2]
    return F.fold(w.reshape(co, -1).t() @ dy.reshape(n, co, -1), (h, wd), 4, padding=1, stride=stride)


def conv_wgrad(x, dy, stride):
    n, co = dy.shape[:2]
    cols = F.unfold(x, 4, padding=1, stride=stride)
    return (dy.reshape(n, co, -1) @ cols.transpose(1, 2)).sum(0).view(co, x.shape[1], 4, 4)


def leaky(z, mask=None):
    mask = (z > 0) if mask is None else mask
    return torch.where(mask, z, LEAK * z), mask


def bn_train(x, gamma, beta):
    """(z, xhat, invstd, mean, biased var) of training-mode BatchNorm2d."""
    mean = x.mean(dim=(0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (x - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    return xhat * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1), xhat, invstd, mean, var


def bn_bwd(dz, xhat, invstd, gamma):
    cnt = dz.shape[0] * dz.shape[2] * dz.shape[3]
    dbeta, dgamma = dz.sum(dim=(0, 2, 3)), (dz * xhat).sum(dim=(0, 2, 3))
    dx = (gamma * invstd).view(1, -1, 1, 1) * (dz - dbeta.view(1, -1, 1, 1) / cnt - xhat * dgamma.view(1, -1, 1, 1) / cnt)
    return dx, dgamma, dbeta


def running_update(running_mean, running_var, mean, var, cnt):
    """torch's rule: momentum 0.1, the running variance from the unbiased batch variance."""
    return ((1 - MOMENTUM) * running_mean + MOMENTUM * mean, (1 - MOMENTUM) * running_var + MOMENTUM * var * (cnt / (cnt - 1.0)))


def forward(x, sd, masks=None, training=True):
    """logits and everything the backward needs.  sd: tensors of x's dtype and device.  Returns a dict: logits, masks (the four
    leaky masks used), running (the new main.N.running_mean / running_var by name, training mode), cache."""
    cache, used, running = [], [], {}
    a = x
    for l, (at, stride) in enumerate(CONVS):
        w, b = sd["main.%d.weight" % at], sd.get("main.%d.bias" % at)
        z = conv(a, w, b, stride)
        entry = dict(x=a, w=w, stride=stride, bias=b is not None, at=at)
        if BNS[l] is not None:
            k = BNS[l]
            gamma, beta = sd["main.%d.weight" % k], sd["main.%d.bias" % k]
            if training:
                cnt = z.shape[0] * z.shape[2] * z.shape[3]
                if cnt == 1:
                    raise ValueError("Expected more than 1 value per channel when training")
                z, xhat, invstd, mean, var = bn_train(z, gamma, beta)
                rm, rv = running_update(sd["main.%d.running_mean" % k], sd["main.%d.running_var" % k], mean, var, cnt)
                running["main.%d.running_mean" % k], running["main.%d.running_var" % k] = rm, rv
                entry.update(bn=k, xhat=xhat, invstd=invstd, gamma=gamma)
            else:
                invstd = 1.0 / torch.sqrt(sd["main.%d.running_var" % k] + EPS)
                z = (z - sd["main.%d.running_mean" % k].view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        if l < 4:
            z, m = leaky(z, None if masks is None else masks["leaky"][l])
            used.append(m)
            entry["mask"] = m
        cache.append(entry)
        a = z
    return dict(logits=a, masks=used, running=running, cache=cache)


def backward(fw, dlogits):
    """(dx, the parameter gradients by state-dict name) of forward()'s training-mode pass."""
    grads, g = {}, dlogits
    for entry in reversed(fw["cache"]):
        if "mask" in entry:
            g = torch.where(entry["mask"], g, LEAK * g)
        if "bn" in entry:
            g, dgamma, dbeta = bn_bwd(g, entry["xhat"], entry["invstd"], entry["gamma"])
            grads["main.%d.weight" % entry["bn"]], grads["main.%d.bias" % entry["bn"]] = dgamma, dbeta
        if entry["bias"]:
            grads["main.%d.bias" % entry["at"]] = g.sum(dim=(0, 2, 3))
        grads["main.%d.weight" % entry["at"]] = conv_wgrad(entry["x"], g, entry["stride"])
        g = conv_dgrad(g, entry["w"], entry["x"].shape[2], entry["x"].shape[3], entry["stride"])
    return g, grads


def g_loss(logits_fake):
    return -logits_fake.mean()


def g_loss_grad(logits_fake, dout=1.0):
    return torch.full_like(logits_fake, -1.0 / logits_fake.numel()) * dout


def hinge_masks(logits_real, logits_fake):
    return (1.0 - logits_real) > 0, (1.0 + logits_fake) > 0


def d_loss(logits_real, logits_fake, masks=None):
    mr, mf = hinge_masks(logits_real, logits_fake) if masks is None else (masks["real"], masks["fake"])
    zero = torch.zeros((), dtype=logits_real.dtype, device=logits_real.device)
    return 0.5 * (torch.where(mr, 1.0 - logits_real, zero).mean() + torch.where(mf, 1.0 + logits_fake, zero).mean())


def d_loss_grad(logits_real, logits_fake, masks=None, dout=1.0):
    mr, mf = hinge_masks(logits_real, logits_fake) if masks is None else (masks["real"], masks["fake"])
    return (mr.to(logits_real.dtype) * (-0.5 * dout / logits_real.numel()), mf.to(logits_fake.dtype) * (0.5 * dout / logits_fake.numel()))


def cast(sd, dtype, device=None):
    return {k: (v.to(device=device) if v.dtype == torch.int64 else v.to(dtype=dtype, device=device)) for k, v in sd.items()}


def max_rel(got, want):
    """The bar's measure: the largest elementwise error divided by the largest magnitude of the float64 tensor."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()
