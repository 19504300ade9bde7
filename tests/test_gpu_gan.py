"""The adversarial loss on the MI355X (scream_amd/gan.py, csrc/gan.hip) against tests/gan_ref.py in float64: every convolution
geometry of the network one kernel at a time, BatchNorm, the losses at their kinks, the whole network on both losses, and the
training loop with it.

Bar (the rule of tests/test_gpu_train_kernels.py): per tensor, max |error| against float64 divided by the float64 tensor's max,
with the float64 pass run UNDER THE GPU PASS'S OWN MASKS (the sign of every LeakyReLU unit and of the two hinge relus), must be
<= max(2 x the same quantity for the fp32 expression on the CPU, 5e-6).  The oracle is tests/gan_ref.py (unfold + matmul, never
nn.Conv2d / MIOpen), float64 on the GPU; the fp32 expression is the same code in float32 on the CPU.  Every test prints its figures
before it asserts.  Needs an MI355X: run with `pytest -m gpu`."""
import functools

import numpy as np
import pytest
import torch

import gan_ref as G
import prep_ref as PR
from scream_amd import FusedAdam, _lib, ops
from scream_amd.evaluate_open_gf import SyntheticDEM
from scream_amd.fit import dem_preparer, dem_real_rows, pair_preparer, pair_real_rows, render_rows, train_epoch, train_epoch_gan
from scream_amd.gan import AdversarialLoss, NLayerDiscriminator, g_loss, hinge_d_loss, weights_init
from scream_amd.model import DEMTransformer, PointTransformer
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 5e-6
# (N, Cin, ndf, H, W): BatchNorm over four values | an odd H | a 2 x 3 last layer, three channels | the size used in training
SHAPES = [(1, 2, 64, 24, 24), (2, 2, 32, 27, 24), (3, 3, 32, 32, 40), (6, 2, 64, 64, 64)]
STRIDES = (2, 2, 2, 1, 1)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def held(what, got, want64, cpu32):
    e, e32 = G.max_rel(got, want64), G.max_rel(cpu32, want64)
    print("%s: error %.3g, the fp32 CPU expression %.3g" % (what, e, e32))
    assert e <= max(2 * e32, FLOOR), (what, e, e32)


def geometries():
    out = []
    for n, cin, ndf, h, w in SHAPES:
        ch = (cin, ndf, 2 * ndf, 4 * ndf, 8 * ndf, 1)
        for l, s in enumerate(STRIDES):
            out.append((n, ch[l], ch[l + 1], h, w, s))
            h, w = G.out_size(h, w, s)
    return out


def randn(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------- single kernels
@pytest.mark.parametrize("geo", geometries(), ids=lambda g: "n%d_c%d_%d_%dx%d_s%d" % g)
def test_convolution_kernels_against_float64(geo):
    n, cin, cout, h, w, s = geo
    rng = np.random.default_rng(hash(geo) % 2 ** 31)
    ho, wo = G.out_size(h, w, s)
    x, wt, b, dy = randn(rng, n, cin, h, w), randn(rng, cout, cin, 4, 4, scale=0.05), randn(rng, cout), randn(rng, n, cout, ho, wo)
    xg, wg, bg, dyg = (t.to(DEV) for t in (x, wt, b, dy))
    x64, w64, b64, dy64 = (t.double() for t in (xg, wg, bg, dyg))
    # forward: plain, and with bias + LeakyReLU under the GPU's own mask
    y = ops.gan_conv_fwd(xg, wg, None, s)
    assert tuple(y.shape) == (n, cout, ho, wo)
    held("forward", y, G.conv(x64, w64, None, s), G.conv(x, wt, None, s))
    ya = ops.gan_conv_fwd(xg, wg, bg, s, leaky=True)
    mask = ya > 0
    held("forward + bias + leaky", ya, G.leaky(G.conv(x64, w64, b64, s), mask)[0], G.leaky(G.conv(x, wt, b, s), mask.cpu())[0])
    assert torch.equal(ops.gan_conv_fwd(xg, wg, bg, s), ops.gan_conv_fwd(xg, wg, None, s) + bg.view(1, -1, 1, 1))
    # data gradient: plain, and through the leaky mask of the layer below
    dx = ops.gan_conv_dgrad(dyg, wg, h, w, s)
    want64, want32 = G.conv_dgrad(dy64, w64, h, w, s), G.conv_dgrad(dy, wt, h, w, s)
    held("dgrad", dx, want64, want32)
    below = randn(rng, n, cin, h, w).to(DEV)
    below.view(-1)[0] = 0.0  # a unit exactly at the kink is closed: 0.2
    dxm = ops.gan_conv_dgrad(dyg, wg, h, w, s, mask=below)
    assert torch.equal(dxm, torch.where(below > 0, dx, 0.2 * dx))
    # weight gradient and bias column sums
    dw, db = ops.gan_conv_wgrad(xg, dyg, s, want_bias=True)
    held("wgrad", dw, G.conv_wgrad(x64, dy64, s), G.conv_wgrad(x, dy, s))
    held("bias sums", db, dy64.sum(dim=(0, 2, 3)), dy.sum(dim=(0, 2, 3)))
    # fixed-order partials: a second call gives the same bits
    for a, bb in ((y, ops.gan_conv_fwd(xg, wg, None, s)), (dx, ops.gan_conv_dgrad(dyg, wg, h, w, s)), (dw, ops.gan_conv_wgrad(xg, dyg, s)[0])):
        assert torch.equal(a, bb)


@pytest.mark.parametrize("shape", [(1, 512, 2, 2), (6, 512, 7, 7)], ids=["count4", "count294"])
def test_batchnorm_forward_backward_and_running_statistics(shape):
    rng = np.random.default_rng(shape[0])
    c = shape[1]
    cnt = shape[0] * shape[2] * shape[3]
    x, dy = randn(rng, *shape) * 0.3 + 0.5, randn(rng, *shape)
    gamma, beta = 1 + randn(rng, c, scale=0.1), randn(rng, c, scale=0.1)
    rm0, rv0 = randn(rng, c, scale=0.1), 1 + randn(rng, c, scale=0.1).abs()
    xg, dyg, gg, bg, rm, rv = (t.to(DEV) for t in (x, dy, gamma, beta, rm0.clone(), rv0.clone()))
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, mean, invstd = ops.gan_bn_fwd(xg, gg, bg, rm, rv, nbt)
    mask = y > 0
    z64, xhat64, invstd64, mean64, var64 = G.bn_train(xg.double(), gg.double(), bg.double())
    z32, xhat32, invstd32, mean32, var32 = G.bn_train(x, gamma, beta)
    held("bn forward", y, G.leaky(z64, mask)[0], G.leaky(z32, mask.cpu())[0])
    held("mean", mean, mean64, mean32)
    held("invstd", invstd, invstd64, invstd32)
    # the running statistics: torch's formula in float64 from the float64 statistics, rounded once to fp32 by the kernel
    want_rm, want_rv = G.running_update(rm0.double().to(DEV), rv0.double().to(DEV), mean64, var64, cnt)
    e_rm, e_rv = G.max_rel(rm, want_rm), G.max_rel(rv, want_rv)
    print("running_mean %.3g running_var %.3g (one fp32 rounding: 6e-8)" % (e_rm, e_rv))
    assert e_rm <= 1.2e-7 and e_rv <= 1.2e-7 and int(nbt) == 1
    ops.gan_bn_fwd(xg, gg, bg, rm, rv, nbt)
    assert int(nbt) == 2
    # eval mode: the affine map of the running statistics, nothing updated
    keep = (rm.clone(), rv.clone())
    ye, me, ie = ops.gan_bn_fwd(xg, gg, bg, rm, rv, nbt, training=False)
    want_e = (xg.double() - rm.double().view(1, -1, 1, 1)) / torch.sqrt(rv.double() + 1e-5).view(1, -1, 1, 1) * gg.double().view(1, -1, 1, 1) + bg.double().view(1, -1, 1, 1)
    assert G.max_rel(ye, G.leaky(want_e, ye > 0)[0]) <= FLOOR and int(nbt) == 2 and torch.equal(rm, keep[0]) and torch.equal(rv, keep[1])
    # backward, the leaky mask from the saved output's sign
    dx, dgamma, dbeta = ops.gan_bn_bwd(dyg, y, xg, gg, mean, invstd)
    dz64, dz32 = torch.where(mask, dyg.double(), 0.2 * dyg.double()), torch.where(mask.cpu(), dy, 0.2 * dy)
    w64, w32 = G.bn_bwd(dz64, xhat64, invstd64, gg.double()), G.bn_bwd(dz32, xhat32, invstd32, gamma)
    for name, got, a, b in zip(("bn dx", "dgamma", "dbeta"), (dx, dgamma, dbeta), w64, w32):
        held(name, got, a, b)


def test_losses_and_their_kinks():
    rng = np.random.default_rng(9)
    real, fake = randn(rng, 6, 1, 6, 6) * 2, randn(rng, 6, 1, 6, 6) * 2
    real.view(-1)[:3] = torch.tensor([1.0, 1.0 + 2 ** -20, 1.0 - 2 ** -20])  # at the kink, just closed, just open
    fake.view(-1)[:3] = torch.tensor([-1.0, -1.0 - 2 ** -20, -1.0 + 2 ** -20])
    r, f = real.to(DEV).requires_grad_(True), fake.to(DEV).requires_grad_(True)
    d = hinge_d_loss(r, f)
    g = g_loss(f)
    e_d, e_g = G.max_rel(d, G.d_loss(real.double(), fake.double())), G.max_rel(g, G.g_loss(fake.double()))
    print("d_loss %.3g g_loss %.3g (one fp32 rounding of a float64 sum)" % (e_d, e_g))
    assert d.dtype == torch.float32 and d.dim() == 0 and e_d <= 1.2e-7 and e_g <= 1.2e-7
    (3.0 * d).backward()
    dr, df = G.d_loss_grad(real.double(), fake.double(), dout=3.0)
    assert torch.equal(r.grad.cpu(), dr.float()) and torch.equal(f.grad.cpu(), df.float())
    assert r.grad.view(-1)[0] == 0 and r.grad.view(-1)[1] == 0 and r.grad.view(-1)[2] == np.float32(-1.5 / 216)  # relu'(0) = 0
    assert f.grad.view(-1)[0] == 0 and f.grad.view(-1)[1] == 0 and f.grad.view(-1)[2] == np.float32(1.5 / 216)
    f.grad = None
    (2.0 * g).backward()
    assert torch.equal(f.grad.cpu(), G.g_loss_grad(fake.double(), dout=2.0).float())
    # unequal counts, and sums longer than one pass of the block
    real2, fake2 = randn(rng, 3, 1, 30, 31), randn(rng, 5, 1, 7, 9)
    assert G.max_rel(hinge_d_loss(real2.to(DEV), fake2.to(DEV)), G.d_loss(real2.double(), fake2.double())) <= 1.2e-7
    assert torch.equal(hinge_d_loss(real2.to(DEV), fake2.to(DEV)), hinge_d_loss(real2.to(DEV), fake2.to(DEV)))


# ------------------------------------------------------------------------------------- the whole network
def discriminator(cin, ndf, seed):
    torch.manual_seed(seed)
    dis = NLayerDiscriminator(cin, ndf).apply(weights_init)
    with torch.no_grad():
        for k in (3, 6, 9):
            dis.main[k].bias.normal_(0.0, 0.1)
            dis.main[k].running_mean.normal_(0.0, 0.1)
            dis.main[k].running_var.uniform_(0.5, 1.5)
        dis.main[0].bias.normal_(0.0, 0.1)
        dis.main[11].bias.normal_(0.0, 0.1)
    return dis.to(DEV)


def gpu_masks(x, sd, training=True):
    """The leaky masks of the GPU pass on x: the same kernels layer by layer (a pass is a pure function of its inputs, bit for
    bit), on copies of the running statistics.  Returns (masks, logits)."""
    a, masks = x, []
    for l, ((at, s), bn) in enumerate(zip(G.CONVS, G.BNS)):
        w, b = sd["main.%d.weight" % at], sd.get("main.%d.bias" % at)
        if bn is None:
            a = ops.gan_conv_fwd(a, w, b, s, leaky=l == 0)
        else:
            a = ops.gan_bn_fwd(ops.gan_conv_fwd(a, w, None, s), sd["main.%d.weight" % bn], sd["main.%d.bias" % bn],
                               sd["main.%d.running_mean" % bn].clone(), sd["main.%d.running_var" % bn].clone(), None, training=training)[0]
        if l < 4:
            masks.append(a > 0)
    return masks, a


def state(dis):
    return {k: v.detach().clone() for k, v in dis.state_dict().items()}


def reference_grads(passes, sd, dtype, device, loss):
    """passes: [(x, leaky masks)]; loss "g" (one pass) or "d" (real, fake) with the hinge masks in passes[i][2].
    Returns (logits per pass, dx per pass, summed parameter gradients)."""
    sdc = G.cast(sd, dtype, device)
    fws = [G.forward(x.to(device=device, dtype=dtype), sdc, masks=dict(leaky=[m.to(device) for m in masks])) for x, masks, *_ in passes]
    if loss == "g":
        dls = [G.g_loss_grad(fws[0]["logits"])]
    else:
        hm = dict(real=passes[0][2].to(device), fake=passes[1][2].to(device))
        dls = list(G.d_loss_grad(fws[0]["logits"], fws[1]["logits"], masks=hm))
    total, dxs = {}, []
    for fw, dl in zip(fws, dls):
        dx, grads = G.backward(fw, dl)
        dxs.append(dx)
        for k, v in grads.items():
            total[k] = total[k] + v if k in total else v
    return [fw["logits"] for fw in fws], dxs, total


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_c%d_ndf%d_%dx%d" % s)
def test_whole_network_on_both_losses(shape):
    n, cin, ndf, h, w = shape
    dis = discriminator(cin, ndf, seed=n)
    sd = state(dis)
    rng = np.random.default_rng(n + 40)
    fake, real = randn(rng, n, cin, h, w).to(DEV), randn(rng, n, cin, h, w).to(DEV)
    mf, lf = gpu_masks(fake, sd)
    mr, lr = gpu_masks(real, sd)

    # ---- g_loss, with the weight gradients on (AdversarialLoss's branch 0 turns them off)
    def run_g():
        dis.load_state_dict(sd)
        dis.zero_grad()
        x = fake.clone().requires_grad_(True)
        logits = dis(x)
        g_loss(logits).backward()
        return logits.detach(), x.grad, {k: p.grad.clone() for k, p in dis.named_parameters()}

    logits, dx, grads = run_g()
    assert torch.equal(logits, lf)  # the layer-by-layer kernels are the pass: its masks are the GPU pass's own
    (l64,), (dx64,), g64 = reference_grads([(fake, mf)], sd, torch.float64, DEV, "g")
    (l32,), (dx32,), g32 = reference_grads([(fake, mf)], sd, torch.float32, "cpu", "g")
    held("g: logits", logits, l64, l32)
    held("g: dX", dx, dx64, dx32)
    assert set(grads) == set(g64) and len(grads) == 13
    for k in grads:
        held("g: " + k, grads[k], g64[k], g32[k])
    assert all(int(dis.main[k].num_batches_tracked) - int(sd["main.%d.num_batches_tracked" % k]) == 1 for k in (3, 6, 9))
    for k, v in G.forward(fake.double(), G.cast(sd, torch.float64), masks=dict(leaky=mf))["running"].items():
        assert G.max_rel(dis.state_dict()[k], v) <= 1.2e-7, k
    logits2, dx2, grads2 = run_g()
    assert torch.equal(logits, logits2) and torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    # branch 0 of the loss: the same dX, no parameter gradient
    loss = AdversarialLoss(cin, ndf).to(DEV)
    loss.discriminator.load_state_dict(sd)
    x = fake.clone().requires_grad_(True)
    loss(x, None, 0).backward()
    assert torch.equal(x.grad, dx) and all(p.grad is None for p in loss.parameters())

    # ---- d_loss: two passes alive before one backward
    def run_d():
        loss.discriminator.load_state_dict(sd)
        loss.zero_grad()
        d = loss(fake, real, 1)
        d.backward()
        return d.detach(), {k: p.grad.clone() for k, p in loss.discriminator.named_parameters()}

    d, grads = run_d()
    hinge = ((1.0 - lr) > 0, (1.0 + lf) > 0)
    passes = [(real, mr, hinge[0]), (fake, mf, hinge[1])]
    ls64, _, g64 = reference_grads(passes, sd, torch.float64, DEV, "d")
    ls32, _, g32 = reference_grads(passes, sd, torch.float32, "cpu", "d")
    hm = dict(real=hinge[0], fake=hinge[1])
    held("d: loss", d, G.d_loss(ls64[0], ls64[1], hm), G.d_loss(ls32[0], ls32[1], {k: v.cpu() for k, v in hm.items()}))
    for k in grads:
        held("d: " + k, grads[k], g64[k], g32[k])
    assert all(int(loss.discriminator.main[k].num_batches_tracked) - int(sd["main.%d.num_batches_tracked" % k]) == 2 for k in (3, 6, 9))
    d2, grads2 = run_d()
    assert torch.equal(d, d2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_scaled_upstream_gradient_scales_every_gradient_exactly():
    """dY x 2^16 gives gradients x 2^16 bit for bit: a GradScaler changes nothing but the exponent."""
    n, cin, ndf, h, w = SHAPES[1]
    dis = discriminator(cin, ndf, seed=1)
    rng = np.random.default_rng(77)
    x = randn(rng, n, cin, h, w).to(DEV)
    out = []
    for scale in (1.0, 65536.0):
        dis.zero_grad()
        xi = x.clone().requires_grad_(True)
        logits = dis(xi)
        if not out:
            dlogits = randn(rng, *logits.shape).to(DEV)
        logits.backward(dlogits * scale)
        out.append([xi.grad] + [p.grad.clone() for p in dis.parameters()])
    for a, b in zip(*out):
        assert torch.isfinite(b).all() and torch.equal(a * 65536.0, b)


def test_eval_mode_under_no_grad():
    n, cin, ndf, h, w = SHAPES[2]
    dis = discriminator(cin, ndf, seed=2).eval()
    sd = state(dis)
    x = randn(np.random.default_rng(3), n, cin, h, w).to(DEV)
    with torch.no_grad():
        logits = dis(x)
    masks, layered = gpu_masks(x, sd, training=False)
    assert torch.equal(logits, layered)  # so the masks are the GPU pass's own
    want64 = G.forward(x.double(), G.cast(sd, torch.float64), masks=dict(leaky=masks), training=False)["logits"]
    want32 = G.forward(x.cpu(), G.cast(sd, torch.float32, "cpu"), masks=dict(leaky=[m.cpu() for m in masks]), training=False)["logits"]
    held("eval logits", logits, want64, want32)
    assert all(torch.equal(dis.state_dict()[k], sd[k]) for k in sd)  # nothing is updated, the counters included
    with pytest.raises(NotImplementedError):
        dis(x)


# ------------------------------------------------------------------------------------- the loops
@functools.lru_cache(maxsize=None)
def raw_batches(seed0, n_batches):
    out = []
    for b in range(n_batches):
        items = []
        for i in range(2):
            k = seed0 + 2 * b + i
            src, tgt, T = PR.raw_pair(k, 200 + 37 * (k % 3), 300 - 29 * (k % 4))
            items.append((torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(T)))
        out.append(items)
    return out


def point_net(seed=3):
    net = PointTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(seed, 256, 1, 1))
    return net.to(DEV)


def gan_run(scaler, steps=3, g_weight=0.1):
    net = point_net()
    torch.manual_seed(0)
    loss = AdversarialLoss().to(DEV)
    opt_g, opt_d = FusedAdam(net.parameters(), lr=2e-4), FusedAdam(loss.parameters(), lr=1e-4, betas=(0.5, 0.999))
    mean, losses = train_epoch_gan(net, loss, opt_g, opt_d, raw_batches(500, steps), pair_preparer("3dmatch", True, DEV, seed=5), pair_real_rows,
                                   scaler=torch.amp.GradScaler("cuda") if scaler else None, g_weight=g_weight)
    return net, loss, mean, losses


@pytest.mark.parametrize("scaler", [False, True], ids=["plain", "grad_scaler"])
def test_train_epoch_gan_three_steps_repeat_bit_for_bit(scaler):
    torch.manual_seed(0)
    start = [p.detach().clone() for p in AdversarialLoss().to(DEV).parameters()]
    net, loss, mean, losses = gan_run(scaler)
    print("losses (point + 0.1 g, g, d) per step:\n%s" % losses)
    assert losses.shape == (3, 3) and losses.dtype == np.float32 and np.isfinite(losses).all() and mean == float(losses[:, 0].astype(np.float64).mean())
    tensors = list(net.parameters()) + list(loss.state_dict().values())
    assert all(torch.isfinite(t).all() for t in tensors)
    net2, loss2, mean2, losses2 = gan_run(scaler)
    assert np.array_equal(losses.view(np.uint32), losses2.view(np.uint32))
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), net2.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(loss.state_dict().values(), loss2.state_dict().values()))
    # fake for G, then real, then fake for D: three training-mode passes per step
    assert all(int(loss.discriminator.main[k].num_batches_tracked) == 3 * 3 for k in (3, 6, 9))
    assert all(not torch.equal(a, b) for a, b in zip(start, loss.parameters()))  # the discriminator's parameters moved


def test_g_weight_zero_leaves_the_generator_step_alone():
    batches = raw_batches(500, 1)
    nets = []
    for gan in (False, True):
        net = point_net()
        opt = FusedAdam(net.parameters(), lr=0.0)
        prepare = pair_preparer("3dmatch", True, DEV, seed=5)
        if gan:
            torch.manual_seed(0)
            loss = AdversarialLoss().to(DEV)
            train_epoch_gan(net, loss, opt, FusedAdam(loss.parameters(), lr=1e-4, betas=(0.5, 0.999)), batches, prepare, pair_real_rows, g_weight=0.0)
        else:
            train_epoch(net, opt, batches, prepare)
        nets.append(net)
    for p, q in zip(nets[0].parameters(), nets[1].parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad)


def test_pair_real_rows_and_the_packed_render_gradient():
    prepared = pair_preparer("3dmatch", False, DEV)(raw_batches(500, 1)[0])
    b = prepared.batch
    rows = pair_real_rows(prepared)
    for p, (xyz, got) in enumerate(zip(b.unpack_src(b.xyz), b.unpack_src(rows))):
        want = (prepared.rot[p].double() @ xyz.double().t() + prepared.trans[p].double()).t()
        assert (got.double() - want).abs().max().item() <= 4e-7 * max(want.abs().max().item(), 1.0)  # three fp32 roundings of order-one sums
    # render_rows: pair-major [B*V, 2, w, w]; equal to the single-pair renderer image by image, and so is its gradient
    net = point_net()
    pred = rows.clone().requires_grad_(True)
    imgs = render_rows(net, pred, prepared)
    assert tuple(imgs.shape) == (2 * 6, 2, 64, 64)
    dimgs = randn(np.random.default_rng(1), *imgs.shape).to(DEV)
    imgs.backward(dimgs)
    for p in range(2):
        src = b.unpack_src(rows)[p].clone().requires_grad_(True)
        tgt = b.xyz[int(b.cloud_row0_host[2 + p]):int(b.cloud_row0_host[2 + p]) + b.tgt_len[p]]
        one = net.generator(src, tgt)
        assert torch.equal(one, imgs[6 * p:6 * p + 6])
        one.backward(dimgs[6 * p:6 * p + 6])
        assert torch.equal(src.grad, b.unpack_src(pred.grad)[p])


def test_dem_path_one_step_single_view():
    ds = SyntheticDEM(2, 50, points=250)
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    net = net.to(DEV)
    torch.manual_seed(0)
    loss = AdversarialLoss().to(DEV)
    before_g = [p.detach().clone() for p in net.parameters()]
    before_d = [p.detach().clone() for p in loss.parameters()]
    opt_g, opt_d = FusedAdam(net.parameters(), lr=2e-4), FusedAdam(loss.parameters(), lr=1e-4, betas=(0.5, 0.999))
    mean, losses = train_epoch_gan(net, loss, opt_g, opt_d, [[ds[0], ds[1]]], dem_preparer(DEV), dem_real_rows)
    print("DEM step losses (point + 0.1 g, g, d): %s" % losses)
    assert losses.shape == (1, 3) and np.isfinite(losses).all()
    # a single view: B images per call, three passes
    assert all(int(loss.discriminator.main[k].num_batches_tracked) == 3 for k in (3, 6, 9))
    assert any(not torch.equal(a, b) for a, b in zip(before_g, net.parameters()))
    assert all(not torch.equal(a, b) for a, b in zip(before_d, loss.parameters()))
    assert all(torch.isfinite(p).all() for p in list(net.parameters()) + list(loss.parameters()))
