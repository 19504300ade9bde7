"""Depth renderer on the MI355X (csrc/render.hip, scream_amd/render.py) against the float64 restatement of tests/render_ref.py:
images, argmax, the rules of include/scream_hip.h, batching, the backward, and both models with get_imgs=True (inference,
training, the reference's use_GAN loop).  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import render_ref as RR
from scream_amd import _lib, ops
from scream_amd.render import RegistrationRender, rotation_matrix, view_eulers
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def clouds(n, m, seed, lo=-0.9, hi=0.9):
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(n, 3, generator=g) * (hi - lo) + lo
    tgt = torch.rand(m, 3, generator=g) * (hi - lo) + lo
    return src.to(DEV), tgt.to(DEV)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.norm(a - b) / max(torch.linalg.norm(b).item(), 1e-300)).item()


def kernel_render(src, tgt, w=64, eulers=None, rho=24):
    """One pair through ops.render_depth: (imgs [V,2,w,w], argmax, rot)."""
    eulers = view_eulers("muti") if eulers is None else eulers
    rot = torch.stack([rotation_matrix(e) for e in eulers]).to(DEV)
    meta = torch.tensor([0, src.shape[0], 0, tgt.shape[0]], dtype=torch.int32, device=DEV)
    imgs, amax = ops.render_depth(src.contiguous(), meta[0:1], meta[1:2], tgt.contiguous(), meta[2:3], meta[3:4], src.shape[0],
                                  tgt.shape[0], rot, w, rho)
    return imgs[0], amax[0], rot


def check_images(src, tgt, w, eulers, imgs, amax):
    ref64, amax64, _, gap64 = RR.render(src.double(), tgt.double(), 24, w, eulers, dtype=torch.float64, top2=True)
    ref32 = RR.render(src, tgt, 24, w, eulers, dtype=torch.float32)[0]
    err = (imgs.double() - ref64).abs().max().item()
    err32 = (ref32.double() - ref64).abs().max().item()
    assert err <= max(2 * err32, 1e-6), (err, err32)
    sure = gap64 > 1e-5
    assert torch.equal(amax.long()[sure], amax64[sure])
    return sure.sum().item()


EULERS_CUSTOM = [np.array([0.3, -1.1, 2.0]), np.array([0.0, 0.0, np.pi / 4]), np.array([1.0, 0.5, -0.25])]


@pytest.mark.parametrize("n,m,w,views", [(1, 1, 64, "muti"), (700, 900, 64, "muti"), (700, 900, 128, "single"),
                                         (700, 900, 64, "custom"), (5000, 5000, 64, "muti"), (5000, 5000, 128, "muti"),
                                         (16000, 16000, 64, "single")])
def test_images_against_float64(n, m, w, views):
    src, tgt = clouds(n, m, seed=n + w)
    gen = RegistrationRender(24, w, view="single" if views == "single" else "muti")
    if views == "custom":
        gen.eulers = EULERS_CUSTOM  # reassigned after construction: the views follow at call time
    with torch.no_grad():
        imgs = gen(src, tgt)
    assert imgs.shape == (len(gen.eulers), 2, w, w) and imgs.dtype == torch.float32
    _, amax, _ = kernel_render(src, tgt, w, gen.eulers)
    assert torch.equal(kernel_render(src, tgt, w, gen.eulers)[0], imgs)
    checked = check_images(src, tgt, w, gen.eulers, imgs, amax)
    assert n == 1 or checked > 0.5 * imgs.numel()


def test_duplicated_points_lowest_index_wins_and_takes_all_the_gradient():
    src, tgt = clouds(300, 200, seed=5)
    src = torch.cat([src, src[:50]])  # rows 300..349 duplicate rows 0..49
    gen = RegistrationRender(24, 64)
    imgs, amax, _ = kernel_render(src, tgt)
    assert not ((amax[:, 0] >= 300) & (amax[:, 0] < 350)).any()
    assert (amax[:, 0] >= 0).any() and ((amax[:, 0] >= 0) & (amax[:, 0] < 50)).any()
    s = src.clone().requires_grad_(True)
    out = gen(s, tgt)
    up = torch.randn(out.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    g = torch.autograd.grad((out * up).sum(), s)[0]
    assert torch.equal(g[300:350], torch.zeros_like(g[300:350])) and g[:50].abs().sum() > 0


def test_flat_view_gives_nan_images_and_no_gradient():
    src, tgt = clouds(200, 150, seed=6)
    src[:, 2], tgt[:, 2] = 0.25, 0.25  # every depth equal in the identity view: dmax == dmin
    s = src.clone().requires_grad_(True)
    gen = RegistrationRender(24, 64, view="single")
    out = gen(s, tgt)
    assert torch.isnan(out).all()
    _, amax, _ = kernel_render(src, tgt, 64, gen.eulers)
    assert (amax == -1).all()
    g = torch.autograd.grad(out, s, grad_outputs=torch.ones_like(out))[0]
    assert torch.equal(g, torch.zeros_like(g))
    torch.cuda.synchronize()
    # the six-view renderer on the same clouds: only the identity and the 180 degree view about y are flat
    imgs = RegistrationRender(24, 64)(src, tgt)
    flat = [torch.isnan(imgs[v]).all().item() for v in range(6)]
    assert flat == [True, False, True, False, False, False]


def test_points_outside_the_grid_give_minus_one_and_no_argmax():
    src, tgt = clouds(300, 300, seed=7)
    src[:, :2] += 10.0
    tgt[:, :2] -= 10.0  # far outside [-1, 1]^2 in the identity view
    imgs, amax, _ = kernel_render(src, tgt, 64, view_eulers("single"))
    assert torch.equal(imgs, torch.full_like(imgs, -1.0)) and (amax == -1).all()


def test_batched_pairs_equal_single_pair_calls_bitwise():
    lens = [(900, 1200), (1, 5), (5000, 4100), (333, 64), (2048, 2049)]
    pairs = [clouds(n, m, seed=20 + i) for i, (n, m) in enumerate(lens)]
    eulers = view_eulers("muti")
    rot = torch.stack([rotation_matrix(e) for e in eulers]).to(DEV)
    # packed rows with gaps between the clouds (padding rows hold garbage the kernels must not read)
    s_parts, t_parts, s_row0, t_row0, r_s, r_t = [], [], [], [], 0, 0
    for (s, t) in pairs:
        s_row0.append(r_s)
        t_row0.append(r_t)
        s_parts += [s, torch.full((37, 3), 1e30, device=DEV)]
        t_parts += [t, torch.full((11, 3), -1e30, device=DEV)]
        r_s += s.shape[0] + 37
        r_t += t.shape[0] + 11
    S, T = torch.cat(s_parts), torch.cat(t_parts)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    s_len, t_len = [n for n, _ in lens], [m for _, m in lens]
    ws = ops.render_workspace(len(lens), 6, 64, S.shape[0], DEV)
    imgs, amax = ops.render_depth(S, i32(s_row0), i32(s_len), T, i32(t_row0), i32(t_len), max(s_len), max(t_len), rot, 64, 24, ws)
    up = torch.randn(imgs.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    dS = ops.render_depth_bwd(up, amax, S, i32(s_row0), i32(s_len), max(s_len), rot, 64, 24, ws)
    for i, (s, t) in enumerate(pairs):
        im1, am1, _ = kernel_render(s, t)
        assert torch.equal(imgs[i], im1) and torch.equal(amax[i], am1), i
        ws1 = ops.render_workspace(1, 6, 64, s.shape[0], DEV)
        meta = i32([0, s.shape[0], 0, t.shape[0]])
        ops.render_depth(s, meta[0:1], meta[1:2], t, meta[2:3], meta[3:4], s.shape[0], t.shape[0], rot, 64, 24, ws1)
        d1 = ops.render_depth_bwd(up[i:i + 1].contiguous(), am1[None].contiguous(), s, meta[0:1], meta[1:2], s.shape[0], rot, 64, 24, ws1)
        assert torch.equal(dS[s_row0[i]:s_row0[i] + s.shape[0]], d1), i
    pad = torch.ones(S.shape[0], dtype=torch.bool, device=DEV)
    for r, n in zip(s_row0, s_len):
        pad[r:r + n] = False
    assert torch.equal(dS[pad], torch.zeros_like(dS[pad]))


@pytest.mark.parametrize("n,m,w,view", [(700, 900, 64, "muti"), (5000, 5000, 64, "muti"), (2000, 1500, 128, "single")])
def test_backward_against_float64_and_repeatable(n, m, w, view):
    src, tgt = clouds(n, m, seed=40 + n)
    gen = RegistrationRender(24, w, view=view)
    s = src.clone().requires_grad_(True)
    out = gen(s, tgt)
    up = torch.randn(out.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    g1 = torch.autograd.grad((out * up).sum(), s)[0]
    out2 = gen(s, tgt)
    g2 = torch.autograd.grad((out2 * up).sum(), s)[0]
    assert torch.equal(out, out2) and torch.equal(g1, g2)  # bitwise repeatable
    _, amax, _ = kernel_render(src, tgt, w, gen.eulers)
    g64 = RR.backward(src.double(), tgt.double(), up, amax, 24, w, gen.eulers, dtype=torch.float64)
    g32 = RR.backward(src, tgt, up, amax, 24, w, gen.eulers, dtype=torch.float32)
    assert g64.abs().max() > 0
    assert rel(g1, g64) <= max(2 * rel(g32, g64), 1e-5), (rel(g1, g64), rel(g32, g64))


def test_target_that_requires_grad_is_refused():
    src, tgt = clouds(10, 10, seed=8)
    with pytest.raises(ValueError):
        RegistrationRender(24, 64)(src, tgt.requires_grad_(True))
    with torch.no_grad():
        RegistrationRender(24, 64)(src, tgt)  # no gradient is asked for: fine


def build_net(seed, ns=1, nc=1):
    from scream_amd.model import PointTransformer
    net = PointTransformer(256, ns, nc)
    net.load_state_dict(make_state_dict(seed, 256, ns, nc))
    return net.to(DEV)


def make_pair(seed, n, m):
    from scream_amd.synthetic import random_rotation
    rng = np.random.default_rng(seed)
    tgt = torch.from_numpy(rng.uniform(-0.7, 0.7, size=(1, m, 3)).astype(np.float32))
    rot = torch.from_numpy(random_rotation(rng, 30.0).astype(np.float32))[None]
    trans = torch.from_numpy(rng.uniform(-0.1, 0.1, size=(1, 3, 1)).astype(np.float32))
    src = ((tgt[:, :n] - trans.permute(0, 2, 1)) @ rot[0]).contiguous()  # rot src + trans == tgt[:n]
    return src, tgt, rot, trans


def test_models_return_images_at_inference():
    from scream_amd.model import DEMTransformer
    net = build_net(1).eval()
    src, tgt, rot, trans = (t.to(DEV) for t in make_pair(1, 400, 500))
    src_, imgs, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0, True, False)
    assert imgs.shape == (6, 2, 64, 64) and imgs.grad_fn is None
    src_b, none, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0, False, False)
    assert none is None and torch.equal(src_, src_b)  # get_imgs does not touch the prediction
    check_images(src_[0], tgt[0], 64, view_eulers("muti"), imgs, kernel_render(src_[0], tgt[0])[1])
    dem = DEMTransformer(256, 1, 1)
    dem.load_state_dict(make_state_dict(2, 256, 1, 1, dem=True))
    dem = dem.to(DEV)
    dem_, dimgs = dem(src, tgt, get_imgs=True)
    assert dimgs.shape == (1, 2, 64, 64) and dimgs.grad_fn is None
    check_images(dem_[0], tgt[0], 64, view_eulers("single"), dimgs, kernel_render(dem_[0], tgt[0], 64, view_eulers("single"))[1])
    assert torch.equal(dem(src, tgt)[0], dem_)


def _param_grads(net):
    return torch.cat([p.grad.detach().reshape(-1) for p in net.parameters()])


def test_training_images_carry_the_gradient_into_the_model():
    net = build_net(3)
    src, tgt, rot, trans = (t.to(DEV) for t in make_pair(3, 500, 600))
    net.train()
    src_, imgs, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0, True, False)
    assert imgs.grad_fn is not None and imgs.shape == (6, 2, 64, 64)
    up = torch.randn(imgs.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    g = torch.autograd.grad((imgs * up).sum(), src_, retain_graph=True)[0][0]
    amax = kernel_render(src_[0].detach(), tgt[0])[1]
    g64 = RR.backward(src_[0].detach().double(), tgt[0].double(), up, amax, dtype=torch.float64)
    g32 = RR.backward(src_[0].detach(), tgt[0], up, amax, dtype=torch.float32)
    assert rel(g, g64) <= max(2 * rel(g32, g64), 1e-5)
    # parameter gradients of point_loss + 0.1 g_loss == those of the two losses taken separately (one forward each: the
    # training graph of the model is freed by its backward)
    def grads(which):
        net.zero_grad(set_to_none=True)
        p_, im, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0, True, False)
        point_loss, g_loss = net.loss(p_, src, rot, trans), (im * up).mean()
        (point_loss * which[0] + 0.1 * g_loss * which[1]).backward()
        return _param_grads(net)

    both, only_point, only_img = grads((1, 1)), grads((1, 0)), grads((0, 1))
    assert only_img.abs().max() > 0
    assert rel(both, only_point + only_img) <= 1e-5


class _Conv(torch.nn.Module):
    """A stride-2 4 x 4 convolution as unfold + matmul (fixed-order arithmetic on the GPU)."""

    def __init__(self, cin, cout, gen):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(cout, cin * 16, generator=gen) * (1.0 / (cin * 16)) ** 0.5)
        self.b = torch.nn.Parameter(torch.zeros(cout))

    def forward(self, x):
        B, _, H, W = x.shape
        cols = F.unfold(x, 4, padding=1, stride=2)  # [B, cin*16, L]
        y = (self.w @ cols) + self.b[:, None]
        return y.view(B, -1, H // 2, W // 2)


def _gan_run():
    """train_3d_match.py:156-210 with use_GAN=True and a small discriminator on the renderer's 2 channels (the reference's
    AdversarialLoss declares input_nc=3, so its loop does not run as written; the discriminator is the user's module)."""
    torch.manual_seed(0)
    net = build_net(4)
    gen = torch.Generator().manual_seed(1)
    D = torch.nn.Sequential(_Conv(2, 8, gen), torch.nn.LeakyReLU(0.2), _Conv(8, 1, gen)).to(DEV)
    opt_g = torch.optim.Adam(net.parameters(), lr=1e-4)
    opt_d = torch.optim.Adam(D.parameters(), lr=1e-4)
    src, tgt, rot, trans = (t.to(DEV) for t in make_pair(4, 400, 500))
    src_real = (rot[0] @ src[0].T + trans[0]).T  # the ground-truth registration of the source
    losses = []
    for _ in range(3):
        net.train()
        src_pred, imgs, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0, True, False)
        point_loss = net.loss(src_pred, src, rot, trans)
        p = D(imgs)
        g_loss = F.mse_loss(p, torch.ones_like(p))
        opt_g.zero_grad()
        (point_loss + 0.1 * g_loss).backward()
        opt_g.step()
        real = net.generator(src_real, tgt[0].detach())
        assert real.grad_fn is None and real.shape == imgs.shape
        pr, pf = D(real), D(imgs.detach())
        d_loss = F.mse_loss(pr, torch.ones_like(pr)) + F.mse_loss(pf, torch.zeros_like(pf))
        opt_d.zero_grad()
        d_loss.backward()
        opt_d.step()
        losses.append((point_loss.item(), g_loss.item(), d_loss.item()))
    return losses, torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def test_reference_gan_loop_runs_and_repeats_bit_for_bit():
    a, pa = _gan_run()
    b, pb = _gan_run()
    assert all(np.isfinite(x) for row in a for x in row)
    assert a == b and torch.equal(pa, pb)
