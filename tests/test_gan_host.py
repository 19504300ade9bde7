"""The host side of the adversarial loss (scream_amd/gan.py), without a GPU: tests/gan_ref.py -- the float64 oracle of
tests/test_gpu_gan.py -- against what the reference's own module recorded (tests/golden/gan.npz, tools/make_gan_golden.py) and,
where a reference checkout is present, against the live module; the state dict's names and shapes; every refusal with its
message; and the discriminator's optimiser settings as the drivers hand them over."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import gan_ref as G
from scream_amd import ScreamHipError, ops
from scream_amd.gan import AdversarialLoss, NLayerDiscriminator, g_loss, hinge_d_loss, weights_init

REF_GAN = os.path.join(os.environ.get("SCREAM_REFERENCE", "/root/reference"), "models", "gan.py")  # as tests/test_render_host.py
F64_TOL = 1e-12  # float64 rounding of sums of at most 16 * 64 products and 156 pixels, against tensors of order one


def _golden_state(g):
    return {k[len("code."):]: torch.from_numpy(float(g["offset." + k[len("code."):]]) + g[k].astype(np.float64) / 64.0)
            for k in g.files if k.startswith("code.")}


def _reference_module():
    if not os.path.exists(REF_GAN):
        pytest.skip("no reference checkout at %s" % os.path.dirname(os.path.dirname(REF_GAN)))
    spec = importlib.util.spec_from_file_location("reference_models_gan", REF_GAN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gan_ref_equals_the_reference_recording(golden):
    g = golden("gan")
    sd = _golden_state(g)
    x, dlogits = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["dlogits"]).double()
    fw = G.forward(x, sd)
    dx, grads = G.backward(fw, dlogits)
    figures = {"logits": G.max_rel(fw["logits"], torch.from_numpy(g["logits"])), "dx": G.max_rel(dx, torch.from_numpy(g["dx"]))}
    for name, t in grads.items():
        want = torch.from_numpy(g["grad." + name])  # the two largest are recorded at every 4th / 16th output channel
        figures["grad." + name] = G.max_rel(t[::t.shape[0] // want.shape[0]], want)
    for name, t in fw["running"].items():
        figures["after." + name] = G.max_rel(t, torch.from_numpy(g["after." + name]))
    print(figures)
    assert len(grads) == 13 and len(fw["running"]) == 6
    assert max(figures.values()) <= F64_TOL, figures
    assert all(int(g["after.main.%d.num_batches_tracked" % k]) == 1 for k in (3, 6, 9))
    assert tuple(fw["logits"].shape) == (2, 1, 1, 1) and [tuple(m.shape[2:]) for m in fw["masks"]] == [(12, 13), (6, 6), (3, 3), (2, 2)]


def test_gan_ref_masks_and_losses():
    rng = np.random.default_rng(5)
    real, fake = torch.from_numpy(rng.standard_normal((3, 1, 2, 3))), torch.from_numpy(rng.standard_normal((3, 1, 2, 3)))
    real.view(-1)[0], fake.view(-1)[0] = 1.0, -1.0  # exactly at the kinks: closed, gradient 0
    r, f = real.clone().requires_grad_(True), fake.clone().requires_grad_(True)
    want = 0.5 * (torch.relu(1.0 - r).mean() + torch.relu(1.0 + f).mean())
    want.backward()
    assert abs(G.d_loss(real, fake).item() - want.item()) < 1e-15
    dr, df = G.d_loss_grad(real, fake)
    assert torch.allclose(dr, r.grad, atol=1e-16) and torch.allclose(df, f.grad, atol=1e-16)
    assert dr.view(-1)[0] == 0 and df.view(-1)[0] == 0
    assert abs(G.g_loss(fake).item() + fake.mean().item()) < 1e-16 and torch.all(G.g_loss_grad(fake) == -1.0 / 18)
    # a mask from outside overrides the pass's own
    z = torch.tensor([[-1.0, 2.0]])
    assert torch.equal(G.leaky(z)[0], torch.tensor([[-0.2, 2.0]]))
    assert torch.equal(G.leaky(z, torch.tensor([[True, False]]))[0], torch.tensor([[-1.0, 0.4]]))


def test_gan_ref_equals_the_live_reference_module():
    ref = _reference_module()
    torch.manual_seed(3)
    net = ref.NLayerDiscriminator(input_nc=3, ndf=8, n_layers=3).apply(ref.weights_init).double().train()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(3, 3, 32, 40, dtype=torch.float64, requires_grad=True)
    logits = net(x)
    dlogits = torch.randn_like(logits)
    (logits * dlogits).sum().backward()
    fw = G.forward(x.detach(), sd)
    dx, grads = G.backward(fw, dlogits)
    assert G.max_rel(fw["logits"], logits) <= F64_TOL and G.max_rel(dx, x.grad) <= F64_TOL
    for name, p in net.named_parameters():
        assert G.max_rel(grads[name], p.grad) <= F64_TOL, name
    after = net.state_dict()
    for name, t in fw["running"].items():
        assert G.max_rel(t, after[name]) <= F64_TOL, name
    net.eval()
    with torch.no_grad():
        assert G.max_rel(G.forward(x.detach(), after, training=False)["logits"], net(x)) <= F64_TOL


SHAPES = {"main.0.weight": (64, 2, 4, 4), "main.0.bias": (64,), "main.2.weight": (128, 64, 4, 4), "main.5.weight": (256, 128, 4, 4),
          "main.8.weight": (512, 256, 4, 4), "main.11.weight": (1, 512, 4, 4), "main.11.bias": (1,)}
for _k, _c in ((3, 128), (6, 256), (9, 512)):
    SHAPES.update({"main.%d.weight" % _k: (_c,), "main.%d.bias" % _k: (_c,), "main.%d.running_mean" % _k: (_c,),
                   "main.%d.running_var" % _k: (_c,), "main.%d.num_batches_tracked" % _k: ()})


def test_state_dict_names_and_shapes():
    sd = NLayerDiscriminator().state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    assert list(sd) == (["main.0.weight", "main.0.bias", "main.2.weight"] + ["main.3." + n for n in bn] + ["main.5.weight"] +
                        ["main.6." + n for n in bn] + ["main.8.weight"] + ["main.9." + n for n in bn] + ["main.11.weight", "main.11.bias"])
    assert sd["main.3.num_batches_tracked"].dtype == torch.int64
    loss = AdversarialLoss()
    assert set(loss.state_dict()) == {"discriminator." + k for k in SHAPES}
    w = loss.discriminator.main[0].weight
    assert abs(w.std().item() - 0.02) < 0.005 and abs(loss.discriminator.main[3].weight.mean().item() - 1.0) < 0.01  # weights_init
    assert loss.adopt_weight(0.7, 5, threshold=10, value=0.1) == 0.1 and loss.adopt_weight(0.7, 15, threshold=10) == 0.7
    assert not hasattr(loss, "calculate_adaptive_weight")


def test_state_dict_interchanges_with_the_reference_both_ways():
    ref = _reference_module()
    for nc in (2, 3):
        theirs = ref.NLayerDiscriminator(input_nc=nc, ndf=32, n_layers=3).apply(ref.weights_init)
        ours = NLayerDiscriminator(input_nc=nc, ndf=32).apply(weights_init)
        assert list(ours.state_dict()) == list(theirs.state_dict())
        ours.load_state_dict(theirs.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), theirs.state_dict().values()))
        sd = {k: v + 1 for k, v in ours.state_dict().items()}
        theirs.load_state_dict(sd)
        assert all(torch.equal(theirs.state_dict()[k], v) for k, v in sd.items())
    # the same seed gives the reference's initial values: the holders are built in the reference's order
    torch.manual_seed(11)
    a = ref.NLayerDiscriminator(input_nc=2, ndf=32).state_dict()
    torch.manual_seed(11)
    b = NLayerDiscriminator(input_nc=2, ndf=32).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    # and weights_init draws what the reference's draws
    torch.manual_seed(12)
    a = ref.NLayerDiscriminator(input_nc=2, ndf=32).apply(ref.weights_init).state_dict()
    torch.manual_seed(12)
    b = NLayerDiscriminator(input_nc=2, ndf=32).apply(weights_init).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kwargs,limit", [(dict(n_layers=4), "n_layers == 3"), (dict(n_layers=2), "n_layers == 3"),
                                          (dict(use_actnorm=True), "use_actnorm"), (dict(ndf=48), "ndf % 32 == 0"),
                                          (dict(ndf=0), "ndf % 32 == 0"), (dict(input_nc=5), "1 <= input_nc <= 4"),
                                          (dict(input_nc=0), "1 <= input_nc <= 4")])
def test_unsupported_configurations_name_their_limit(kwargs, limit):
    with pytest.raises(NotImplementedError) as e:
        NLayerDiscriminator(**kwargs)
    assert limit in str(e.value)


def test_refusals_of_the_forward():
    dis = NLayerDiscriminator(ndf=32)
    for shape in ((2, 2, 23, 64), (2, 2, 64, 23)):
        with pytest.raises(ValueError, match="H and W >= 24"):
            dis(torch.zeros(shape))
    with pytest.raises(ValueError, match=r"\[n, 2, h, w\]"):
        dis(torch.zeros(2, 3, 64, 64))
    with pytest.raises(TypeError, match="fp32"):
        dis(torch.zeros(2, 2, 64, 64, dtype=torch.float64))
    with pytest.raises(ScreamHipError, match="no CPU path"):  # as the renderer refuses CPU tensors
        dis(torch.zeros(2, 2, 24, 24))
    with pytest.raises(ScreamHipError, match="no CPU path"):
        AdversarialLoss(ndf=32)(torch.zeros(6, 2, 64, 64), None, 0)
    with pytest.raises(ScreamHipError, match="no CPU path"):
        g_loss(torch.zeros(6, 1, 6, 6))
    with pytest.raises(ScreamHipError, match="no CPU path"):
        hinge_d_loss(torch.zeros(6, 1, 6, 6), torch.zeros(6, 1, 6, 6))
    with pytest.raises(ValueError, match="optimizer_idx"):
        AdversarialLoss(ndf=32)(torch.zeros(6, 2, 64, 64), None, 2)
    dis.eval()
    with pytest.raises(NotImplementedError, match="no_grad"):
        dis(torch.zeros(2, 2, 64, 64))
    # BatchNorm over a single value per channel, as torch refuses it
    c = torch.zeros(4)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.gan_bn_fwd(torch.zeros(1, 4, 1, 1), c, c, c, c, torch.zeros((), dtype=torch.int64))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        G.forward(torch.zeros(1, 2, 16, 16, dtype=torch.float64), {k: torch.zeros(v, dtype=torch.float64) for k, v in SHAPES.items()})


@pytest.mark.parametrize("driver,real_rows", [("train_3d_match", "pair_real_rows"), ("train_kitti", "pair_real_rows"),
                                              ("train_open_gf", "dem_real_rows")])
def test_the_drivers_hand_lr_d_and_the_betas_to_the_optimiser(driver, real_rows, monkeypatch):
    mod = importlib.import_module(driver)
    assert mod.use_GAN is False and mod.lr_d == 1e-4 and mod.discriminator_save_path == "params/discriminator.pth"
    gan = mod._gan("cpu")
    group, = gan.opt.param_groups
    assert type(gan.opt).__name__ == "FusedAdam" and group["lr"] == 1e-4 and tuple(group["betas"]) == (0.5, 0.999)
    assert [id(p) for p in group["params"]] == [id(p) for p in gan.loss.parameters()] and len(group["params"]) == 13
    assert gan.real_rows.__name__ == real_rows and gan.save_path == mod.discriminator_save_path and gan.g_weight == 0.1
    assert gan.loss.discriminator.input_nc == 2 and gan.loss.discriminator.ndf == 64
    # --gan turns use_GAN on; without the flag nothing changes
    seen = []
    monkeypatch.setattr(mod, "train", lambda *a, **k: seen.append(mod.use_GAN))
    monkeypatch.setattr(mod, "use_GAN", False)
    mod.main(["--synthetic", "4"])
    mod.main(["--synthetic", "4", "--gan"])
    assert seen == [False, True]
