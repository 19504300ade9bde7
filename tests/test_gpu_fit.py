"""The training loops of scream_amd/fit.py and the three root-level drivers on the MI355X, on (1, 1) models, clouds of 200 - 300
points and B = 2.  Run with `pytest -m gpu`."""
import functools
import importlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

import prep_ref as PR
from scream_amd import FusedAdam, _lib, synthetic
from scream_amd.evaluate_open_gf import SyntheticDEM
from scream_amd.fit import dem_preparer, fit, pair_preparer, train_epoch, val_loss
from scream_amd.model import DEMTransformer, PointTransformer
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


@functools.lru_cache(maxsize=None)
def raw_batches(seed0, n_batches, scale=1.0):
    """n_batches lists of two raw (src, tgt, T) float64 items, 200 - 300 points per cloud."""
    out = []
    for b in range(n_batches):
        items = []
        for i in range(2):
            k = seed0 + 2 * b + i
            src, tgt, T = PR.raw_pair(k, 200 + 37 * (k % 3), 300 - 29 * (k % 4))
            T = T.copy()
            T[:3, 3] *= scale
            items.append((torch.from_numpy(src * scale), torch.from_numpy(tgt * scale), torch.from_numpy(T)))
        out.append(items)
    return out


def point_net(seed=3, backend=None):
    net = PointTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(seed, 256, 1, 1))
    if backend:
        net.train_backend = backend
    return net.to(DEV)


def test_train_epoch_equals_the_hand_written_loop():
    batches = raw_batches(100, 2)
    net = point_net()
    opt = FusedAdam(net.parameters(), lr=2e-4)
    mean, losses = train_epoch(net, opt, batches, pair_preparer("3dmatch", True, DEV, seed=5))
    # the same by hand: same weights, same optimiser, same seeds
    net2 = point_net()
    opt2 = FusedAdam(net2.parameters(), lr=2e-4)
    prepare = pair_preparer("3dmatch", True, DEV, seed=5)
    by_hand = []
    net2.train()
    for raw in batches:
        prepared = prepare(raw)
        loss = net2.loss_packed(net2.forward_packed_train(prepared.batch), prepared)
        opt2.zero_grad()
        loss.backward()
        opt2.step()
        by_hand.append(loss.item())
    by_hand = np.array(by_hand, dtype=np.float32)
    assert losses.dtype == np.float32 and losses.shape == (2,) and np.isfinite(losses).all()
    assert np.array_equal(losses.view(np.uint32), by_hand.view(np.uint32)), (losses, by_hand)
    assert mean == float(by_hand.astype(np.float64).mean())
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(p, q)
    assert float(opt.state[next(net.parameters())]["step"]) == 2.0
    # and the validation loss: eval(), no_grad, the inference forward, the same accumulation
    v, per_batch = val_loss(net, batches, pair_preparer("3dmatch", False, DEV))
    assert not net.training and per_batch.shape == (2,) and v == float(per_batch.astype(np.float64).mean()) and np.isfinite(v)
    net2.eval()
    with torch.no_grad():
        prepared = pair_preparer("3dmatch", False, DEV)(batches[0])
        want = net2.loss_packed(net2.forward_packed(prepared.batch), prepared)
    assert float(want) == float(per_batch[0])


def test_fit_three_epochs_halves_the_rate_and_saves_on_improvement_only(tmp_path):
    train_b, val_b = raw_batches(200, 2), raw_batches(300, 1)
    net = point_net(4)
    opt = FusedAdam(net.parameters(), lr=2e-4)
    path = str(tmp_path / "params" / "point-generator.pth")
    with mock.patch("scream_amd.fit.torch.save", wraps=torch.save) as save:
        hist = fit(net, opt, train_b, val_b, pair_preparer("3dmatch", True, DEV, seed=1), pair_preparer("3dmatch", False, DEV), 4, path,
                   every=1, floor=5e-5, log=None)
    assert [h["epoch"] for h in hist] == [1, 2, 3]  # range(1, epochs), as the reference writes it
    assert [h["lr"] for h in hist] == [1e-4, 5e-5, 5e-5] and opt.param_groups[0]["lr"] == 5e-5  # halved down to the floor
    best, want = 1e8, []
    for h in hist:
        want.append(h["val_loss"] < best)
        best = min(best, h["val_loss"])
    assert [h["saved"] for h in hist] == want and hist[0]["saved"] and save.call_count == sum(want)
    assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    fresh = PointTransformer(256, 1, 1)
    fresh.load_state_dict(torch.load(path, map_location="cpu"))
    if hist[-1]["saved"]:  # the file is the final model: the same validation loss, bit for bit
        v, _ = val_loss(fresh.to(DEV), val_b, pair_preparer("3dmatch", False, DEV))
        assert v == hist[-1]["val_loss"]
    # a model that does not move does not improve: one checkpoint, at the first epoch
    still = point_net(4)
    frozen = FusedAdam(still.parameters(), lr=0.0)
    path2 = str(tmp_path / "frozen.pth")
    with mock.patch("scream_amd.fit.torch.save", wraps=torch.save) as save:
        hist = fit(still, frozen, train_b, val_b, pair_preparer("3dmatch", True, DEV, seed=1), pair_preparer("3dmatch", False, DEV), 4, path2,
                   every=100, log=None)
    assert [h["saved"] for h in hist] == [True, False, False] and save.call_count == 1 and os.path.exists(path2)
    assert hist[0]["val_loss"] == hist[1]["val_loss"] == hist[2]["val_loss"] and [h["lr"] for h in hist] == [0.0] * 3


@pytest.mark.parametrize("backend", ["split", "f32"])
def test_kitti_flavour_runs_under_a_grad_scaler(backend):
    batches = raw_batches(400, 2, scale=20.0)
    net = point_net(5, backend)
    before = [p.detach().clone() for p in net.parameters()]
    opt = FusedAdam(net.parameters(), lr=3.2e-4)
    scaler = torch.amp.GradScaler("cuda")
    mean, losses = train_epoch(net, opt, batches, pair_preparer("kitti", True, DEV, seed=2), scaler=scaler)
    assert np.isfinite(losses).all() and losses.shape == (2,)
    assert float(scaler.get_scale()) == 2.0 ** 16  # no step was skipped
    assert float(opt.state[next(net.parameters())]["step"]) == 2.0
    assert all(not torch.equal(p, q) and torch.isfinite(p).all() for p, q in zip(net.parameters(), before))
    # the logged loss is the unscaled one: the first step's equals that of the same epoch without a scaler
    net2 = point_net(5, backend)
    opt2 = FusedAdam(net2.parameters(), lr=3.2e-4)
    _, plain = train_epoch(net2, opt2, batches[:1], pair_preparer("kitti", True, DEV, seed=2))
    assert plain[0] == losses[0]


def test_dem_flavour_runs_on_synthetic_terrain():
    ds = SyntheticDEM(4, 50, points=250)
    batches = [[ds[0], ds[1]], [ds[2], ds[3]]]
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    net = net.to(DEV)
    before = [p.detach().clone() for p in net.parameters()]
    opt = FusedAdam(net.parameters(), lr=2e-4)
    prepare = dem_preparer(DEV)
    batch, target = prepare(batches[0])
    assert batch.n_pairs == 2 and target.shape == (batch.rows_src, 3)
    for t, it in zip(batch.unpack_src(target), batches[0]):
        assert torch.equal(t.cpu(), it[2])
    mean, losses = train_epoch(net, opt, batches, prepare)
    v, _ = val_loss(net, batches, prepare)
    assert np.isfinite(losses).all() and losses.shape == (2,) and np.isfinite(v) and mean == float(losses.astype(np.float64).mean())
    assert all(not torch.equal(p, q) for p, q in zip(net.parameters(), before))


def test_3dmatch_driver_evaluate_returns_the_loss_and_pose_errors_when_asked(monkeypatch):
    import train_3d_match as drv
    from scream_amd.data import SyntheticPairs, SyntheticRawPairs
    monkeypatch.setattr(synthetic, "make_3dmatch_pair", functools.partial(synthetic.make_3dmatch_pair, n_samples=6000))
    net = point_net(7)
    raw = SyntheticRawPairs("3dmatch", 2, 900)
    loader, prepare = [[raw[0], raw[1]]], pair_preparer("3dmatch", False, DEV)
    loss = drv.evaluate(net, loader, prepare)
    assert isinstance(loss, float) and np.isfinite(loss) and loss == val_loss(net, loader, prepare)[0]
    got = drv.evaluate(net, loader, prepare, metrics_items=SyntheticPairs("3dmatch", 2, 900))
    assert len(got) == 3 and got[0] == loss and all(isinstance(x, float) for x in got)  # (loss, mean RE, mean TE) of the pre-ICP pose


@pytest.mark.parametrize("name,model", [("train_3d_match", PointTransformer), ("train_kitti", PointTransformer), ("train_open_gf", DEMTransformer)])
def test_driver_trains_on_synthetic_data(name, model, tmp_path, monkeypatch):
    # smaller synthetic clouds than the generators' defaults: the drivers are what is tested here
    monkeypatch.setattr(synthetic, "make_3dmatch_pair", functools.partial(synthetic.make_3dmatch_pair, n_samples=6000))
    monkeypatch.setattr(synthetic, "make_kitti_pair", functools.partial(synthetic.make_kitti_pair, n_rings=16, pts_per_ring=200))
    saves = []
    with mock.patch("torch.save", side_effect=lambda *a, **k: saves.append(a)):
        drv = importlib.import_module(name)
    assert not saves and not hasattr(drv, "net") and not hasattr(drv, "optimizer_G")  # importing starts nothing
    assert (drv.use_GAN, drv.min_learning_rate, drv.learning_rate_decay_gamma) == (False, 1e-5, 0.5)
    assert all(callable(getattr(drv, f)) for f in ("update_lr", "evaluate", "train", "main"))
    path = str(tmp_path / "params" / os.path.basename(drv.generator_save_path))
    hist = drv.train(synthetic=4, batch=2, layers=(1, 1), n_epochs=3, save_path=path, device=DEV, log=None)
    assert [h["epoch"] for h in hist] == [1, 2] and hist[0]["saved"] and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    fresh = model(256, 1, 1)
    fresh.load_state_dict(torch.load(path, map_location="cpu"))
