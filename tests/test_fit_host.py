"""The raw training data sources (scream_amd/data.py) and the import surface of the three training drivers.  No GPU."""
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

from scream_amd import synthetic
from scream_amd.data import RawPairFiles, SyntheticRawPairs


@pytest.fixture()
def small_synthetic(monkeypatch):
    monkeypatch.setattr(synthetic, "make_3dmatch_pair", functools.partial(synthetic.make_3dmatch_pair, n_samples=4000))
    monkeypatch.setattr(synthetic, "make_kitti_pair", functools.partial(synthetic.make_kitti_pair, n_rings=8, pts_per_ring=100))


def test_raw_pair_files_yield_the_raw_float64_items(tmp_path):
    rng = np.random.default_rng(0)
    want = []
    for i in range(3):
        src, tgt, T = rng.uniform(-3, 3, size=(40 + i, 3)), rng.uniform(-3, 3, size=(50 - i, 3)), np.eye(4)
        T[:3, 3] = rng.uniform(-1, 1, size=3)
        for k, a in (("src", src), ("tgt", tgt), ("T", T)):
            np.save(str(tmp_path / ("%s%d.npy" % (k, i))), a)
        want.append((src, tgt, T))
    ds = RawPairFiles(str(tmp_path))  # a training split has no info/: the pairs are counted by their files
    assert len(ds) == 3
    for i, w in enumerate(want):
        item = ds[i]
        assert len(item) == 3 and all(t.dtype == torch.float64 for t in item)
        assert all(np.array_equal(t.numpy(), a) for t, a in zip(item, w))  # raw: not normalised, not rounded
    os.makedirs(str(tmp_path / "info"))
    with open(str(tmp_path / "info" / "scene_names.txt"), "w") as f:
        f.write("7-scenes-redkitchen\n7-scenes-redkitchen\n")
    assert len(RawPairFiles(str(tmp_path))) == 2  # a test split: the count PairFileDataset uses
    batches = list(torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=list))
    assert [len(b) for b in batches] == [2, 1] and batches[0][1][0].shape == (41, 3)


@pytest.mark.parametrize("kind", ["3dmatch", "lo", "kitti"])
def test_synthetic_raw_pairs(kind, small_synthetic):
    ds = SyntheticRawPairs(kind, 2, seed0=5)
    assert len(ds) == 2
    src, tgt, T = ds[1]
    assert src.dtype == tgt.dtype == T.dtype == torch.float64 and src.shape[1] == 3 and tgt.shape[1] == 3 and T.shape == (4, 4)
    raw = synthetic.make_kitti_pair(6) if kind == "kitti" else synthetic.make_3dmatch_pair(6, kind)
    assert np.array_equal(src.numpy(), raw[0]) and np.array_equal(tgt.numpy(), raw[1]) and np.array_equal(T.numpy(), raw[2])
    with pytest.raises(IndexError):
        ds[2]
    with pytest.raises(ValueError):
        SyntheticRawPairs("kitty")


@pytest.mark.parametrize("name,path,lr,n_epochs,every", [("train_3d_match", "params/point-generator.pth", 0.0002, 45, 15),
                                                       ("train_kitti", "params/kitti-generator.pth", 0.00032, 120, 10),
                                                       ("train_open_gf", "params/dem-generator.pth", 0.0002, 45, 15)])
def test_drivers_keep_the_reference_surface_and_run_nothing_at_import(name, path, lr, n_epochs, every, capsys):
    drv = importlib.import_module(name)
    assert capsys.readouterr().out == ""
    assert (drv.generator_save_path, drv.lr_g, drv.epochs, drv.lr_update_epoch, drv.use_GAN) == (path, lr, n_epochs, every, False)
    assert not hasattr(drv, "net") and not hasattr(drv, "optimizer_G") and not hasattr(drv, "train_loader")
    assert all(callable(getattr(drv, f)) for f in ("update_lr", "evaluate", "train", "main"))
    p = torch.zeros(3, requires_grad=True)
    opt = torch.optim.SGD([p], lr=lr)
    try:
        drv.update_lr(opt, 0.5)  # the reference's update_lr: the module's lr_g, halved, into every group
        assert opt.param_groups[0]["lr"] == drv.lr_g == max(lr * 0.5, 1e-5)
    finally:
        drv.lr_g = lr
    with pytest.raises(SystemExit):
        drv.main(["--train-backend", "fp8"])


def test_the_training_entry_points_are_written_once():
    """The loaders, the command line, the optimiser and update_lr's loop stand in scream_amd/fit.py, not in the three drivers;
    render.py has one autograd Function for its one kernel pair; model.py has one constructor body and no forward body per
    mode."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = lambda *parts: open(os.path.join(repo, *parts)).read()
    for drv in ("train_3d_match.py", "train_kitti.py", "train_open_gf.py"):
        for needle in ("DataLoader(", "ArgumentParser(", "FusedAdam(", "param_groups"):
            assert needle not in text(drv), (drv, needle)
    render = text("scream_amd", "render.py")
    assert len(re.findall(r"^class \w+\(torch\.autograd\.Function\):", render, re.M)) == 1 and render.count("autograd.Function") == 1
    model = text("scream_amd", "model.py")
    assert model.count("nn.Conv1d(3, d_model") == 1
    assert not re.search(r"_forward_train|_forward_infer", model)
