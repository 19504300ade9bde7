"""The Chamfer distance without a GPU: the numpy restatement (tests/chamfer_ref.py) against torch-CPU float64 autograd of the
reference's own five lines, its tie and empty-cloud rules, the header rules of the two entry points, and the drivers' --chamfer."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import chamfer_ref as R
from scream_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_RTOL = 6 * 2.0 ** -24   # five roundings of non-negative terms per distance, and the fp32 inputs are exact in float64
GRAD_RTOL = 2.0 ** -23        # relative to the sum of the absolute values of a row's terms


def reference_f64(f: torch.Tensor, f_: torch.Tensor) -> torch.Tensor:
    """evaluate_open_gf.py:25-41 with utils.square_distance (utils.py:72-78) written out, for [B,N,3] and [B,M,3]."""
    dist = -2 * torch.matmul(f, f_.permute(0, 2, 1))
    dist = dist + torch.sum(f ** 2, -1)[:, :, None]
    dist = dist + torch.sum(f_ ** 2, -1)[:, None, :]
    return torch.mean(torch.min(dist, dim=2)[0], dim=1).mean() + torch.mean(torch.min(dist, dim=1)[0], dim=1).mean()


# (N, M, sigma, seed): Gaussian clouds without ties whose fp32 and float64 arg-mins agree on every row (asserted below)
CLOUDS = [(2049, 1300, 5.0, 0), (257, 130, 1000.0, 1), (1, 7, 5.0, 2), (300, 1, 5.0, 3)]


def gaussian_pair(N, M, sigma, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, 3)) * sigma).astype(np.float32), (rng.standard_normal((M, 3)) * sigma).astype(np.float32)


@pytest.mark.parametrize("N,M,sigma,seed", CLOUDS)
def test_the_restatement_is_the_references_module_in_float64(N, M, sigma, seed):
    a, b = gaussian_pair(N, M, sigma, seed)
    A, B = a.astype(np.float64), b.astype(np.float64)
    d64 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    r = R.chamfer(a, [0], [N], b, [0], [M])
    # the arg-mins of the two precisions agree on every row, so value and gradient are comparable row by row
    np.testing.assert_array_equal(r.idx_ab, d64.argmin(1))
    np.testing.assert_array_equal(r.idx_ba, d64.argmin(0))
    fa, fb = torch.from_numpy(A)[None].requires_grad_(), torch.from_numpy(B)[None].requires_grad_()
    want = reference_f64(fa, fb)
    want.backward()
    w = float(want.detach())
    print("value: restatement %.17g  float64 %.17g  relative error %.3g x 2^-24" % (r.loss_pair[0], w, abs(r.loss_pair[0] - w) / w * 2 ** 24))
    assert abs(r.loss_pair[0] - w) <= VALUE_RTOL * w
    assert r.loss == np.float32(r.loss_pair[0])
    # sum of |terms| of a row's gradient: its own neighbour and everyone whose neighbour it is
    for got, g64, X, Y, ixy, iyx, nx, ny in ((r.da, fa.grad[0].numpy(), A, B, r.idx_ab, r.idx_ba, N, M),
                                             (r.db, fb.grad[0].numpy(), B, A, r.idx_ba, r.idx_ab, M, N)):
        terms = np.abs(X - Y[ixy]) * (2.0 / nx)
        np.add.at(terms, iyx, np.abs(X[iyx] - Y) * (2.0 / ny))
        err = np.abs(got.astype(np.float64) - g64)
        print("gradient: worst error / sum|terms| = %.3g x 2^-23" % ((err / np.maximum(terms, 1e-300)).max() * 2 ** 23))
        assert (err <= GRAD_RTOL * terms).all()


def test_equal_distances_go_to_the_lowest_index():
    """An integer lattice with repeated rows: every distance is exact, equal minima abound, and the index must be the lowest."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, size=(70, 3)).astype(np.float32)
    b = np.concatenate([rng.integers(0, 4, size=(50, 3)), a[:20].astype(np.int64), a[:20].astype(np.int64)]).astype(np.float32)
    idx_ab, d_ab, idx_ba, d_ba = R.nearest(a, b, block=16)  # (several row blocks: the strict < between blocks is exercised)
    d = ((a[:, None, :].astype(np.int64) - b[None, :, :].astype(np.int64)) ** 2).sum(-1)
    for n in range(a.shape[0]):
        assert idx_ab[n] == min(m for m in range(b.shape[0]) if d[n, m] == d[n].min()) and d_ab[n] == d[n].min()
    for m in range(b.shape[0]):
        assert idx_ba[m] == min(n for n in range(a.shape[0]) if d[n, m] == d[:, m].min()) and d_ba[m] == d[:, m].min()
    assert (np.bincount(idx_ab, minlength=90) > 1).any() and (d_ab[:20] == 0).all()
    # the scatter term is summed in ascending index: the restatement's loop against a float64 loop written the other way round
    # gives the same sums here only because lattice differences are exact
    da, db = R.pair_grad(a, b, idx_ab, idx_ba, np.float64(1.0))
    want = (a.astype(np.float64) - b[idx_ab]) * (2.0 / 70)
    for m in reversed(range(90)):
        want[idx_ba[m]] += (a[idx_ba[m]].astype(np.float64) - b[m]) * (2.0 / 90)
    np.testing.assert_allclose(da, want, rtol=2.0 ** -22, atol=0)


def test_an_empty_side_counts_zero_and_padding_rows_stay_out():
    a, b = gaussian_pair(40, 30, 1.0, 11)
    pa, a0, al = R.pack([a, a[:0], a[:5]])
    pb, b0, bl = R.pack([b, b, b[:0]])
    r = R.chamfer(pa, a0, al, pb, b0, bl)
    alone = R.chamfer(a, [0], [40], b, [0], [30])
    assert r.loss_pair[0] == alone.loss_pair[0] > 0 and r.loss_pair[1] == 0 and r.loss_pair[2] == 0
    assert r.loss == np.float32(alone.loss_pair[0] / 3)
    assert (r.idx_ab[40:] == -1).all() and (r.d_ab[40:] == 0).all() and (r.da[40:] == 0).all()
    assert (r.idx_ba[30:] == -1).all() and (r.db[30:] == 0).all()
    np.testing.assert_array_equal(r.idx_ab[:40], alone.idx_ab)
    da, db = R.pair_grad(a, b, alone.idx_ab, alone.idx_ba, np.float64(1.0) / np.float64(3.0))  # g = dout / n_pairs
    np.testing.assert_array_equal(r.da[:40], da)
    np.testing.assert_array_equal(r.db[:30], db)
    assert (r.db[128:128 + 30] == 0).all() and (r.da[256:256 + 5] == 0).all()  # the rows of the pairs with an empty side


def test_the_chunk_sum_is_sequential_not_pairwise():
    v = np.float32(1.0) + np.arange(1000, dtype=np.float32) * np.float32(1e-3)
    s = 0.0
    parts = []
    for c in range(0, 1000, 256):
        t = np.float64(v[c])
        for x in v[c + 1:c + 256]:
            t = t + np.float64(x)
        parts.append(t)
    for i, t in enumerate(parts):
        s = t if i == 0 else s + t
    assert R.cloud_sum(v) == s
    assert abs(R.cloud_sum(v) - math.fsum(float(x) for x in v)) <= 1000 * 2.0 ** -53 * s


# ------------------------------------------------------------------------------ the C ABI of the two entries
def test_the_header_declares_the_two_entries_without_a_sizer_or_a_struct():
    P = _lib.PROTOTYPES
    fwd, bwd = P["scream_chamfer_fwd"], P["scream_chamfer_bwd"]
    assert fwd.stream and bwd.stream and not any(n.startswith("scream_chamfer") and n.endswith("_bytes") for n in P)
    f = dict(zip(fwd.params, fwd.pointees))
    assert f["keys_a"] == f["keys_b"] == "uint64_t" and f["part"] == f["loss_pair"] == "double" and f["loss"] == "float"
    assert [k for k, v in f.items() if v == "int32_t"] == ["a_row0", "a_len", "b_row0", "b_len", "idx_ab", "idx_ba"]
    assert all(f[k] is None for k in ("a_rows", "max_a_len", "b_rows", "max_b_len", "n_pairs"))
    b = dict(zip(bwd.params, bwd.pointees))
    assert bwd.params[0] == "dout" and b["da"] == b["db"] == "float" and "workspace" not in b and "keys_a" not in b
    assert all(isinstance(v, (str, type(None))) for p in (fwd, bwd) for v in p.pointees)  # no struct
    src = open(os.path.join(REPO, "scream_amd", "csrc", "chamfer.hip")).read()
    assert "hipMemcpy" not in src and "Synchronize" not in src and "getenv" not in src and "align256(" not in src
    assert not re.search(r"atomic(Add|Exch|CAS|Max)|unsafeAtomic", src)  # the only atomic is the integer minimum of the keys
    from scream_amd import build
    assert build.SOURCES["chamfer.hip"] == ["-ffp-contract=off"]
    assert build.GATE["chamfer.hip"] == (False, ("chamfer_scan_kernel", "chamfer_bwd_kernel"))  # no scratch, checked at every build


def test_refused_arguments_come_back_as_codes_before_any_launch():
    lib = _lib.load()
    assert lib.scream_abi_version() == 21
    p = 4096  # a non-null, aligned address nobody dereferences: every refusal below happens on the host
    def fwd(a=p, a_rows=256, max_a=100, b=p, b_rows=256, max_b=100, n_pairs=2, keys_a=p, part=p, loss=p):
        return lib.scream_chamfer_fwd(a, p, p, a_rows, max_a, b, p, p, b_rows, max_b, n_pairs, keys_a, p, part, p, p, p, p, p, loss, None)
    def bwd(dout=p, a_rows=256, max_a=100, b_rows=256, max_b=100, n_pairs=2, idx_ab=p):
        return lib.scream_chamfer_bwd(dout, p, p, p, a_rows, max_a, p, p, p, b_rows, max_b, n_pairs, idx_ab, p, p, p, None)
    assert fwd(a=None) == fwd(b=None) == fwd(keys_a=None) == fwd(part=None) == fwd(loss=None) == -1
    assert fwd(n_pairs=0) == fwd(n_pairs=-1) == fwd(max_a=257) == fwd(max_b=257) == fwd(max_a=-1) == fwd(a_rows=-1) == -1
    assert fwd(a_rows=2 ** 31, max_a=100) == -1 and fwd(keys_a=p + 4) == fwd(part=p + 4) == -1
    assert fwd(n_pairs=65536) == -2
    assert bwd(dout=None) == bwd(idx_ab=None) == bwd(n_pairs=0) == bwd(max_a=257) == bwd(max_b=257) == bwd(b_rows=-1) == -1
    assert bwd(n_pairs=65536) == -2
    assert lib.scream_chamfer_fwd(*([None] * 3), 1, 1, *([None] * 3), 1, 1, 1, *([None] * 9), None) == -1


# ------------------------------------------------------------------------------ the training loops and the drivers
class _Net:
    """A stand-in model on the CPU: the loops only call these."""

    def __init__(self):
        self.w = torch.ones(3, requires_grad=True)
        self.chamfer_calls = 0

    def train(self):
        pass

    def eval(self):
        pass

    def forward_packed_train(self, batch):
        return batch * self.w

    forward_packed = forward_packed_train

    def loss_packed(self, pred, batch, target):
        return (pred - target).abs().sum()

    def chamfer_packed_loss(self, pred, batch, rows):
        self.chamfer_calls += 1
        return ((pred - rows) ** 2).sum()


def test_weight_zero_never_enters_the_chamfer_path_and_a_weight_adds_it():
    from scream_amd import fit
    net = _Net()
    opt = torch.optim.SGD([net.w], lr=0.0)
    x, t = torch.arange(6.0).reshape(2, 3), torch.ones(2, 3)
    prepare = lambda raw: (x, t)
    rows = lambda prepared: prepared[1] * 2
    base = fit.train_epoch(net, opt, [0, 1], prepare)[1]
    zero = fit.train_epoch(net, opt, [0, 1], prepare, chamfer_weight=0.0, chamfer_rows=rows)[1]
    assert net.chamfer_calls == 0 and base.tobytes() == zero.tobytes()
    assert fit.val_loss(net, [0], prepare, 0.0, rows)[1].tobytes() == fit.val_loss(net, [0], prepare)[1].tobytes() and net.chamfer_calls == 0
    half = fit.train_epoch(net, opt, [0, 1], prepare, chamfer_weight=0.5, chamfer_rows=rows)[1]
    assert net.chamfer_calls == 2
    l1, ch = float((x - t).abs().sum()), float(((x - 2 * t) ** 2).sum())
    assert half.tolist() == [np.float32(l1 + 0.5 * ch)] * 2 and base.tolist() == [np.float32(l1)] * 2
    assert fit.val_loss(net, [0], prepare, 0.5, rows)[1].tolist() == [np.float32(l1 + 0.5 * ch)]
    with pytest.raises(ValueError, match="chamfer_rows"):
        fit.train_epoch(net, opt, [0], prepare, chamfer_weight=0.5)
    for f in (fit.train_epoch, fit.train_epoch_gan, fit.val_loss, fit.fit):
        import inspect
        sig = inspect.signature(f).parameters
        assert sig["chamfer_weight"].default == 0.0 and sig["chamfer_rows"].default is None, f.__name__


@pytest.mark.parametrize("driver,real_rows", [("train_3d_match", "pair_real_rows"), ("train_kitti", "pair_real_rows"),
                                              ("train_open_gf", "dem_real_rows")])
def test_the_drivers_parse_chamfer_and_hand_fit_their_own_real_rows(driver, real_rows, monkeypatch):
    from scream_amd import fit
    mod = importlib.import_module(driver)
    seen = []
    monkeypatch.setattr(mod, "train", lambda *a, **k: seen.append(getattr(mod, "chamfer_weight", 0.0)))
    monkeypatch.setattr(mod, "chamfer_weight", 0.0, raising=False)
    mod.main(["--synthetic", "4"])
    mod.main(["--synthetic", "4", "--chamfer", "0.25"])
    assert seen == [0.0, 0.25]
    with pytest.raises(SystemExit):
        mod.main(["--chamfer", "-1"])
    with pytest.raises(SystemExit):
        mod.main(["--chamfer", "much"])
    # Driver.train hands fit() the weight and the driver's own ground-truth rows
    got = {}
    monkeypatch.setattr(fit, "fit", lambda *a, **k: got.update(k) or [])
    monkeypatch.setattr(fit, "DataLoader", lambda *a, **k: None)
    monkeypatch.setattr("scream_amd.optim.FusedAdam", lambda **k: None)
    model = lambda **k: type("N", (), {"to": lambda s, d: s, "parameters": lambda s: []})()
    for weight, want in ((None, 0.25), (0.75, 0.75)):
        mod._driver.train(model, lambda s: (None, None), lambda d: (None, None), device="cpu", chamfer_weight=weight, gan=False)
        assert got["chamfer_weight"] == want and got["chamfer_rows"].__name__ == real_rows and got["gan"] is None
    monkeypatch.setattr(mod, "chamfer_weight", 0.0)
    mod._driver.train(model, lambda s: (None, None), lambda d: (None, None), device="cpu", gan=False)
    assert got["chamfer_weight"] == 0.0


def test_the_reference_import_path_holds():
    import evaluate_open_gf
    from scream_amd import ChamferDistance, chamfer_packed  # noqa: F401
    import scream_amd
    assert evaluate_open_gf.ChamferDistance is ChamferDistance and issubclass(ChamferDistance, torch.nn.Module)
    assert {"chamfer_packed", "ChamferDistance"} <= set(scream_amd.__all__)
    assert ChamferDistance()(torch.zeros(1, 0, 3), torch.zeros(1, 5, 3)) == 0  # evaluate_open_gf.py:31-32, before anything runs
    with pytest.raises(_lib.ScreamHipError, match="on the GPU"):
        chamfer_packed(torch.zeros(4, 3), None, None, torch.zeros(4, 3), None, None, 4, 4)  # there is no CPU path
