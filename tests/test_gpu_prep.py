"""Batch preparation and the packed L1 loss on the MI355X (csrc/prep.hip, scream_amd/prep.py) against the float64 numpy
restatement of tests/prep_ref.py.  Without noise both sides are the same IEEE sequence, so every output is compared bit for bit;
with noise the device's log / sin / cos may differ from numpy's in the last bit, so fp32 outputs are equal or neighbours.  Run
with `pytest -m gpu`."""
import functools
import math

import numpy as np
import pytest
import torch

import prep_ref as PR
from scream_amd import _lib
from scream_amd.model import DEMTransformer, PointTransformer
from scream_amd.packing import PackedBatch
from scream_amd.prep import (PreparedPairs, packed_l1_loss, prepare_3dmatch_train, prepare_3dmatch_val, prepare_kitti_train,
                             prepare_kitti_val, prepare_pairs, sample_perturbations)
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RULES = ["mean", "trans", "neg_rt_trans"]
EDGE_LENS = [(2, 1000), (129, 256), (257, 255)]  # N, M from {2, 129, 255, 256, 257, 1000}: tile and chunk edges, mixed in one batch


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r != %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def adjacent(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    ok = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    assert ok.all(), "%s: %d of %d elements are not fp32 neighbours" % (what, (~ok).sum(), ok.size)


@functools.lru_cache(maxsize=None)
def edge_pairs(dtype):
    return [PR.raw_pair(60 + i, n, m, np.dtype(dtype).type) for i, (n, m) in enumerate(EDGE_LENS)]


def gpu_prepare(raws, **kw):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return prepare_pairs([to(r[0]) for r in raws], [to(r[1]) for r in raws], np.stack([r[2] for r in raws]), **kw)


def ref_prepare(raws, mode, center, perturb=None, side=None, noise_std=0.0, seed=0, sample_ids=None):
    B = len(raws)
    return [PR.prep_pair(r[0], r[1], r[2], None if perturb is None else perturb[i], 0 if side is None else side[i], noise_std, seed,
                         i if sample_ids is None else sample_ids[i], mode, RULES.index(center)) for i, r in enumerate(raws)]


def compare(prep, want, check, what):
    """Every output of a PreparedPairs against the per-pair restatement; check(got, want, what) for the fp32 ones."""
    B = len(want)
    xyz, row0 = PR.pack(want)
    b = prep.batch
    assert b.n_pairs == B and b.rows_total == xyz.shape[0] and b.rows_src == int(row0[B])
    assert np.array_equal(b.cloud_row0.cpu().numpy(), row0) and np.array_equal(b.cloud_row0_host, row0)
    assert np.array_equal(b.cloud_len.cpu().numpy(), [w["src_n"].shape[0] for w in want] + [w["tgt_n"].shape[0] for w in want])
    check(b.xyz, xyz, what + " xyz")
    pad = np.ones(xyz.shape[0], dtype=bool)
    for r, n in zip(row0, b.cloud_len_host):
        pad[r:r + n] = False
    assert not bits(b.xyz.cpu().numpy()[pad]).any(), what + ": a padding row is not exactly zero"
    check(b.center, np.concatenate([np.stack([w["center"] for w in want]), np.zeros((B, 3), dtype=np.float32)]), what + " center")
    check(prep.rot, np.stack([w["rot"] for w in want]), what + " rot")
    check(prep.trans, np.stack([w["trans"] for w in want]).reshape(B, 3, 1), what + " trans")
    return xyz, row0


# ---- 1. bit for bit without noise

@pytest.mark.parametrize("center", RULES)
@pytest.mark.parametrize("mode", ["ball", "bbox"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_prepare_pairs_bit_for_bit(dtype, mode, center):
    raws = edge_pairs(dtype)
    perturb, _ = sample_perturbations(3, 0.1, 5)
    for side in ([0, 1, 0], [1, 0, 1]):
        what = "%s %s %s sides %s" % (dtype, mode, center, side)
        prep = gpu_prepare(raws, mode=mode, center=center, perturb=perturb, side=side)
        want = ref_prepare(raws, mode, center, perturb, side)
        compare(prep, want, same_bits, what)
        same_bits(prep.s, np.array([w["s"] for w in want]), what + " s")
        same_bits(prep.c, np.stack([w["c"] for w in want]), what + " c")
        same_bits(prep.T_aug, np.stack([w["T_aug"] for w in want]), what + " T_aug")


def test_identity_perturbation_is_no_perturbation_and_feeds_the_model():
    raws = edge_pairs("float64")
    prep = gpu_prepare(raws, mode="ball", center="trans")
    same_bits(prep.T_aug, np.stack([r[2] for r in raws]), "T_aug without a perturbation")
    compare(prep, ref_prepare(raws, "ball", "trans"), same_bits, "no perturbation")
    net = PointTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(3, 256, 1, 1))
    net = net.to(DEV).train()
    pred = net.forward_packed_train(prep.batch)
    assert pred.shape == (prep.batch.rows_src, 3) and pred.grad_fn is not None and torch.isfinite(pred).all()
    for a, n in zip(prep.batch.unpack_src(pred), (2, 129, 257)):
        assert a.shape == (n, 3)


# ---- 2. batch independence, noise included

def test_a_pair_does_not_depend_on_its_batch():
    raws = edge_pairs("float32")
    perturb, side = sample_perturbations(3, 0.1, 8)
    kw = dict(mode="ball", center="mean", noise_std=0.003, seed=2 ** 40 + 5)
    full = gpu_prepare(raws, perturb=perturb, side=side, sample_ids=[3, 2 ** 35 + 7, 9], **kw)
    again = gpu_prepare(raws, perturb=perturb, side=side, sample_ids=[3, 2 ** 35 + 7, 9], **kw)
    for a, b in ((full.batch.xyz, again.batch.xyz), (full.trans, again.trans), (full.s, again.s)):
        assert torch.equal(a, b)
    for p in range(3):
        alone = gpu_prepare(raws[p:p + 1], perturb=perturb[p:p + 1], side=side[p:p + 1], sample_ids=[[3, 2 ** 35 + 7, 9][p]], **kw)
        n, m = EDGE_LENS[p]
        fb, ab = full.batch, alone.batch
        for cl_f, cl_a, k in ((p, 0, n), (3 + p, 1, m)):
            rf, ra = int(fb.cloud_row0_host[cl_f]), int(ab.cloud_row0_host[cl_a])
            same_bits(fb.xyz[rf:rf + k], ab.xyz[ra:ra + k].cpu().numpy(), "pair %d cloud %d" % (p, cl_a))
        for name in ("rot", "trans", "s", "c", "T_aug"):
            same_bits(getattr(full, name)[p], getattr(alone, name)[0].cpu().numpy(), "pair %d %s" % (p, name))
        same_bits(fb.center[p], ab.center[0].cpu().numpy(), "pair %d center" % p)
    other = gpu_prepare(raws, perturb=perturb, side=side, sample_ids=[3, 2 ** 35 + 8, 9], **kw)  # another sample id: another noise
    assert not torch.equal(other.batch.xyz, full.batch.xyz)


# ---- 3. noise against the restatement

@pytest.mark.parametrize("mode,center", [("ball", "trans"), ("bbox", "mean")])
def test_noise_against_the_restatement(mode, center):
    raws = edge_pairs("float64")
    perturb, side = sample_perturbations(3, 0.1, 21)
    kw = dict(perturb=perturb, side=side, noise_std=0.003, seed=77, sample_ids=[11, 2 ** 33, 5])
    prep = gpu_prepare(raws, mode=mode, center=center, **kw)
    want = ref_prepare(raws, mode, center, **kw)
    compare(prep, want, adjacent, "noise %s %s" % (mode, center))
    assert np.allclose(prep.s.cpu().numpy(), [w["s"] for w in want], rtol=1e-12, atol=0)
    assert np.allclose(prep.c.cpu().numpy(), np.stack([w["c"] for w in want]), rtol=0, atol=1e-12)
    same_bits(prep.T_aug, np.stack([w["T_aug"] for w in want]), "T_aug does not see the noise")


def test_noise_statistics():
    """One 30 000-row source: z = (noisy - clean) / (s std), taken in the metric frame (x / s + c of each preparation, because
    the noise moves c and s themselves), is standard normal: over n = 90 000 values the mean lies within 5 / sqrt n of zero and
    the variance within 5 sqrt(2 / n) of one.  The fp32 rounding of xyz is 6e-8 / s metres, 1e-4 of the 3 mm."""
    raw = [PR.raw_pair(91, 30000, 256, np.float32)]
    std = 0.003
    clean = gpu_prepare(raw, mode="ball", center="trans")
    noisy = gpu_prepare(raw, mode="ball", center="trans", noise_std=std, seed=1234, sample_ids=[42])
    metric = lambda p: p.batch.xyz[:30000].double().cpu().numpy() / float(p.s[0]) + p.c[0].cpu().numpy()
    z = ((metric(noisy) - metric(clean)) / std).reshape(-1)
    n = z.size
    assert n == 90000
    print("noise: mean %.5f (bound %.5f)  variance %.5f (bound 1 +- %.5f)" % (z.mean(), 5 / math.sqrt(n), z.var(), 5 * math.sqrt(2 / n)))
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    want = PR.gauss3(1234, 42, 0, 30000)
    assert np.abs(z.reshape(-1, 3) - want).max() <= 1e-3  # and it IS the contract's z, up to that rounding


# ---- 4. the packed loss

@functools.lru_cache(maxsize=None)
def loss_case():
    L = PR.loss_inputs()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pairs = L["pairs"]
    batch = PackedBatch.from_pairs([dev(p["src_n"]) for p in pairs], [dev(p["tgt_n"]) for p in pairs], [dev(p["trans"]) for p in pairs])
    assert np.array_equal(batch.xyz.cpu().numpy(), L["xyz"])
    B = len(pairs)
    prepared = PreparedPairs(batch, dev(L["rot"]), dev(L["trans"]).reshape(B, 3, 1), torch.tensor([p["s"] for p in pairs], device=DEV, dtype=torch.float64),
                             dev(np.stack([p["c"] for p in pairs])), dev(np.stack([p["T_aug"] for p in pairs])))
    return L, prepared, dev(L["pred"]), dev(L["target"])


def torch64_loss(L, form, pred64):
    """The reference's loss (models/pointnet.py:93-99 / 163-167) per pair in float64 torch on the same fp32 tensors."""
    out = []
    for p, n in enumerate(L["lens"]):
        sl = slice(int(L["row0"][p]), int(L["row0"][p]) + int(n))
        if form == "target":
            g = torch.from_numpy(L["target"][sl]).double()
        else:
            g = (torch.from_numpy(L["rot"][p]).double() @ torch.from_numpy(L["xyz"][sl]).double().T).T + torch.from_numpy(L["trans"][p]).double()
        out.append(torch.mean(torch.sum(torch.abs(pred64[sl] - g), dim=-1)))
    return torch.stack(out)


@pytest.mark.parametrize("form", ["rt", "target"])
def test_packed_l1_loss_forward_and_backward(form):
    L, prepared, pred, target = loss_case()
    pred = pred.clone().requires_grad_(True)
    if form == "target":
        loss, pair = packed_l1_loss(pred, prepared.batch, target=target, return_pairs=True)
        ref = PR.l1_pairs(L["pred"], L["lens"], L["row0"], target=L["target"])
    else:
        loss, pair = packed_l1_loss(pred, prepared, return_pairs=True)
        ref = PR.l1_pairs(L["pred"], L["lens"], L["row0"], xyz=L["xyz"], rot=L["rot"], trans=L["trans"])
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None and pair.dtype == torch.float64
    pred64 = torch.from_numpy(L["pred"]).double().requires_grad_(True)
    want_pair = torch64_loss(L, form, pred64)
    want = want_pair.mean()
    rel = abs(loss.item() - want.item()) / want.item()
    rel_pair = ((pair.cpu() - want_pair.detach()).abs() / want_pair.detach()).max().item()
    print("loss %s: %.9g against float64 %.17g, relative %.3g; per pair relative %.3g" % (form, loss.item(), want.item(), rel, rel_pair))
    assert rel <= 2.0 ** -22
    assert rel_pair <= 1e-12
    same_bits(loss, np.asarray(ref[0]), "loss against the restatement")
    same_bits(pair, ref[1], "per-pair losses against the restatement")
    # backward: the float64 autograd gradient rounded to fp32, exactly
    dout = 0.37
    (loss * dout).backward()
    (want * float(np.float32(dout))).backward()
    g64 = pred64.grad.numpy()
    got = pred.grad.cpu().numpy()
    d = np.zeros_like(g64)
    for p, n in enumerate(L["lens"]):
        d[int(L["row0"][p]):int(L["row0"][p]) + int(n)] = ref[2][p]
    real = np.zeros(len(d), dtype=bool)
    for p, n in enumerate(L["lens"]):
        real[int(L["row0"][p]):int(L["row0"][p]) + int(n)] = True
    keep = (np.abs(d) >= 1e-6) & real[:, None]
    assert (~keep[real]).mean() <= 0.001
    assert np.array_equal(bits(got[keep]), bits(g64.astype(np.float32)[keep]))
    assert not bits(got[~real]).any(), "a padding row has a gradient"
    same_bits(got, PR.l1_pairs_grad(np.float32(dout), ref[2], L["lens"], L["row0"], L["rows_src"]), "dpred against the restatement")


def test_packed_l1_loss_sign_of_zero_is_zero_and_dem_method():
    L, prepared, pred, target = loss_case()
    pred = target.clone()
    pred[5, 1] += 0.25
    pred.requires_grad_(True)
    net = DEMTransformer(256, 1, 1)
    loss = net.loss_packed(pred, prepared.batch, target)
    loss.backward()
    g = pred.grad
    assert g[5, 1].item() == np.float32(1.0 / (float(L["lens"][0]) * 3.0)) and g.count_nonzero().item() == 1
    assert abs(loss.item() - 0.25 / (L["lens"][0] * 3)) <= 1e-9
    with pytest.raises(_lib.ScreamHipError):
        packed_l1_loss(pred, prepared.batch)
    with pytest.raises(_lib.ScreamHipError):
        packed_l1_loss(pred[:-1], prepared)


# ---- 5. one optimiser step through the whole chain

def test_one_sgd_step_changes_every_parameter_and_repeats_bitwise():
    raws = [PR.raw_pair(70 + i, n, m, np.float32) for i, (n, m) in enumerate([(300, 450), (129, 257)])]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    srcs, tgts, Ts = [dev(r[0]) for r in raws], [dev(r[1]) for r in raws], [r[2] for r in raws]
    sd = make_state_dict(4, 256, 1, 1)
    runs = []
    for _ in range(2):
        net = PointTransformer(256, 1, 1)
        net.load_state_dict(sd)
        net = net.to(DEV).train()
        opt = torch.optim.SGD(net.parameters(), lr=0.05)
        prep = prepare_3dmatch_train(srcs, tgts, Ts, rng=31, seed=6, sample_ids=[100, 101])
        loss = net.loss_packed(net.forward_packed_train(prep.batch), prep)
        opt.zero_grad()
        loss.backward()
        opt.step()
        runs.append((loss.detach().cpu(), {k: v.detach().cpu().clone() for k, v in net.named_parameters()}))
    assert torch.isfinite(runs[0][0]) and torch.equal(runs[0][0], runs[1][0])
    for k, v in runs[0][1].items():
        assert torch.isfinite(v).all() and not torch.equal(v, sd[k].reshape(v.shape)), "%s did not move" % k
        assert torch.equal(v, runs[1][1][k]), "%s differs between two identical steps" % k


def test_presets():
    """The four presets are prepare_pairs under the reference's settings."""
    raws = edge_pairs("float64")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    srcs, tgts, Ts = [to(r[0]) for r in raws], [to(r[1]) for r in raws], np.stack([r[2] for r in raws])
    P, side = sample_perturbations(3, 0.1, 17)
    got = prepare_3dmatch_train(srcs, tgts, Ts, rng=17, seed=9)
    want = prepare_pairs(srcs, tgts, Ts, mode="ball", center="trans", perturb=P, side=side, noise_std=0.003, seed=9)
    assert torch.equal(got.batch.xyz, want.batch.xyz) and torch.equal(got.batch.center, want.batch.center) and torch.equal(got.T_aug, want.T_aug)
    Pk, sk = sample_perturbations(3, 0.1, 17, side="source")
    got = prepare_kitti_train(srcs, tgts, Ts, rng=17)
    want = prepare_pairs(srcs, tgts, Ts, mode="bbox", center="neg_rt_trans", perturb=Pk, side=sk)
    assert torch.equal(got.batch.xyz, want.batch.xyz) and torch.equal(got.batch.center, want.batch.center) and torch.equal(got.trans, want.trans)
    for fn, mode, center in ((prepare_3dmatch_val, "ball", "trans"), (prepare_kitti_val, "bbox", "neg_rt_trans")):
        got, want = fn(srcs, tgts, Ts), prepare_pairs(srcs, tgts, Ts, mode=mode, center=center)
        assert torch.equal(got.batch.xyz, want.batch.xyz) and torch.equal(got.batch.center, want.batch.center)
        assert torch.equal(got.T_aug, torch.from_numpy(Ts).to(DEV))
        on_dev = prepare_pairs(srcs, tgts, torch.from_numpy(Ts).to(DEV), mode=mode, center=center)  # T may live on the device
        assert torch.equal(on_dev.batch.xyz, want.batch.xyz) and torch.equal(on_dev.trans, want.trans)
    with pytest.raises(_lib.ScreamHipError):
        prepare_pairs([s.cpu() for s in srcs], tgts, Ts, mode="ball", center="trans")
    with pytest.raises(ValueError):
        prepare_pairs(srcs, tgts, Ts, mode="cube", center="trans")
