"""The HIP Chamfer distance (csrc/chamfer.hip, scream_amd/chamfer.py) on the MI355X against the numpy restatement of its contract
(tests/chamfer_ref.py), bit for bit, at the smallest shapes where the scan can go wrong: one length below, at and above the
kernel's tile constants (1024 queries per block, 1024 targets per LDS tile, 256-row chunk sums, 64-row waves in the backward).
Run with `pytest -m gpu`."""
import functools
import math

import numpy as np
import pytest
import torch

import chamfer_ref as R
from scream_amd import ChamferDistance, _lib, chamfer_packed, ops
from scream_amd.evaluate_open_gf import SyntheticDEM, evaluate_samples
from scream_amd.fit import dem_preparer, dem_real_rows, pair_preparer, pair_real_rows, train_epoch
from scream_amd.model import DEMTransformer, PointTransformer
from scream_amd.optim import FusedAdam
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_RTOL = 6 * 2.0 ** -24  # five roundings of non-negative terms per distance (tests/test_chamfer_host.py)
LENGTHS = [(1, 1), (1, 7), (300, 1), (257, 130), (1024, 1024), (1025, 2049)]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


@functools.lru_cache(maxsize=None)
def cloud_pair(i):
    rng = np.random.default_rng(40 + i)
    N, M = LENGTHS[i]
    return rng.standard_normal((N, 3)).astype(np.float32) * np.float32(5), rng.standard_normal((M, 3)).astype(np.float32) * np.float32(5)


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


class Run:
    """One forward and one backward of the kernels over packed numpy clouds, every output on the host."""

    def __init__(self, a, a0, al, b, b0, bl, dout=1.0):
        ta, tb = dev(a).requires_grad_(), dev(b).requires_grad_()
        row = [dev(v, torch.int32) for v in (a0, al, b0, bl)]
        ma, mb = int(max(al)), int(max(bl))
        _, self.loss_pair_raw, idx_ab, d_ab, idx_ba, d_ba = ops.chamfer_fwd(ta.detach(), row[0], row[1], ma, tb.detach(), row[2], row[3], mb)
        loss, pairs = chamfer_packed(ta, row[0], row[1], tb, row[2], row[3], ma, mb, return_pairs=True)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
        assert pairs.dtype == torch.float64 and not pairs.requires_grad and torch.equal(pairs, self.loss_pair_raw)
        (loss * dout).backward()
        self.loss, self.loss_pair = loss.item(), pairs.cpu().numpy()
        self.idx_ab, self.d_ab, self.idx_ba, self.d_ba = (t.cpu().numpy() for t in (idx_ab, d_ab, idx_ba, d_ba))
        self.da, self.db = ta.grad.cpu().numpy(), tb.grad.cpu().numpy()

    def outputs(self):
        return (self.idx_ab, self.d_ab, self.idx_ba, self.d_ba, self.loss_pair, np.float32(self.loss), self.da, self.db)


def assert_is_the_restatement(got: Run, want):
    np.testing.assert_array_equal(got.idx_ab, want.idx_ab)
    np.testing.assert_array_equal(got.idx_ba, want.idx_ba)
    np.testing.assert_array_equal(got.d_ab.view(np.uint32), want.d_ab.view(np.uint32))
    np.testing.assert_array_equal(got.d_ba.view(np.uint32), want.d_ba.view(np.uint32))
    np.testing.assert_array_equal(got.loss_pair, want.loss_pair)
    assert np.float32(got.loss) == want.loss
    np.testing.assert_array_equal(got.da.view(np.uint32), want.da.view(np.uint32))
    np.testing.assert_array_equal(got.db.view(np.uint32), want.db.view(np.uint32))


def assert_pair_is_the_exact_sum(got: Run, a0, al, b0, bl):
    for p in range(len(al)):
        N, M = int(al[p]), int(bl[p])
        if N == 0 or M == 0:
            assert got.loss_pair[p] == 0
            continue
        exact = math.fsum(map(float, got.d_ab[a0[p]:a0[p] + N])) / N + math.fsum(map(float, got.d_ba[b0[p]:b0[p] + M])) / M
        assert abs(got.loss_pair[p] - exact) <= (N + M) * 2.0 ** -53 * exact


@functools.lru_cache(maxsize=None)
def alone(i):
    a, b = cloud_pair(i)
    N, M = LENGTHS[i]
    return Run(a, [0], [N], b, [0], [M]), R.chamfer(a, [0], [N], b, [0], [M])


@pytest.mark.parametrize("i", range(len(LENGTHS)))
def test_a_pair_alone_is_the_restatement_bit_for_bit(i):
    got, want = alone(i)
    N, M = LENGTHS[i]
    assert_is_the_restatement(got, want)
    assert_pair_is_the_exact_sum(got, [0], [N], [0], [M])
    again = Run(*cloud_pair(i)[:1], [0], [N], cloud_pair(i)[1], [0], [M])
    for x, y in zip(got.outputs(), again.outputs()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()  # two runs: the same bits


def test_six_pairs_in_one_packed_batch_match_the_pairs_alone():
    pa, a0, al = R.pack([cloud_pair(i)[0] for i in range(6)])
    pb, b0, bl = R.pack([cloud_pair(i)[1] for i in range(6)])
    got, want = Run(pa, a0, al, pb, b0, bl), R.chamfer(pa, a0, al, pb, b0, bl)
    assert_is_the_restatement(got, want)
    assert_pair_is_the_exact_sum(got, a0, al, b0, bl)
    for i, (N, M) in enumerate(LENGTHS):  # what else is in the batch changes nothing about a pair
        one = alone(i)[0]
        for x, y in ((got.idx_ab[a0[i]:a0[i] + N], one.idx_ab), (got.d_ab[a0[i]:a0[i] + N], one.d_ab),
                     (got.idx_ba[b0[i]:b0[i] + M], one.idx_ba), (got.d_ba[b0[i]:b0[i] + M], one.d_ba)):
            np.testing.assert_array_equal(x, y)
        assert got.loss_pair[i] == one.loss_pair[0]
    inside = np.zeros(pa.shape[0], dtype=bool)
    for r0, n in zip(a0, al):
        inside[r0:r0 + n] = True
    assert (got.idx_ab[~inside] == -1).all() and (got.d_ab[~inside] == 0).all() and (got.da[~inside] == 0).all()  # the 128-row padding
    again = Run(pa, a0, al, pb, b0, bl)
    for x, y in zip(got.outputs(), again.outputs()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_a_target_range_longer_than_one_lds_tile():
    """64 pairs with up to 2048 rows a side fill the 256 CUs with unsplit blocks (2 query blocks x 2 directions x 64), so every
    block walks two LDS tiles, the second one short; the pairs cycle over two distinct ones.  Were the launch heuristic to
    change, this would still pass and cover less."""
    rng = np.random.default_rng(7)
    base = [(rng.standard_normal((2048, 3)).astype(np.float32), rng.standard_normal((1030, 3)).astype(np.float32)),
            (rng.standard_normal((1500, 3)).astype(np.float32), rng.standard_normal((2047, 3)).astype(np.float32))]
    pa, a0, al = R.pack([base[p % 2][0] for p in range(64)])
    pb, b0, bl = R.pack([base[p % 2][1] for p in range(64)])
    got = Run(pa, a0, al, pb, b0, bl)
    for k in range(2):
        a, b = base[k]
        idx_ab, d_ab, idx_ba, d_ba = R.nearest(a, b)
        da, db = R.pair_grad(a, b, idx_ab, idx_ba, np.float64(1.0) / np.float64(64))
        for p in range(k, 64, 2):
            sa, sb = slice(a0[p], a0[p] + al[p]), slice(b0[p], b0[p] + bl[p])
            np.testing.assert_array_equal(got.idx_ab[sa], idx_ab)
            np.testing.assert_array_equal(got.idx_ba[sb], idx_ba)
            np.testing.assert_array_equal(got.d_ab[sa], d_ab)
            np.testing.assert_array_equal(got.d_ba[sb], d_ba)
            assert got.loss_pair[p] == R.pair_value(d_ab, d_ba)
            np.testing.assert_array_equal(got.da[sa], da)
            np.testing.assert_array_equal(got.db[sb], db)


def test_ties_go_to_the_lowest_row():
    """Clouds on an integer lattice with repeated rows: equal distances abound, across chunks of the scan, LDS tiles and blocks."""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 5, size=(1500, 3)).astype(np.float32)
    b = np.concatenate([rng.integers(0, 5, size=(1100, 3)).astype(np.float32), a[:200], a[:200]])
    got, want = Run(a, [0], [1500], b, [0], [1500]), R.chamfer(a, [0], [1500], b, [0], [1500])
    assert (want.d_ab == 0).sum() > 200 and len(set(want.idx_ab.tolist())) < 200  # many rows share few nearest rows
    assert_is_the_restatement(got, want)


def test_a_hub_row_collects_a_whole_cluster():
    """One row of a near a cluster of 1500 rows of b, the other rows of a far away: one segment of 1500 in the scatter term and
    many empty ones; and the same with the roles exchanged, as the second pair of the batch."""
    rng = np.random.default_rng(13)
    hub = (rng.standard_normal((300, 3)) + 100.0).astype(np.float32)
    hub[70] = np.float32(0.25)  # (inside the second wave of its block)
    cluster = (rng.standard_normal((1500, 3)) * 0.5).astype(np.float32)
    pa, a0, al = R.pack([hub, cluster])
    pb, b0, bl = R.pack([cluster, hub])
    got, want = Run(pa, a0, al, pb, b0, bl, dout=0.75), R.chamfer(pa, a0, al, pb, b0, bl, dout=0.75)
    assert (want.idx_ba[:1500] == 70).all() and (want.idx_ab[a0[1]:a0[1] + 1500] == 70).all()
    assert_is_the_restatement(got, want)


def test_a_cloud_against_itself_is_exactly_zero():
    a = cloud_pair(5)[1]
    got = Run(a, [0], [len(a)], a.copy(), [0], [len(a)])
    np.testing.assert_array_equal(got.idx_ab, np.arange(len(a)))
    np.testing.assert_array_equal(got.idx_ba, np.arange(len(a)))
    assert (got.d_ab == 0).all() and (got.d_ba == 0).all() and got.loss == 0 and got.loss_pair[0] == 0
    assert (got.da == 0).all() and (got.db == 0).all()


@pytest.mark.parametrize("side", ["a", "b"])
def test_an_empty_side_inside_a_batch(side):
    a, b = cloud_pair(3)
    a2, b2 = cloud_pair(1)
    empty = np.zeros((0, 3), dtype=np.float32)
    pa, a0, al = R.pack([a, empty if side == "a" else a2, a2])
    pb, b0, bl = R.pack([b, b2 if side == "a" else empty, b2])
    got, want = Run(pa, a0, al, pb, b0, bl), R.chamfer(pa, a0, al, pb, b0, bl)
    assert_is_the_restatement(got, want)
    assert got.loss_pair[1] == 0 and got.loss_pair[0] == alone(3)[0].loss_pair[0] and got.loss_pair[2] == alone(1)[0].loss_pair[0]
    other0, other_len = (b0, bl) if side == "a" else (a0, al)
    grad, idx = (got.db, got.idx_ba) if side == "a" else (got.da, got.idx_ab)
    rows = slice(other0[1], other0[1] + other_len[1])
    assert other_len[1] > 0 and (grad[rows] == 0).all() and (idx[rows] == -1).all()  # the rows facing the empty side
    np.testing.assert_array_equal(got.idx_ab[:len(a)], alone(3)[0].idx_ab)


@pytest.mark.parametrize("kind", ["shifted", "wide"])
def test_large_offsets_keep_the_value(kind):
    """sigma = 1 clouds shifted by 10^4, and sigma = 1000 clouds: the difference form stays within six fp32 roundings of the float64
    value of the same fp32 points.  The expansion -2ab + |a|^2 + |b|^2 of geometry.chamfer_distance does not: at an offset of 10^4
    its terms are 10^8 and one fp32 rounding of them is 8, against nearest-neighbour distances of about 0.1."""
    rng = np.random.default_rng(17)
    a, b = rng.standard_normal((257, 3)), rng.standard_normal((130, 3))
    a, b = ((a + 1e4, b + 1e4) if kind == "shifted" else (a * 1000, b * 1000))
    a, b = a.astype(np.float32), b.astype(np.float32)
    got = Run(a, [0], [257], b, [0], [130])
    d = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    exact = d.min(1).mean() + d.min(0).mean()
    print("%s: kernel %.17g  float64 %.17g  relative error %.3g x 2^-24" % (kind, got.loss_pair[0], exact, abs(got.loss_pair[0] - exact) / exact * 2 ** 24))
    assert abs(got.loss_pair[0] - exact) <= VALUE_RTOL * exact
    assert_is_the_restatement(got, R.chamfer(a, [0], [257], b, [0], [130]))


def test_the_module_has_the_references_shapes():
    rng = np.random.default_rng(21)
    f = dev(rng.standard_normal((3, 130, 3)).astype(np.float32)).requires_grad_()
    f_ = dev(rng.standard_normal((3, 257, 3)).astype(np.float32))
    loss = ChamferDistance()(f, f_)
    want = R.chamfer(f.detach().cpu().numpy().reshape(-1, 3), [0, 130, 260], [130] * 3, f_.cpu().numpy().reshape(-1, 3), [0, 257, 514], [257] * 3)
    assert loss.dtype == torch.float32 and np.float32(loss.item()) == want.loss
    assert want.loss == np.float32((want.loss_pair[0] + want.loss_pair[1] + want.loss_pair[2]) / 3)  # the mean of three packed pairs
    loss.backward()
    assert f.grad.shape == f.shape and f_.grad is None
    np.testing.assert_array_equal(f.grad.cpu().numpy().reshape(-1, 3), want.da)
    assert ChamferDistance()(torch.zeros(1, 0, 3, device=DEV), f_[:1]) == 0
    none = ChamferDistance()(f[:1].detach(), torch.zeros(1, 0, 3, device=DEV))  # an empty second cloud: the pair counts 0
    assert float(none) == 0


# ------------------------------------------------------------------------------ training
def _dem_case():
    ds = SyntheticDEM(2, 50, points=250)
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    return net.to(DEV), [[ds[0], ds[1]]], dem_preparer(DEV), dem_real_rows


def _pair_case():
    import prep_ref as PR
    items = []
    for k in (0, 1):
        src, tgt, T = PR.raw_pair(100 + k, 200 + 37 * k, 300 - 29 * k)
        items.append((torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(T)))
    net = PointTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(3, 256, 1, 1))
    return net.to(DEV), [items], pair_preparer("3dmatch", False, DEV), pair_real_rows


@pytest.mark.parametrize("case", [_dem_case, _pair_case], ids=["dem", "pairs"])
def test_training_with_the_chamfer_weight(case):
    from scream_amd.fit import _batch_of, _loss
    losses = {}
    for key, kw in (("plain", {}), ("zero", dict(chamfer_weight=0.0)), ("half", dict(chamfer_weight=0.5))):
        net, batches, prepare, real_rows = case()
        seen = {}
        fwd = net.forward_packed_train

        def recording_forward(batch, fwd=fwd, seen=seen):
            seen["pred"] = fwd(batch)
            seen["pred"].retain_grad()
            return seen["pred"]

        def recording_prepare(raw, prepare=prepare, seen=seen):
            seen["prepared"] = prepare(raw)
            return seen["prepared"]

        net.forward_packed_train = recording_forward
        if kw:
            kw["chamfer_rows"] = real_rows
        losses[key] = train_epoch(net, FusedAdam(net.parameters(), lr=2e-4), batches, recording_prepare, **kw)[1]
    assert losses["plain"].tobytes() == losses["zero"].tobytes()  # weight 0: bit for bit the call without the argument
    # the last run had weight 0.5: both losses again, separately, on the prediction it saw
    pred, prepared = seen["pred"], seen["prepared"]
    batch, rows = _batch_of(prepared), real_rows(prepared)
    p1, p2 = pred.detach().clone().requires_grad_(), pred.detach().clone().requires_grad_()
    l1, ch = _loss(net, p1, prepared), net.chamfer_packed_loss(p2, batch, rows)
    l1v, chv = float(l1.detach()), float(ch.detach())
    assert chv > 0 and losses["plain"][0] == np.float32(l1v)
    assert losses["half"][0] == np.float32(l1v + 0.5 * chv)  # one fp32 rounding of the sum
    l1.backward()
    (ch * 0.5).backward()
    assert torch.equal(pred.grad, (p1.grad.double() + p2.grad.double()).float())  # the two analytic gradients, one rounding
    n = [int(x) for x in batch.src_len]
    row0 = batch.src_row0.cpu().numpy()
    want = R.chamfer(pred.detach().cpu().numpy(), row0, n, rows.cpu().numpy(), row0, n, dout=0.5)
    assert np.float32(chv) == want.loss
    np.testing.assert_array_equal(p2.grad.cpu().numpy(), want.da)


def test_evaluate_samples_direct_takes_the_column_from_one_call():
    ds = SyntheticDEM(4, 50, points=300)
    samples = [ds[i] for i in range(4)]
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    net = net.to(DEV).eval()
    default, direct = evaluate_samples(net, samples), evaluate_samples(net, samples, chamfer="direct")
    assert default.shape == direct.shape == (4, 3) and np.array_equal(default[:, 1:], direct[:, 1:])  # the height columns: the same bits
    with torch.no_grad():
        preds = net.forward_batch([s[0].to(DEV) for s in samples], [s[1].to(DEV) for s in samples])
    for i, (p, s) in enumerate(zip(preds, samples)):
        P, D = p.cpu().numpy().astype(np.float64), s[2].numpy().astype(np.float64)
        d = ((P[:, None, :] - D[None, :, :]) ** 2).sum(-1)
        exact = (d.min(1).mean() + d.min(0).mean()) * 1000
        print("sample %d: direct %.10g  reference %.10g  float64 %.10g" % (i, direct[i, 0], default[i, 0], exact))
        assert abs(direct[i, 0] - exact) <= VALUE_RTOL * exact
    with pytest.raises(ValueError, match="chamfer"):
        evaluate_samples(net, samples, chamfer="fast")
