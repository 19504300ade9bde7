"""train_backend = "bf16" on the MI355X (csrc/gemm_bf16.hip, scream_amd/train.py): ONE bf16 product per training GEMM with
fp32 accumulation.  The three kernels against float64 products of the ROUNDED operands (bf16 x bf16 is exact, so only the
accumulation order is left and the project's rule applies: <= max(2 x the fp32 CPU product of the same rounded operands, 5e-6)),
their scale invariance bit for bit, then whole models against the restated arithmetic of tests/bf16_ref.py under the GPU
pass's own masks, repeatability, the untouched "f32" / "split" arms, the mixed-precision loop, and two ways of dropping one
piece that the bar must see.  Every test prints its figures before it asserts.  Run with `pytest -m gpu`.

Measured on the MI355X: see DESIGN.md section 8, "One bf16 product per GEMM"."""
import functools

import numpy as np
import pytest
import torch

import bf16_ref as B
import train_ref as T
from scream_amd import FusedAdam, _lib, ops, train
from scream_amd.synthetic import make_state_dict
from train_ref import FLOOR, make_pair, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI_NONE, EPI_ELU1, EPI_RELU, EPI_BIAS_RELU = ops.EPI_NONE, ops.EPI_ELU1, ops.EPI_RELU, ops.EPI_BIAS_RELU
SHAPES = [(256, 256), (768, 256), (1024, 256), (256, 1024), (512, 256)]  # (N, K)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def operand(rng, rows, cols):
    """fp32 values over a 2^+-20 spread of magnitudes, every seventh one an exact bf16 tie (1 + odd 2^-8, scaled): the value
    whose rounding tells round-to-nearest-even from every other rounding."""
    x = rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-20, 21, size=(rows, cols)).astype(np.float64))
    tie = (1.0 + (2 * rng.integers(0, 64, size=(rows, cols)) + 1) * 2.0 ** -8) * np.exp2(rng.integers(-20, 21, size=(rows, cols)).astype(np.float64))
    flat = x.reshape(-1)
    flat[::7] = (tie.reshape(-1) * rng.choice([-1.0, 1.0], size=flat.shape))[::7]
    return torch.from_numpy(x.astype(np.float32))


def wide(t, extra=64, fill=7.0):
    """t as a column slice of a wider matrix (ld = columns + extra)."""
    w = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=t.dtype, device=t.device)
    w[:, :t.shape[1]] = t
    return w[:, :t.shape[1]]


def epilogue64(y, epi, n_act, bias):
    if epi == EPI_ELU1:
        y = y.clone()
        y[:, :n_act] = torch.nn.functional.elu(y[:, :n_act]) + 1
        return y
    if epi == EPI_RELU:
        return y.clamp_min(0)
    if epi == EPI_BIAS_RELU:
        return (y + bias.to(y.dtype)).clamp_min(0)
    return y


def held(what, got, want, cpu32):
    e, e32 = rel(got, want), rel(cpu32, want)
    print("%s: error %.3g, fp32 CPU product of the same rounded operands %.3g" % (what, e, e32))
    assert e <= max(2 * e32, FLOOR), (what, e, e32)


# ------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("M", [128, 384])
def test_forward_against_float64_of_the_rounded_operands(M):
    rng = np.random.default_rng(M)
    for N, K in SHAPES:
        A, W, bias = operand(rng, M, K), operand(rng, N, K), torch.from_numpy(rng.standard_normal(N).astype(np.float32))
        rA, rW = B.r(A), B.r(W)
        cases = [(EPI_NONE, 0), (EPI_RELU, 0), (EPI_BIAS_RELU, 0)] + ([(EPI_ELU1, 256)] if N == 768 else [(EPI_ELU1, N)])
        for epi, n_act in cases:
            want = epilogue64(rA.double() @ rW.double().t(), epi, n_act, bias)
            cpu32 = epilogue64(rA @ rW.t(), epi, n_act, bias)
            b = bias.to(DEV) if epi == EPI_BIAS_RELU else None
            got = ops.gemm_bf16(A.to(DEV), W.to(DEV), epi, n_act=n_act, bias=b)
            held("forward M %d N %d K %d epilogue %d" % (M, N, K, epi), got, want, cpu32)
            out = wide(torch.zeros(M, N, device=DEV))
            got2 = ops.gemm_bf16(wide(A.to(DEV)), W.to(DEV), epi, n_act=n_act, bias=b, out=out)
            assert torch.equal(got2, got), "lda / ldc wider than the matrix changed the result"
            assert (out._base[:, N:] == 7.0).all(), "the kernel wrote past the columns of C"
            assert torch.equal(ops.gemm_bf16(A.to(DEV), W.to(DEV), epi, n_act=n_act, bias=b), got)  # repeatable


@pytest.mark.parametrize("M", [128, 384])
def test_data_gradient_against_float64_of_the_rounded_operands(M):
    rng = np.random.default_rng(10 + M)
    for N, K in SHAPES:  # sums over N = 256, 768, 1024, 512 in one launch
        dY, W = operand(rng, M, N), operand(rng, N, K)
        dY[5] = 0.0
        dY[M - 128 + 100:] = 0.0  # padded rows
        rdY, rW = B.r(dY), B.r(W)
        got = ops.gemm_dgrad_bf16(dY.to(DEV), W.to(DEV))
        held("data gradient M %d N %d K %d" % (M, N, K), got, rdY.double() @ rW.double(), rdY @ rW)
        assert (got[5] == 0).all() and (got[M - 128 + 100:] == 0).all(), "padded rows must give zero data gradient"
        out = wide(torch.zeros(M, K, device=DEV))
        got2 = ops.gemm_dgrad_bf16(wide(dY.to(DEV)), W.to(DEV), out=out)
        assert torch.equal(got2, got) and (out._base[:, K:] == 7.0).all()
        assert torch.equal(ops.gemm_dgrad_bf16(dY.to(DEV), W.to(DEV)), got)


@pytest.mark.parametrize("rows", [0, 1, 31, 32, 33, 128, 300, 9000])
def test_weight_gradient_against_float64_of_the_rounded_operands(rows):
    rng = np.random.default_rng(20 + rows)
    shapes = [(256, 256), (768, 256)] + ([(1024, 256), (256, 1024)] if rows in (33, 300) else [])
    for N, K in shapes:
        dW, cs = torch.full((N, K), 3.0, device=DEV), torch.full((N,), 3.0, device=DEV)
        if rows == 0:  # an empty sum over rows that are there but not counted
            train.wgrad_bf16(operand(rng, 128, N).to(DEV), operand(rng, 128, K).to(DEV), dW, cs, rows=0)
            assert (dW == 0).all() and (cs == 0).all()
            continue
        dY, X = operand(rng, rows, N), operand(rng, rows, K)
        rdY, rX = B.r(dY), B.r(X)
        want, cpu32 = rdY.double().t() @ rX.double(), rdY.t() @ rX
        train.wgrad_bf16(dY.to(DEV), X.to(DEV), dW, cs)
        held("weight gradient rows %d N %d K %d" % (rows, N, K), dW, want, cpu32)
        ec = rel(cs, dY.double().sum(0))  # the column sums are fp32 sums of the UNROUNDED dY
        print("colsum error", ec)
        assert ec <= FLOOR
        # without colsum, accumulating, strided
        dW2 = dW.clone()
        train.wgrad_bf16(wide(dY.to(DEV)), wide(X.to(DEV), 128), dW2, accumulate=True, ldy=N + 64, ldx=K + 128)
        first = torch.empty(N, K, device=DEV)
        train.wgrad_bf16(dY.to(DEV), X.to(DEV), first)
        assert torch.equal(first, dW), "colsum changed dW"
        assert torch.equal(dW2, dW + dW), "accumulate / ldy / ldx: dW + the same product"
        cs2 = cs.clone()
        train.wgrad_bf16(dY.to(DEV), X.to(DEV), dW2, cs2, accumulate=True)
        assert torch.equal(cs2, cs + cs)


def test_a_power_of_two_comes_out_bit_for_bit():
    """bf16 rounding and fp32 accumulation are exponent-blind while everything stays normal: |values| in [2^-10, 1], so products
    are >= 2^-20 (2^-50 at the scale 2^-30) and sums of <= 1300 of them < 2^11 (2^51 at 2^40)."""
    rng = np.random.default_rng(7)
    mag = lambda *shape: torch.from_numpy((rng.choice([-1.0, 1.0], size=shape) * np.exp2(-10.0 * rng.uniform(size=shape))).astype(np.float32)).to(DEV)
    M, N, K, rows = 384, 768, 256, 1300
    A, W, dY, dYr, X = mag(M, K), mag(N, K), mag(M, N), mag(rows, N), mag(rows, K)
    fwd, dg = ops.gemm_bf16(A, W), ops.gemm_dgrad_bf16(dY, W)
    dW, cs = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    train.wgrad_bf16(dYr, X, dW, cs)
    for e in (16, -30, 40):
        s = 2.0 ** e
        dWs, css = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        train.wgrad_bf16(dYr * s, X, dWs, css)
        same = [torch.equal(ops.gemm_bf16(A * s, W), fwd * s), torch.equal(ops.gemm_dgrad_bf16(dY * s, W), dg * s),
                torch.equal(dWs, dW * s), torch.equal(css, cs * s)]
        print("scale 2^%d: forward, data gradient, weight gradient, colsum equal:" % e, same)
        assert torch.isfinite(dWs).all() and all(same), (e, same)


# ------------------------------------------------------------------------------------- models
def point_net(sd, ns, nc, backend="bf16"):
    from scream_amd.model import PointTransformer
    net = PointTransformer(256, ns, nc)
    net.load_state_dict(sd)
    net.train_backend = backend
    return net.to(DEV)


def restated(grads_fn, sd, samples, masks, **mode):
    """(g64r, g32r): the float64 and the fp32 restatement under `masks`.  A batch takes ONE backward of the mean loss
    (bf16_ref.point_batch_grads says why: 1 / 3 does not commute with the rounding of the gradients)."""
    with B.rounded_gemms(**mode):
        if len(samples) > 1:
            assert grads_fn is T.oracle_grads
            return [B.point_batch_grads(sd, samples, dtype, masks) for dtype in (torch.float64, torch.float32)]
        return T.masked_oracles(grads_fn, sd, samples, masks)


@functools.lru_cache(maxsize=None)
def point_case(ns, nc, sizes):
    """One GPU pass of a (ns, nc) PointTransformer over the pairs of `sizes` and the restatements under its masks, shared by
    the tests below (never modified)."""
    sd = make_state_dict(50 + ns, 256, ns, nc)
    pairs = [make_pair(60 + i, n, m) for i, (n, m) in enumerate(sizes)]
    net = point_net(sd, ns, nc)
    loss, g, masks = T.point_gpu(net, pairs, DEV)
    g64r, g32r = restated(T.oracle_grads, sd, pairs, masks)
    return sd, pairs, net, loss, g, masks, g64r, g32r


def report_unrounded(what, grads_fn, sd, samples, masks, g):
    g64 = {k: sum(grads_fn(sd, *s, torch.float64, masks=m)[1][k] for s, m in zip(samples, masks)) / len(samples) for k in sd}
    far = [rel(g[k], g64[k]) for k in g64 if g64[k].abs().max() > 0]
    print("%s against the UNROUNDED float64 oracle under the same masks (reported, not held): %.2g .. %.2g" % (what, min(far), max(far)))


@pytest.mark.parametrize("ns,nc,sizes", [pytest.param(1, 1, ((300, 280),), id="1-1"), pytest.param(2, 2, ((129, 127),), id="2-2"),
                                         pytest.param(1, 1, ((150, 260), (129, 100), (40, 131)), id="1-1-ragged-three-pairs")])
def test_model_gradients_against_the_restated_arithmetic(ns, nc, sizes):
    sd, pairs, net, loss, g, masks, g64r, g32r = point_case(ns, nc, sizes)
    assert len(g) == len(sd) and all(torch.isfinite(v).all() for v in g.values())
    what = "bf16 (%d,%d) %d pair(s)" % (ns, nc, len(pairs))
    report_unrounded(what, T.oracle_grads, sd, pairs, masks, g)
    bad = T.rule(what, g, g64r, g32r)
    assert not bad, bad


def test_dem_gradients_against_the_restated_arithmetic():
    from scream_amd.model import DEMTransformer
    sd = make_state_dict(71, 256, 1, 1, dem=True)
    sample = T.terrain(3, 300)
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(sd)
    net.train_backend = "bf16"
    net = net.to(DEV).train()
    loss, g, masks = T.dem_gpu(net, [sample], DEV)
    T.assert_bitwise("forward_saving + backward against net(...); loss.backward()", g, T.dem_module_grads(net, *sample, DEV)[1])
    g64r, g32r = restated(T.dem_oracle_grads, sd, [sample], masks)
    report_unrounded("bf16 DEM (1,1)", T.dem_oracle_grads, sd, [sample], masks, g)
    bad = T.rule("bf16 DEM (1,1)", g, g64r, g32r)
    assert not bad, bad


# ------------------------------------------------------------------------------------- compatibility, repeatability
def test_module_path_two_passes_and_a_loss_scale_are_bitwise():
    sd, pairs, net, loss, g, masks, _, _ = point_case(1, 1, ((300, 280),))
    T.assert_bitwise("forward_saving + backward against net(...); loss.backward()", g, T.point_module_grads(net, *pairs[0], DEV)[1])
    loss2, g2, _ = T.point_gpu(net, pairs, DEV)
    assert loss2 == loss
    T.assert_bitwise("two passes", g, g2)
    # loss x 2^16: every gradient x 2^16, bit for bit
    from scream_amd.packing import PackedBatch
    d = [t.to(DEV) for t in pairs[0]]
    batch = PackedBatch.from_pairs([d[0][0]], [d[1][0]], [d[3].reshape(3)])
    _, gs, _, _ = T.gpu_pass(net, batch, lambda preds: net.loss(preds[0][None], d[0], d[2], d[3]) * 65536.0)
    for k in g:
        assert torch.isfinite(gs[k]).all() and torch.equal(gs[k], g[k] * 65536.0), "gradient of %s is not the unscaled one x 2^16" % k


def test_f32_and_split_are_bitwise_what_they_were():
    sd = make_state_dict(52, 256, 1, 1)
    pair = make_pair(61, 200, 260)
    net = point_net(sd, 1, 1, "f32")
    before = {}
    for backend in ("f32", "split"):
        net.train_backend = backend
        before[backend] = T.point_module_grads(net, *pair, DEV)
    net.train_backend = "bf16"
    _, gb = T.point_module_grads(net, *pair, DEV)
    assert any(not torch.equal(gb[k], before["f32"][1][k]) for k in gb)  # another arithmetic did run
    for backend in ("f32", "split"):
        net.train_backend = backend
        loss, g = T.point_module_grads(net, *pair, DEV)
        assert loss == before[backend][0]
        T.assert_bitwise("%s after a bf16 pass" % backend, g, before[backend][1])


def test_five_steps_under_a_grad_scaler():
    """The reference's mixed-precision loop (train_kitti.py:150-188) through fit.train_epoch: FusedAdam, a GradScaler at 2^16."""
    import prep_ref as PR
    from scream_amd.fit import pair_preparer, train_epoch
    items = []
    for k in (0, 1):
        src, tgt, Tm = PR.raw_pair(500 + k, 220 + 30 * k, 280 - 20 * k)
        Tm = Tm.copy()
        Tm[:3, 3] *= 20.0
        items.append((torch.from_numpy(src * 20.0), torch.from_numpy(tgt * 20.0), torch.from_numpy(Tm)))
    net = point_net(make_state_dict(5, 256, 1, 1), 1, 1)
    opt = FusedAdam(net.parameters(), lr=3.2e-4)
    scaler = torch.amp.GradScaler("cuda")
    _, losses = train_epoch(net, opt, [items] * 5, pair_preparer("kitti", False, DEV), scaler=scaler)
    print("losses", losses, "scale", float(scaler.get_scale()))
    assert float(scaler.get_scale()) == 2.0 ** 16, "the scaler saw inf / NaN gradients and backed off"
    assert float(opt.state[next(net.parameters())]["step"]) == 5.0
    assert np.isfinite(losses).all() and all(torch.isfinite(p).all() for p in net.parameters())
    assert losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------- drop one piece: the bar sees it
@pytest.mark.parametrize("drop", ["x", "w", "dy"])
def test_a_restatement_without_one_rounding_is_over_the_bar(drop):
    sd, pairs, net, loss, g, masks, _, _ = point_case(1, 1, ((300, 280),))
    g64d, g32d = restated(T.oracle_grads, sd, pairs, masks, drop=(drop,))
    bad = T.rule("bf16 (1,1) against a restatement that leaves %s unrounded" % drop, g, g64d, g32d)
    assert bad, "the bar does not see a missing rounding of %s" % drop


def test_one_gemm_on_the_f32_path_is_over_the_bar(monkeypatch):
    sd, pairs, net, loss, g, masks, _, _ = point_case(1, 1, ((300, 280),))
    plain = train.Bf16Gemms.fwd

    def fwd(self, A, W, epilogue=EPI_NONE, n_act=0, bias=None):
        if W.shape[0] == 1024:  # the FFN's first product of every block
            return ops.gemm_f32(A, W, epilogue, n_act=n_act, bias=bias)
        return plain(self, A, W, epilogue, n_act=n_act, bias=bias)

    monkeypatch.setattr(train.Bf16Gemms, "fwd", fwd)
    _, g1, masks1 = T.point_gpu(point_net(sd, 1, 1), pairs, DEV)
    g64r, g32r = restated(T.oracle_grads, sd, pairs, masks1)
    bad = T.rule("bf16 (1,1) with mlp.0 on the fp32 path", g1, g64r, g32r)
    assert bad, "the bar does not see one GEMM in another arithmetic"


# ------------------------------------------------------------------------------------- the loops that only consume gradients
def test_the_gan_loop_and_the_rendered_views_train_on_it():
    """fit.train_epoch_gan on both models: the adversarial loss differentiates the rendered views (get_imgs) into the
    prediction, and the bf16 backward takes that gradient like any other.  Two steps under a GradScaler repeat bit for bit."""
    import prep_ref as PR
    from scream_amd.evaluate_open_gf import SyntheticDEM
    from scream_amd.fit import dem_preparer, dem_real_rows, pair_preparer, pair_real_rows, train_epoch_gan
    from scream_amd.gan import AdversarialLoss
    from scream_amd.model import DEMTransformer
    batches = [[tuple(torch.from_numpy(a) for a in PR.raw_pair(700 + 2 * b + i, 200 + 30 * i, 280 - 25 * i)) for i in range(2)] for b in range(2)]
    runs = []
    for _ in range(2):
        net = point_net(make_state_dict(3, 256, 1, 1), 1, 1)
        torch.manual_seed(0)
        loss = AdversarialLoss().to(DEV)
        opt_g, opt_d = FusedAdam(net.parameters(), lr=2e-4), FusedAdam(loss.parameters(), lr=1e-4, betas=(0.5, 0.999))
        scaler = torch.amp.GradScaler("cuda")
        _, losses = train_epoch_gan(net, loss, opt_g, opt_d, batches, pair_preparer("3dmatch", True, DEV, seed=5), pair_real_rows, scaler=scaler)
        assert losses.shape == (2, 3) and np.isfinite(losses).all() and float(scaler.get_scale()) == 2.0 ** 16
        runs.append([p.detach().clone() for p in net.parameters()])
    assert all(torch.equal(p, q) and torch.isfinite(p).all() for p, q in zip(*runs))
    ds = SyntheticDEM(2, 50, points=250)
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    net.train_backend = "bf16"
    net = net.to(DEV)
    before = [p.detach().clone() for p in net.parameters()]
    torch.manual_seed(0)
    loss = AdversarialLoss().to(DEV)
    opt_g, opt_d = FusedAdam(net.parameters(), lr=2e-4), FusedAdam(loss.parameters(), lr=1e-4, betas=(0.5, 0.999))
    _, losses = train_epoch_gan(net, loss, opt_g, opt_d, [[ds[0], ds[1]]], dem_preparer(DEV), dem_real_rows)
    print("DEM step losses (point + 0.1 g, g, d): %s" % losses)
    assert losses.shape == (1, 3) and np.isfinite(losses).all()
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters())) and all(torch.isfinite(p).all() for p in net.parameters())
