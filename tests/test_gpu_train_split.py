"""Training with train_backend = "split" (scream_amd/train.py, csrc/backward.hip: scream_gemm_wgrad_split_f32) against float64:
the bf16 x 3 weight-gradient kernel on its own (accuracy, scale invariance, determinism), then the gradients of whole models
under the bars of tests/test_gpu_train.py and tests/test_gpu_train_dem.py, the two backends side by side, the untouched "f32"
and inference paths, and the reference's mixed-precision loop.  Every test prints its figures before it asserts.
Needs an MI355X: run with `pytest -m gpu`."""

import numpy as np
import pytest
import torch

import train_ref as T
from oracle import scream_ref as O
from scream_amd import _lib, train
from scream_amd.synthetic import make_state_dict, make_trained_like_state_dict
from train_ref import FLOOR, make_pair, packed_rows, rel  # the yardstick shared by the training test files

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


# ------------------------------------------------------------------------------------- the kernel
# the row counts and shapes of test_gpu_train.py::test_wgrad_against_float64, plus the q|k|v shape 768 x 256
@pytest.mark.parametrize("lens", [[100], [700, 500], [20000, 17000, 3000], [160000, 169000]])
def test_wgrad_split_against_float64(lens):
    rng = np.random.default_rng(len(lens))
    shapes = [(256, 256), (1024, 256), (256, 1024)] if sum(lens) < 100000 else [(256, 256)]
    if lens == [700, 500]:
        shapes.append((768, 256))
    for N, K in shapes:
        dY = packed_rows(lens, rng, N)  # padded rows: zero gradient
        X = packed_rows(lens, rng, K, pad_value=3.0)  # padded rows: finite activations
        want = dY.double().t() @ X.double()
        cpu32 = rel(dY.t() @ X, want)
        dW = torch.empty(N, K, device=DEV)
        cs = torch.empty(N, device=DEV)
        train.wgrad_split(dY.to(DEV), X.to(DEV), dW, cs)
        e, ec = rel(dW, want), rel(cs, dY.double().sum(0))
        print("wgrad_split", lens, (N, K), "error", e, "fp32 CPU product", cpu32, "colsum", ec)
        assert e <= max(2 * cpu32, FLOOR), (N, K, e, cpu32)
        assert ec <= FLOOR
        dW2 = dW.clone()
        train.wgrad_split(dY.to(DEV), X.to(DEV), dW2, accumulate=True)
        assert rel(dW2, 2 * want) <= max(2 * cpu32, FLOOR)


def test_wgrad_split_is_scale_invariant_bit_for_bit():
    """What makes the kernel safe under a GradScaler: bf16 x 3 is exponent-blind, so dY times a power of two gives dW (and
    colsum) times that power, bit for bit.  The inputs keep every intermediate NORMAL in fp32 at every scale: |dY|, |X| in
    [2^-10, 1], so every plane is a multiple of 2^-33, every product and partial sum a multiple of 2^-66 (2^-96 at the scale
    2^-30), and no sum over 1 300 rows of products <= 1 exceeds 2^11 (2^51 at the scale 2^40)."""
    rng = np.random.default_rng(7)
    rows, N, K = 1300, 256, 384
    mag = lambda shape: (rng.choice([-1.0, 1.0], size=shape) * np.exp2(-10.0 * rng.uniform(size=shape))).astype(np.float32)
    dY, X = torch.from_numpy(mag((rows, N))).to(DEV), torch.from_numpy(mag((rows, K))).to(DEV)
    dW, cs = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
    train.wgrad_split(dY, X, dW, cs)
    assert rel(dW, dY.double().t() @ X.double()) <= FLOOR
    for e in (16, -30, 40):
        s = 2.0 ** e
        dWs, css = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        train.wgrad_split(dY * s, X, dWs, css)
        print("scale 2^%d: dW equal %s, colsum equal %s" % (e, torch.equal(dWs, dW * s), torch.equal(css, cs * s)))
        assert torch.isfinite(dWs).all()
        assert torch.equal(dWs, dW * s) and torch.equal(css, cs * s), e


def test_wgrad_split_is_deterministic():
    rng = np.random.default_rng(8)
    lens = [5000, 3000, 77]
    dY, X = packed_rows(lens, rng, 256).to(DEV), packed_rows(lens, rng, 1024, pad_value=3.0).to(DEV)
    outs = []
    for _ in range(2):
        dW, cs = torch.empty(256, 1024, device=DEV), torch.empty(256, device=DEV)
        train.wgrad_split(dY, X, dW, cs)
        outs.append((dW, cs))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------- model gradients
def build_net(sd, ns, nc, backend=None):
    from scream_amd.model import PointTransformer
    net = PointTransformer(256, ns, nc)
    net.load_state_dict(sd)
    if backend is not None:
        net.train_backend = backend
    return net.to(DEV)


def gpu_grads(net, src, tgt, rot, trans):
    return T.point_module_grads(net, src, tgt, rot, trans, DEV)


def masked_rule(what, net, sd, pair):
    """The rule of tests/train_ref.py for one pair on `net`: the gradients of a direct train.forward_saving / train.backward
    pass (bitwise those of net(...); loss.backward()) against float64 under THAT pass's relu masks and L1 signs, per tensor
    <= max(2 x the fp32 CPU oracle's error under the same masks, 5e-6).  Returns (loss, gradients)."""
    loss, g, masks = T.point_gpu(net, [pair], DEV)
    assert len(g) == len(sd)
    T.assert_bitwise("forward_saving + backward against net(...); loss.backward()", g, gpu_grads(net, *pair)[1])
    g64m, g32m = T.masked_oracles(T.oracle_grads, sd, [pair], masks)
    bad = T.rule(what, g, g64m, g32m)
    assert not bad, bad
    return loss, g


# The three configurations and the rule of test_gpu_train.py::test_model_gradients_against_float64.  The split products round
# differently from the fp32-input MFMA, so a hidden unit within rounding of zero can be switched differently (in the (1, 1)
# configuration unit 619 of packed row 250 of stem.0: pre-activation 5e-8 beside |m1| = 16; docs/design/oracle_and_parity.md,
# "Training under split arithmetic"); under the split pass's OWN masks every tensor takes the one rule.
# The case ids are the ones these cases have had since they were added: they end in the (ratio, floor) each case was held to
# before every case took the one rule of masked_rule.  Kept, so that the record of a case stays one series; they set nothing.
@pytest.mark.parametrize("ns,nc,n,m", [pytest.param(1, 1, 700, 900, id="1-1-700-900-2-5e-06"),
                                      pytest.param(2, 2, 690, 910, id="2-2-690-910-4-0.0005"),
                                      pytest.param(6, 6, 2000, 2100, id="6-6-2000-2100-4-0.0005")])
def test_model_gradients_against_float64_split(ns, nc, n, m):
    sd = make_state_dict(5 + ns, 256, ns, nc)
    pair = make_pair(ns, n, m)
    loss, _ = masked_rule("split (%d,%d)" % (ns, nc), build_net(sd, ns, nc, "split"), sd, pair)
    d = lambda t: t.double()
    src, tgt, rot, trans = pair
    with torch.no_grad():  # float64 under its own masks
        pred = O.point_transformer_forward(d(src), d(tgt), {k: d(v) for k, v in sd.items()}, d(trans).permute(0, 2, 1))
        loss64 = O.point_loss(pred, d(src), d(rot), d(trans)).item()
    print("loss", loss, "float64", loss64)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)


def test_dem_gradients_against_float64_split():
    """The (2, 2) configuration of test_gpu_train_dem.py::test_model_gradients_against_float64: separate stems, the target-side
    stem's gradient through the cross layers' key/value path (the K = 512 data gradient)."""
    from scream_amd.model import DEMTransformer
    ns, nc, points = 2, 2, 690
    sd = make_state_dict(30 + ns, 256, ns, nc, dem=True)
    sample = T.terrain(ns, points)
    net = DEMTransformer(256, ns, nc)
    net.load_state_dict(sd)
    net.train_backend = "split"
    net = net.to(DEV).train()
    loss, g, masks = T.dem_gpu(net, [sample], DEV)
    assert len(g) == len(sd)
    T.assert_bitwise("forward_saving + backward against net(...); loss.backward()", g, T.dem_module_grads(net, *sample, DEV)[1])
    g64m, g32m = T.masked_oracles(T.dem_oracle_grads, sd, [sample], masks)
    bad = T.rule("split DEM (2,2)", g, g64m, g32m)
    assert not bad, bad
    dsm, coarse, dem = (t.double() for t in sample)
    with torch.no_grad():
        loss64 = O.dem_loss(O.dem_transformer_forward(dsm, coarse, {k: v.double() for k, v in sd.items()}), dem).item()
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)


def test_trained_like_weights_split_against_the_f32_backend():
    """LayerNorm gains up to 240 (make_trained_like_state_dict): an fp16 x 2 forward would leave its range here; bf16 x 3 has
    none to leave.  The two backends switch hidden units differently, so each is held to the rule against float64 under its
    own masks."""
    ns, nc = 2, 2
    sd = make_trained_like_state_dict(3, 256, ns, nc)
    pair = make_pair(21, 690, 910)
    for backend in ("f32", "split"):
        _, g = masked_rule("%s trained-like (2,2)" % backend, build_net(sd, ns, nc, backend), sd, pair)
        assert all(torch.isfinite(v).all() for v in g.values())


def test_the_two_backends_agree_within_the_float64_rule():
    ns, nc = 2, 2
    sd = make_state_dict(17, 256, ns, nc)
    pair = make_pair(22, 640, 800)
    for backend in ("f32", "split"):
        masked_rule("%s (2,2)" % backend, build_net(sd, ns, nc, backend), sd, pair)


def test_sgd_trajectory_matches_float64_oracle_split():
    """test_gpu_train.py::test_sgd_trajectory_matches_float64_oracle under "split": 1e-4 for 5 steps, 5e-4 over 10."""
    ns, nc = 1, 1
    sd = make_state_dict(13, 256, ns, nc)
    src, tgt, rot, trans = make_pair(8, 500, 700)
    net = build_net(sd, ns, nc, "split")
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    sd64 = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    opt64 = torch.optim.SGD(list(sd64.values()), lr=0.05)
    d = lambda t: t.double()
    for step in range(10):
        net.train()
        src_, _, _ = net(src.to(DEV), tgt.to(DEV), trans.permute(0, 2, 1).to(DEV), 1.0)
        loss = net.loss(src_, src.to(DEV), rot.to(DEV), trans.to(DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()
        pred64 = O.point_transformer_forward(d(src), d(tgt), sd64, d(trans).permute(0, 2, 1))
        loss64 = O.point_loss(pred64, d(src), d(rot), d(trans))
        opt64.zero_grad()
        loss64.backward()
        opt64.step()
        tol = 1e-4 if step < 5 else 5e-4
        print("step", step, "relative loss difference", abs(loss.item() - loss64.item()) / abs(loss64.item()))
        assert abs(loss.item() - loss64.item()) <= tol * abs(loss64.item()), (step, loss.item(), loss64.item())


# ------------------------------------------------------------------------------------- nothing else moved
def test_f32_backend_and_inference_are_untouched():
    ns, nc = 2, 2
    sd = make_state_dict(19, 256, ns, nc)
    src, tgt, rot, trans = make_pair(23, 500, 650)
    _, g0 = gpu_grads(build_net(sd, ns, nc), src, tgt, rot, trans)  # the attribute never touched
    _, g1 = gpu_grads(build_net(sd, ns, nc, "f32"), src, tgt, rot, trans)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), "gradient of %s differs between the default and train_backend = 'f32'" % k

    def infer(net):
        net.eval()
        out, _, _ = net(src.to(DEV), tgt.to(DEV), trans.permute(0, 2, 1).to(DEV), 1.0)
        assert out.grad_fn is None
        return out

    want = infer(build_net(sd, ns, nc))
    net = build_net(sd, ns, nc, "split")
    before = infer(net)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    src_, _, _ = net(src.to(DEV), tgt.to(DEV), trans.permute(0, 2, 1).to(DEV), 1.0)
    net.loss(src_, src.to(DEV), rot.to(DEV), trans.to(DEV)).backward()
    opt.step()
    assert not torch.equal(infer(net), want)  # the step did move the weights
    net.load_state_dict(sd)  # ... and restoring them restores inference bit for bit
    after = infer(net)
    assert torch.equal(before, want) and torch.equal(after, want)
    net.train()
    with torch.no_grad():  # no_grad keeps the inference path whatever the backend
        out, _, _ = net(src.to(DEV), tgt.to(DEV), trans.permute(0, 2, 1).to(DEV), 1.0)
    assert out.grad_fn is None and torch.equal(out, want)


# ------------------------------------------------------------------------------------- the reference's mixed-precision loop
def test_reference_mixed_precision_loop_split():
    """train_kitti.py:150-186: `with autocast():` around forward and loss, scaler.scale(loss).backward(), scaler.step,
    scaler.update.  The loss scale (2^16) multiplies every gradient product's dY: the scale-free bf16 x 3 products carry it, the
    scaler must find no inf / NaN (it would skip the step and halve its scale), and the loss must fall."""
    net = build_net(make_state_dict(12, 256, 1, 1), 1, 1, "split")
    opt = torch.optim.Adam(net.parameters(), lr=2e-4)
    scaler = torch.cuda.amp.GradScaler()
    src, tgt, rot, trans = (t.to(DEV) for t in make_pair(7, 600, 800))
    losses, scale0 = [], None
    for step in range(5):
        net.train()
        with torch.cuda.amp.autocast():
            src_, _, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0)
            loss = net.loss(src_, src, rot, trans)
        opt.zero_grad()
        scaler.scale(loss).backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())  # still times the loss scale
        scale0 = scaler.get_scale() if scale0 is None else scale0
        scaler.step(opt)
        scaler.update()  # halves the scale if the step found inf / NaN
        losses.append(float(loss.detach()))
        print("step", step, "loss", losses[-1], "scale", scaler.get_scale())
        assert scaler.get_scale() >= scale0, "the scaler saw inf / NaN gradients and backed off"
    assert scale0 >= 2.0 ** 16
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
