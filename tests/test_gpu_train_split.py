"""Training with train_backend = "split" (scream_amd/train.py, csrc/backward.hip: scream_gemm_wgrad_split_f32) against float64:
the bf16 x 3 weight-gradient kernel on its own (accuracy, scale invariance, determinism), then the gradients of whole models
under the bars of tests/test_gpu_train.py and tests/test_gpu_train_dem.py, the two backends side by side, the untouched "f32"
and inference paths, and the reference's mixed-precision loop.  Every test prints its figures before it asserts.
Needs an MI355X: run with `pytest -m gpu`."""

import numpy as np
import pytest
import torch

from oracle import scream_ref as O
from scream_amd import _lib, train
from scream_amd.evaluate_open_gf import SyntheticDEM
from scream_amd.synthetic import make_state_dict, make_trained_like_state_dict, random_rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 5e-6  # the fixed floor of the "<= 2 x the fp32 path's error" rule


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.norm(a - b) / max(torch.linalg.norm(b).item(), 1e-300)).item()


def packed_rows(lens, rng, width, pad_value=0.0):
    """[sum(padded lens), width] with real rows random and padded tails `pad_value`."""
    parts = []
    for n in lens:
        p = (n + 127) // 128 * 128
        x = np.full((p, width), pad_value, dtype=np.float32)
        x[:n] = rng.standard_normal((n, width)).astype(np.float32)
        parts.append(x)
    return torch.from_numpy(np.concatenate(parts))


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
def make_pair(seed, n, m):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-0.6, 0.6, size=(m, 3)).astype(np.float32)
    R = random_rotation(rng, 30.0).astype(np.float32)
    t = rng.uniform(-0.1, 0.1, size=(3, 1)).astype(np.float32)
    base = tgt[rng.permutation(m)[:n]] if n <= m else np.concatenate([tgt, rng.uniform(-0.6, 0.6, size=(n - m, 3))])
    src = ((base - t.T) @ R + 0.005 * rng.standard_normal((n, 3))).astype(np.float32)  # R src + t ~ tgt
    return (torch.from_numpy(src)[None], torch.from_numpy(tgt)[None], torch.from_numpy(R)[None], torch.from_numpy(t)[None])


def oracle_grads(sd, src, tgt, rot, trans, dtype):
    sdx = {k: v.to(dtype).requires_grad_() for k, v in sd.items()}
    c = lambda t: t.to(dtype)
    pred = O.point_transformer_forward(c(src), c(tgt), sdx, c(trans).permute(0, 2, 1))
    loss = O.point_loss(pred, c(src), c(rot), c(trans))
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sdx.items()}


def build_net(sd, ns, nc, backend=None):
    from scream_amd.model import PointTransformer
    net = PointTransformer(256, ns, nc)
    net.load_state_dict(sd)
    if backend is not None:
        net.train_backend = backend
    return net.to(DEV)


def gpu_grads(net, src, tgt, rot, trans):
    net.train()
    net.zero_grad(set_to_none=True)
    src_, _, _ = net(src.to(DEV), tgt.to(DEV), trans.permute(0, 2, 1).to(DEV), 1.0)
    assert src_.grad_fn is not None
    loss = net.loss(src_, src.to(DEV), rot.to(DEV), trans.to(DEV))
    loss.backward()
    return loss.item(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


def check_rule(what, g, g64, gref, ratio, floor, floors=None):
    """Per tensor: error against float64 <= max(ratio x the yardstick's error against float64, floor).  floors: tensors with a
    floor of their own.  Prints the worst tensor."""
    bad, worst = [], (0.0, None, 0.0, 0.0)
    for k in g64:
        e, er = rel(g[k], g64[k]), rel(gref[k], g64[k])
        bar = max(ratio * er, (floors or {}).get(k, floor))
        if e / bar > worst[0]:
            worst = (e / bar, k, e, er)
        if not e <= bar:
            bad.append((k, e, er))
    print("%s: worst tensor %s at %.3g of its bar (error %.3g, yardstick %.3g); largest error %.3g; %d over the bar"
          % (what, worst[1], worst[0], worst[2], worst[3], max(rel(g[k], g64[k]) for k in g64), len(bad)))
    return bad


# A finding (docs/design/oracle_and_parity.md, "Training under split arithmetic"): in the (1, 1) configuration ONE unit of
# stem.0's FFN hidden layer (packed row 250, unit 619) has the pre-activation 5e-8 beside |m1| = 16, i.e. 3e-9 relative --
# inside every fp32 product's rounding.  float64 and the fp32-input MFMA give it a positive sign (hid = 2.1e-7), bf16 x 3 gives
# 0, so its relu mask differs and with it every gradient that flows through stem.0's hidden layer: the eleven tensors below land
# at 9.2e-5 .. 5.53e-4 relative (measured; every other tensor of that model, and every tensor of four other seeds, stays within
# 3.2e-6, the same as "f32").  It is the effect that gives the deeper models 4 x / 5e-4 in test_gpu_train.py, met here in the
# shallow one.  Those eleven tensors take the issue's rule for a tensor that needs a looser bar: the measured worst case over
# five seeds (5.53e-4) with a factor 2 on top.  That is above 5e-4 because one unit among the 1.8 M of that layer carries
# 5.5e-4 of the gradient norm of v_proj here; every other tensor keeps max(2 x, 5e-6).
BEHIND_STEM0_RELU = ["embedding.weight", "embedding.bias", "pre_norm.weight", "pre_norm.bias", "stem.0.q_proj.weight",
                     "stem.0.k_proj.weight", "stem.0.v_proj.weight", "stem.0.merge.weight", "stem.0.norm1.weight",
                     "stem.0.norm1.bias", "stem.0.mlp.0.weight"]
RELU_FLIP_FLOOR = 2 * 5.53e-4


# the three configurations, rule and (ratio, floor) of test_gpu_train.py::test_model_gradients_against_float64
@pytest.mark.parametrize("ns,nc,n,m,ratio,floor", [(1, 1, 700, 900, 2, FLOOR), (2, 2, 690, 910, 4, 5e-4), (6, 6, 2000, 2100, 4, 5e-4)])
def test_model_gradients_against_float64_split(ns, nc, n, m, ratio, floor):
    sd = make_state_dict(5 + ns, 256, ns, nc)
    src, tgt, rot, trans = make_pair(ns, n, m)
    loss64, g64 = oracle_grads(sd, src, tgt, rot, trans, torch.float64)
    _, g32 = oracle_grads(sd, src, tgt, rot, trans, torch.float32)
    net = build_net(sd, ns, nc, "split")
    loss, g = gpu_grads(net, src, tgt, rot, trans)
    assert len(g) == len(sd)
    floors = {k: RELU_FLIP_FLOOR for k in BEHIND_STEM0_RELU} if (ns, nc) == (1, 1) else None
    assert floors is None or all(k in sd for k in floors)
    bad = check_rule("split (%d,%d)" % (ns, nc), g, g64, g32, ratio, floor, floors)
    assert not bad, bad
    print("loss", loss, "float64", loss64)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)


def test_dem_gradients_against_float64_split():
    """The (2, 2) configuration of test_gpu_train_dem.py::test_model_gradients_against_float64: separate stems, the target-side
    stem's gradient through the cross layers' key/value path (the K = 512 data gradient)."""
    from scream_amd.model import DEMTransformer
    ns, nc, points, ratio, floor = 2, 2, 690, 4, 5e-4
    sd = make_state_dict(30 + ns, 256, ns, nc, dem=True)
    dsm, coarse, dem, _ = SyntheticDEM(1, ns, points)[0]
    dsm, coarse, dem = dsm[None], coarse[None], dem[None]
    l1 = lambda pred, ref: torch.mean(torch.sum(torch.abs(pred - ref), dim=-1), dim=1).mean(dim=0)  # models/pointnet.py:162-166

    def oracle(dtype):
        sdx = {k: v.to(dtype).requires_grad_() for k, v in sd.items()}
        loss = l1(O.dem_transformer_forward(dsm.to(dtype), coarse.to(dtype), sdx), dem.to(dtype))
        loss.backward()
        return loss.item(), {k: v.grad for k, v in sdx.items()}

    loss64, g64 = oracle(torch.float64)
    _, g32 = oracle(torch.float32)
    net = DEMTransformer(256, ns, nc)
    net.load_state_dict(sd)
    net.train_backend = "split"
    net = net.to(DEV).train()
    dem_, imgs = net(dsm.to(DEV), coarse.to(DEV), False)
    assert dem_.grad_fn is not None and imgs is None
    loss = net.loss(dem_, dem.to(DEV))
    loss.backward()
    g = {n: p.grad.detach().cpu() for n, p in net.named_parameters()}
    assert len(g) == len(sd)
    bad = check_rule("split DEM (2,2)", g, g64, g32, ratio, floor)
    assert not bad, bad
    assert abs(loss.item() - loss64) <= 1e-5 * abs(loss64)


def test_trained_like_weights_split_against_the_f32_backend():
    """LayerNorm gains up to 240 (make_trained_like_state_dict): an fp16 x 2 forward would leave its range here; bf16 x 3 has
    none to leave.  No training test used these weights before, so the yardstick is the "f32" backend on the same model and
    input: per tensor, the "split" error against float64 <= max(4 x the "f32" backend's error against float64, 5e-4)."""
    ns, nc = 2, 2
    sd = make_trained_like_state_dict(3, 256, ns, nc)
    src, tgt, rot, trans = make_pair(21, 690, 910)
    _, g64 = oracle_grads(sd, src, tgt, rot, trans, torch.float64)
    _, gf = gpu_grads(build_net(sd, ns, nc, "f32"), src, tgt, rot, trans)
    _, gs = gpu_grads(build_net(sd, ns, nc, "split"), src, tgt, rot, trans)
    assert all(torch.isfinite(v).all() for v in gs.values())
    ratios = {k: rel(gs[k], g64[k]) / max(rel(gf[k], g64[k]), 1e-300) for k in sd}
    k = max(ratios, key=ratios.get)
    print("trained-like: largest split / f32 error ratio %.3g (%s: split %.3g, f32 %.3g); median ratio %.3g"
          % (ratios[k], k, rel(gs[k], g64[k]), rel(gf[k], g64[k]), float(np.median(list(ratios.values())))))
    bad = check_rule("split trained-like (2,2) vs f32 backend", gs, g64, gf, 4, 5e-4)
    assert not bad, bad


def test_the_two_backends_agree_within_the_float64_rule():
    ns, nc = 2, 2
    sd = make_state_dict(17, 256, ns, nc)
    src, tgt, rot, trans = make_pair(22, 640, 800)
    _, g64 = oracle_grads(sd, src, tgt, rot, trans, torch.float64)
    _, g32 = oracle_grads(sd, src, tgt, rot, trans, torch.float32)
    for backend in ("f32", "split"):
        _, g = gpu_grads(build_net(sd, ns, nc, backend), src, tgt, rot, trans)
        bad = check_rule("%s (2,2)" % backend, g, g64, g32, 4, 5e-4)
        assert not bad, (backend, bad)


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
