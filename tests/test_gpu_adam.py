"""FusedAdam (scream_amd/optim.py, csrc/optim.hip) on the MI355X against the numpy restatement of its contract
(tests/adam_ref.py): m and v use only +, - and * and must match bit for bit; p goes through a float64 square root and two
divisions and must be equal or an adjacent fp32 value (expected: equal everywhere; the count of unequal elements is printed).
Run with `pytest -m gpu`."""
import functools

import numpy as np
import pytest
import torch

from adam_ref import AdamRef, running_powers
from scream_amd import FusedAdam, _lib
from scream_amd.optim import ADAM_CHUNK
from scream_amd.synthetic import make_state_dict
from train_ref import make_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-3
# tail lengths 1, 3, 0, 1 around the 16-byte vector; a block's lane count and one past it; one chunk and its neighbours; several
# chunks with a tail; a matrix; an empty tensor.  The last entry never receives a gradient.
SHAPES = [(1,), (3,), (4,), (5,), (255,), (256,), (257,), (4096,), (ADAM_CHUNK - 1,), (ADAM_CHUNK,), (ADAM_CHUNK + 1,), (65541,),
          (256, 1024), (0,), (100,)]
NO_GRAD = len(SHAPES) - 1


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(seed, steps, shapes=tuple(SHAPES)):
    """(p0 per tensor, [grads per tensor] per step): weights-like parameters, gradients of magnitude 1e-6 .. 1."""
    rng = np.random.default_rng(seed)
    p0 = [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    grads = [[(rng.choice([-1.0, 1.0], size=s) * 10.0 ** rng.uniform(-6.0, 0.0, size=s)).astype(np.float32) for s in shapes]
             for _ in range(steps)]
    return p0, grads


SENTINEL = 12345.0


def device_params(p0, misalign=(), bufs=None):
    """Leaf fp32 tensors on the GPU; those listed in `misalign` begin 4 bytes past a 16-byte boundary and are followed by a
    sentinel element (their buffers are appended to `bufs`)."""
    out = []
    for i, a in enumerate(p0):
        if i in misalign:
            buf = torch.full((a.size + 2,), SENTINEL, device=DEV)
            t = buf[1:-1].view(a.shape)
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == 4
            if bufs is not None:
                bufs.append(buf)
        else:
            t = torch.from_numpy(a).to(DEV)
        out.append(t.requires_grad_(True))
    return out


def set_grads(params, grads, skip=(NO_GRAD,), scale=1.0, misalign=()):
    for i, (p, g) in enumerate(zip(params, grads)):
        if i in skip:
            p.grad = None
        elif i in misalign:
            buf = torch.zeros(g.size + 1, device=DEV)
            buf[1:] = torch.from_numpy(g.reshape(-1)).to(DEV) * scale
            p.grad = buf[1:].view(g.shape)
        else:
            p.grad = torch.from_numpy(g).to(DEV) * scale


def compare(opt, params, ref, what, skip=(NO_GRAD,)):
    """m and v bit for bit, p equal or adjacent, the step count and the powers; returns the number of unequal p elements."""
    unequal = 0
    for i, p in enumerate(params):
        got, want = host(p), ref.p[i]
        near = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
        assert near.all(), "%s: tensor %d %s: %d elements of p are not fp32 neighbours of the restatement" % (what, i, got.shape, (~near).sum())
        unequal += int((got != want).sum())
        st = opt.state[p]
        assert np.array_equal(bits(host(st["exp_avg"])), bits(ref.m[i])), "%s: tensor %d: m differs" % (what, i)
        assert np.array_equal(bits(host(st["exp_avg_sq"])), bits(ref.v[i])), "%s: tensor %d: v differs" % (what, i)
        assert float(st["step"]) == ref.steps
    gs = opt._groups[0]
    assert tuple(gs.powers().tolist()) == (ref.q1, ref.q2), what
    return unequal


def run(seed, steps, misalign=(), lrs=None, betas=(0.9, 0.999)):
    p0, grads = inputs(seed, steps)
    params = device_params(p0, misalign)
    opt = FusedAdam(params, lr=LR, betas=betas)
    ref = AdamRef(p0, LR, betas)
    for k, g in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        set_grads(params, g, misalign=misalign)
        opt.step()
        ref.step([None if i == NO_GRAD else a for i, a in enumerate(g)], lr=None if lrs is None else lrs[k])
    return opt, params, ref


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
def test_mixed_length_list_against_the_restatement(betas):
    opt, params, ref = run(1, 5, betas=betas)
    versions = [p._version for p in params]
    unequal = compare(opt, params, ref, "mixed list")
    print("mixed-length list, betas %s, five steps: %d of %d elements of p differ from the restatement (all within one fp32 neighbour)"
          % (betas, unequal, sum(p.numel() for p in params)))
    assert np.array_equal(host(params[NO_GRAD]), inputs(1, 5)[0][NO_GRAD]) and not host(opt.state[params[NO_GRAD]]["exp_avg"]).any()
    assert all(v >= 5 for i, v in enumerate(versions) if i not in (NO_GRAD, 13)) and versions[NO_GRAD] == 0  # 13: the empty tensor
    for p in params:
        assert opt.state[p]["exp_avg"].data_ptr() % 16 == 0 or p.numel() == 0


def test_tensors_that_are_not_16_byte_aligned_are_handled_element_by_element():
    """A parameter and a gradient that begin 4 bytes past a 16-byte boundary (and one of each alone): the same values, and the
    element just past each tensor's end is untouched."""
    mis = (2, 5, 8, 11)
    p0, grads = inputs(1, 5)
    bufs = []
    params = device_params(p0, mis, bufs)
    opt = FusedAdam(params, lr=LR)
    ref = AdamRef(p0, LR)
    for k, g in enumerate(grads):
        set_grads(params, g, misalign=mis[1:] if k % 2 else mis[:-1])
        opt.step()
        ref.step([None if i == NO_GRAD else a for i, a in enumerate(g)])
    compare(opt, params, ref, "misaligned")
    assert len(bufs) == len(mis) and all(float(b[0]) == SENTINEL and float(b[-1]) == SENTINEL for b in bufs)


def test_pointer_table_of_300_tensors():
    shapes = tuple((1 + (7 * i) % 23,) for i in range(300))
    p0, grads = inputs(3, 2, shapes)
    params = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in p0]
    opt = FusedAdam(params, lr=LR)
    ref = AdamRef(p0, LR)
    for g in grads:
        set_grads(params, g, skip=())
        opt.step()
        ref.step(g)
    compare(opt, params, ref, "300 tensors", skip=())


def test_two_identical_runs_are_bitwise_equal():
    a = run(2, 3)
    b = run(2, 3)
    for p, q in zip(a[1], b[1]):
        assert np.array_equal(bits(host(p)), bits(host(q)))
        assert np.array_equal(bits(host(a[0].state[p]["exp_avg_sq"])), bits(host(b[0].state[q]["exp_avg_sq"])))
    assert torch.equal(a[0]._groups[0].scalars, b[0]._groups[0].scalars)


def test_learning_rate_is_read_from_param_groups_at_every_step():
    lrs = [1e-3, 5e-4, 5e-4, 2.5e-4]
    opt, params, ref = run(4, 4, lrs=lrs)
    compare(opt, params, ref, "lr schedule")
    fixed = run(4, 4)
    assert not np.array_equal(host(fixed[1][7]), host(params[7]))


# ---------------------------------------------------------------------------------------------- GradScaler
def scaler_step(scaler, opt, sync_error=False):
    scaler.scale(torch.zeros((), device=DEV))  # what a loop's scaler.scale(loss) does for the scaler: its scale tensor exists
    mode = torch.cuda.get_sync_debug_mode()
    if sync_error:
        torch.cuda.set_sync_debug_mode("error")
    try:
        scaler.step(opt)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    scaler.update()


def sync_debug_mode_is_live():
    mode = torch.cuda.get_sync_debug_mode()
    x = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def test_grad_scaler_with_finite_gradients_equals_the_unscaled_run():
    p0, grads = inputs(5, 3)
    plain = run(5, 3)
    params = device_params(p0)
    opt = FusedAdam(params, lr=LR)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    for g in grads:
        set_grads(params, g, scale=2.0 ** 16)
        scaler_step(scaler, opt)
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    assert float(scaler.get_scale()) == 2.0 ** 16
    for p, q in zip(params, plain[1]):
        assert np.array_equal(bits(host(p)), bits(host(q)))
        assert np.array_equal(bits(host(opt.state[p]["exp_avg"])), bits(host(plain[0].state[q]["exp_avg"])))
        assert np.array_equal(bits(host(opt.state[p]["exp_avg_sq"])), bits(host(plain[0].state[q]["exp_avg_sq"])))
    # unscale_ first: the gradients are unscaled in place, grad_scale is None, the same result again
    params2 = device_params(p0)
    opt2 = FusedAdam(params2, lr=LR)
    scaler2 = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    for g in grads:
        set_grads(params2, g, scale=2.0 ** 16)
        scaler2.scale(torch.zeros((), device=DEV))
        scaler2.unscale_(opt2)
        scaler2.step(opt2)
        scaler2.update()
    for p, q in zip(params2, plain[1]):
        assert np.array_equal(bits(host(p)), bits(host(q)))


def snapshot(opt, params):
    gs = opt._groups[0]
    return [host(p).copy() for p in params] + [host(gs.m).copy(), host(gs.v).copy(), host(gs.scalars).copy()]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_grad_scaler_skips_a_non_finite_step_without_a_host_sync(bad, where):
    """A non-finite gradient in the 1-element tensor / in the last element of the last tensor with a gradient: scaler.step changes
    nothing (p, m, v, the step count, the powers), under torch's sync debug mode "error"; update() halves the scale; the next
    finite step is the restatement's step 1.  Then the same once more with non-zero moments."""
    live = sync_debug_mode_is_live()
    print("torch.cuda.set_sync_debug_mode('error') %s on this build" % ("raises on a synchronising call: the check is live" if live
                                                                       else "is INERT: the no-sync check proves nothing"))
    p0, grads = inputs(6, 2)
    params = device_params(p0)
    opt = FusedAdam(params, lr=LR)
    ref = AdamRef(p0, LR)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    target = 0 if where == "first" else NO_GRAD - 2  # the [256, 1024] matrix: the last tensor that is updated
    scale = 2.0 ** 16
    for k in range(2):
        poisoned = [a.copy() for a in grads[k]]
        poisoned[target].reshape(-1)[-1] = bad
        set_grads(params, poisoned, scale=scale)
        if k == 0:
            opt._group_state(0)  # the state exists (zeros, step 0, powers 1) so that it can be compared
        before = snapshot(opt, params)
        scaler_step(scaler, opt, sync_error=True)
        after = snapshot(opt, params)
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64), y.view(np.uint32 if y.dtype == np.float32 else np.uint64))
        assert float(opt.state[params[0]]["step"]) == k and tuple(opt._groups[0].powers().tolist()) == running_powers(0.9, 0.999, k)
        scale /= 2
        assert float(scaler.get_scale()) == scale
        set_grads(params, grads[k], scale=scale)
        scaler_step(scaler, opt, sync_error=True)
        ref.step([None if i == NO_GRAD else a for i, a in enumerate(grads[k])])
        assert float(scaler.get_scale()) == scale
        compare(opt, params, ref, "finite step %d after a skipped one" % (k + 1))


# ---------------------------------------------------------------------------------------------- state dict
def test_load_state_dict_from_torch_adam_continues_like_the_restatement():
    p0, grads = inputs(7, 5)
    theirs = device_params(p0)
    adam = torch.optim.Adam(theirs, lr=LR)
    for g in grads[:3]:
        set_grads(theirs, g)
        adam.step()
    params = [p.detach().clone().requires_grad_(True) for p in theirs]
    opt = FusedAdam(params, lr=LR)
    opt.load_state_dict(adam.state_dict())
    ref = AdamRef([host(p) for p in theirs], LR)
    zeros = lambda i: np.zeros(SHAPES[i], dtype=np.float32)
    ref.load([host(adam.state[p]["exp_avg"]) if p in adam.state else zeros(i) for i, p in enumerate(theirs)],
             [host(adam.state[p]["exp_avg_sq"]) if p in adam.state else zeros(i) for i, p in enumerate(theirs)], 3)
    compare(opt, params, ref, "loaded")
    for g in grads[3:]:
        set_grads(params, g)
        opt.step()
        ref.step([None if i == NO_GRAD else a for i, a in enumerate(g)])
    compare(opt, params, ref, "continued after load_state_dict")
    back = torch.optim.Adam([p.detach().clone().requires_grad_(True) for p in params], lr=LR)
    back.load_state_dict(opt.state_dict())  # and torch loads what FusedAdam saves
    assert float(back.state[back.param_groups[0]["params"][0]]["step"]) == 5.0


# ---------------------------------------------------------------------------------------------- the model
def build_net(seed):
    from scream_amd.model import PointTransformer
    net = PointTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(seed, 256, 1, 1))
    return net.to(DEV)


def loop_step(net, opt, src, tgt, rot, trans):
    """train_3d_match.py:156-193 up to the optimiser step."""
    net.train()
    src_, _, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0)
    loss = net.loss(src_, src, rot, trans)
    opt.zero_grad()
    loss.backward()
    return loss


def test_version_counters_move_so_that_eval_sees_the_trained_weights():
    """The end of test_reference_training_loop_runs_and_learns under FusedAdam: PointTransformer keys its cached weight images on
    p._version, which a kernel writing through raw pointers does not move by itself."""
    from scream_amd.model import PointTransformer
    net = build_net(12)
    opt = FusedAdam(net.parameters(), lr=2e-4)
    src, tgt, rot, trans = (t.to(DEV) for t in make_pair(7, 600, 800))
    net.eval()
    stale, _, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0)  # the inference images exist before training
    for _ in range(3):
        loop_step(net, opt, src, tgt, rot, trans)
        opt.step()
    net.eval()
    fresh = PointTransformer(256, 1, 1)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    fresh = fresh.to(DEV).eval()
    a, _, _ = net(src, tgt, trans.permute(0, 2, 1), 1.0)
    b, _, _ = fresh(src, tgt, trans.permute(0, 2, 1), 1.0)
    assert a.grad_fn is None and torch.equal(a, b) and not torch.equal(a, stale)


def test_twenty_steps_of_the_reference_loop_against_torch_adam():
    """FusedAdam drives the loop; a torch.optim.Adam on copies of the parameters and the all-float64 restatement are fed the same
    gradients.  Per parameter: |FusedAdam - float64| <= max(2 x |torch - float64|, one fp32 spacing of max|p|)."""
    net = build_net(12)
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())
    opt = FusedAdam(params, lr=2e-4)
    shadow = [p.detach().clone().requires_grad_(True) for p in params]
    adam = torch.optim.Adam(shadow, lr=2e-4)
    exact = AdamRef([host(p) for p in params], 2e-4, state=np.float64)
    src, tgt, rot, trans = (t.to(DEV) for t in make_pair(7, 600, 800))
    losses = []
    for _ in range(20):
        losses.append(loop_step(net, opt, src, tgt, rot, trans).detach())
        grads = [p.grad for p in params]
        assert all(g is not None for g in grads)
        for q, g in zip(shadow, grads):
            q.grad = g.clone()
        exact.step([host(g) for g in grads])
        opt.step()
        adam.step()
    losses = [float(l) for l in losses]
    assert losses[-1] < losses[0], losses
    bad, worst = [], 0.0
    for n, p, q, want in zip(names, params, shadow, exact.p):
        e_fused = np.abs(host(p).astype(np.float64) - want).max()
        e_torch = np.abs(host(q).astype(np.float64) - want).max()
        bound = max(2 * e_torch, float(np.spacing(np.float32(np.abs(want).max()))))
        worst = max(worst, e_fused / bound)
        if not e_fused <= bound:
            bad.append((n, e_fused, e_torch, bound))
    print("20 steps: worst |FusedAdam - float64| / bound over %d parameters: %.3f; loss %.5f -> %.5f" % (len(names), worst, losses[0], losses[-1]))
    assert not bad, bad
