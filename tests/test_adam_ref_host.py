"""The numpy restatement of the Adam contract (tests/adam_ref.py) against an all-float64 trajectory, the learning-rate rule of
scream_amd/fit.py and the state-dict interchange of FusedAdam with torch.optim.Adam.  No GPU."""
import copy
import functools
import inspect

import numpy as np
import pytest
import torch

from adam_ref import AdamRef, running_powers
from scream_amd import FusedAdam, _lib
from scream_amd.fit import lr_after_epoch
from scream_amd.optim import running_powers as layer_powers

N = 4096
LR = 1e-3


@functools.lru_cache(maxsize=None)
def trajectory_inputs(steps):
    """p0 like weights; gradients of magnitude 1e-6 .. 1 (log-uniform per element and step, random sign), fp32."""
    rng = np.random.default_rng(steps)
    p0 = (0.1 * rng.standard_normal(N)).astype(np.float32)
    grads = [(rng.choice([-1.0, 1.0], size=N) * 10.0 ** rng.uniform(-6.0, 0.0, size=N)).astype(np.float32) for _ in range(steps)]
    return p0, grads


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
@pytest.mark.parametrize("steps", [10, 200])
def test_restatement_against_the_all_float64_trajectory(steps, betas):
    """fp32 state with one rounding per stored value against state kept in float64: the restatement's worst error is held to
    max(2 x torch.optim.Adam(foreach=False)'s in fp32 on the CPU, one fp32 spacing of max|p|) -- the project's rule for fp32 paths
    held to float64."""
    p0, grads = trajectory_inputs(steps)
    exact, ref = AdamRef([p0], LR, betas, state=np.float64), AdamRef([p0], LR, betas)
    pt = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=LR, betas=betas, foreach=False)
    for g in grads:
        exact.step([g])
        ref.step([g])
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
    want = exact.p[0]
    err_ref = np.abs(ref.p[0].astype(np.float64) - want).max()
    err_torch = np.abs(pt.detach().numpy().astype(np.float64) - want).max()
    spacing = float(np.spacing(np.float32(np.abs(want).max())))
    print("steps %d betas %s: restatement %.3g, torch fp32 %.3g, one spacing %.3g" % (steps, betas, err_ref, err_torch, spacing))
    assert ref.p[0].dtype == np.float32 and ref.m[0].dtype == np.float32 and exact.p[0].dtype == np.float64
    assert np.abs(want - p0).max() > 100 * spacing  # the parameters moved
    assert err_ref <= max(2 * err_torch, spacing)
    assert ref.steps == steps and (ref.q1, ref.q2) == running_powers(betas[0], betas[1], steps)


def test_restatement_skipped_step_and_grad_scale():
    p0, grads = trajectory_inputs(10)
    a, b = AdamRef([p0], LR), AdamRef([p0], LR)
    for k, g in enumerate(grads):
        a.step([g])
        if k == 4:  # a skipped step changes nothing: not the values, not the count, not the powers
            before = (b.p[0].copy(), b.m[0].copy(), b.v[0].copy(), b.q1, b.q2, b.steps)
            b.step([np.full(N, np.inf, dtype=np.float32)], grad_scale=65536.0, found_inf=1.0)
            assert all(np.array_equal(x, y) for x, y in zip(before[:3], (b.p[0], b.m[0], b.v[0]))) and before[3:] == (b.q1, b.q2, b.steps)
        b.step([g * np.float32(65536.0)], grad_scale=65536.0, found_inf=0.0)  # a power of two scales exactly
    for x, y in zip(a.p + a.m + a.v, b.p + b.m + b.v):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    c = AdamRef([p0, p0], LR)
    c.step([grads[0], None])  # a parameter without a gradient is skipped
    assert np.array_equal(c.p[1], p0) and not c.m[1].any() and not np.array_equal(c.p[0], p0)


def test_lr_after_epoch_is_the_reference_rule():
    lr, seen = 2e-4, {}
    for epoch in range(1, 45):
        lr = lr_after_epoch(lr, epoch)
        seen[epoch] = lr
    assert seen[14] == 2e-4 and seen[15] == 1e-4 and seen[29] == 1e-4 and seen[30] == 5e-5 and seen[44] == 5e-5
    lr = 2e-4
    for epoch in range(1, 45):  # every epoch: halved down to the floor and never below it
        lr = lr_after_epoch(lr, epoch, every=1)
        assert lr >= 1e-5
    assert lr == 1e-5
    assert lr_after_epoch(3.2e-4, 10, every=10) == 1.6e-4 and lr_after_epoch(3.2e-4, 9, every=10) == 3.2e-4


def _params(seed, shapes=((7,), (3, 5), (256,))):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).requires_grad_(True) for s in shapes]


def _torch_steps(opt, params, steps, seed0):
    for k in range(steps):
        g = torch.Generator().manual_seed(seed0 + k)
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
def test_state_dict_interchange_with_torch_adam(betas):
    params = _params(1)
    adam = torch.optim.Adam(params, lr=2e-4, betas=betas)
    _torch_steps(adam, params, 3, 10)
    # torch -> FusedAdam: the arenas hold torch's moments, one step count, the powers rebuilt by repeated multiplication
    mine = [p.detach().clone().requires_grad_(True) for p in params]
    fused = FusedAdam(mine, lr=1.0, betas=(0.1, 0.2))
    fused.load_state_dict(adam.state_dict())
    assert fused.param_groups[0]["lr"] == 2e-4 and tuple(fused.param_groups[0]["betas"]) == betas
    gs = fused._groups[0]
    for p, q in zip(mine, params):
        assert torch.equal(fused.state[p]["exp_avg"], adam.state[q]["exp_avg"]) and fused.state[p]["exp_avg"].shape == p.shape
        assert torch.equal(fused.state[p]["exp_avg_sq"], adam.state[q]["exp_avg_sq"])
        assert fused.state[p]["exp_avg"].data_ptr() % 16 == 0 and fused.state[p]["exp_avg"].untyped_storage().data_ptr() == gs.m.untyped_storage().data_ptr()
        assert fused.state[p]["step"].dtype == torch.float32 and float(fused.state[p]["step"]) == 3.0
        assert fused.state[p]["step"].untyped_storage().data_ptr() == gs.scalars.untyped_storage().data_ptr()
    assert tuple(gs.powers().tolist()) == running_powers(betas[0], betas[1], 3) == layer_powers(betas[0], betas[1], 3)
    # FusedAdam -> torch: a torch Adam loaded with it continues exactly like the one that never stopped
    sd = fused.state_dict()
    assert sd["state"][0]["exp_avg"].data_ptr() != fused.state[mine[0]]["exp_avg"].data_ptr()  # copies, not views of the arenas
    theirs = [p.detach().clone().requires_grad_(True) for p in params]
    resumed = torch.optim.Adam(theirs, lr=1.0)
    resumed.load_state_dict(copy.deepcopy(sd))
    _torch_steps(adam, params, 2, 20)
    _torch_steps(resumed, theirs, 2, 20)
    for p, q in zip(params, theirs):
        assert torch.equal(p, q)
    # and FusedAdam -> FusedAdam
    again = FusedAdam([p.detach().clone().requires_grad_(True) for p in mine], lr=1.0)
    again.load_state_dict(sd)
    for p, q in zip(again.param_groups[0]["params"], mine):
        assert torch.equal(again.state[p]["exp_avg_sq"], fused.state[q]["exp_avg_sq"]) and float(again.state[p]["step"]) == 3.0


def test_fused_adam_refuses_what_it_does_not_implement():
    p = _params(2)
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(lr=torch.tensor(1e-3)), dict(betas=(1.0, 0.9)),
               dict(lr=-1.0), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            FusedAdam(p, **kw)
    opt = FusedAdam(p, lr=2e-4)
    assert opt._step_supports_amp_scaling and opt.state_dict()["state"] == {}
    assert "grad_scaler" not in inspect.signature(opt.step).parameters  # GradScaler hands its scale over through attributes
    opt.step()  # no gradient anywhere: nothing to do, as in torch
    assert len(opt.state) == 0
    for q in p:
        q.grad = torch.ones_like(q)
    with pytest.raises(_lib.ScreamHipError):
        opt.step()  # there is no CPU path
    # torch counts steps per parameter, FusedAdam per group: a state whose parameters disagree is refused
    adam = torch.optim.Adam(p, lr=2e-4)
    _torch_steps(adam, p, 1, 0)
    p[0].grad = None
    adam.step()
    with pytest.raises(ValueError):
        FusedAdam([q.detach().clone().requires_grad_(True) for q in p]).load_state_dict(adam.state_dict())
    wd = torch.optim.Adam(_params(3), lr=2e-4, weight_decay=0.1)
    with pytest.raises(ValueError):
        FusedAdam(_params(3)).load_state_dict(wd.state_dict())
