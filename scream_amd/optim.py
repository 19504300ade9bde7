"""FusedAdam: torch.optim.Adam for the models of this package with the whole update in one HIP launch (csrc/optim.hip).

    opt = FusedAdam(net.parameters(), lr=2e-4)                   # the reference's Adam(params=net.parameters(), lr=lr_g)
    opt_d = FusedAdam(dis.parameters(), lr=2e-4, betas=(0.5, 0.999))
    loss.backward(); opt.step()                                  # or scaler.step(opt) under a torch.amp.GradScaler

The arithmetic is the float64 contract of include/scream_hip.h ("The optimiser step"), restated in numpy by tests/adam_ref.py:
torch's update with one rounding per stored value.  What differs from torch.optim.Adam, all of it on purpose:
  * exp_avg / exp_avg_sq of a param group live in two flat arenas and ``state[p]`` holds views of them; ``state[p]["step"]`` is
    a view of the group's ONE device step count, with the running powers beta^step beside it.  A skipped GradScaler step
    therefore needs no host knowledge, and a step never reads anything back.  A parameter whose ``.grad`` is None is skipped as
    torch skips it, but the count it will be corrected with is the group's.
  * weight_decay, amsgrad, maximize, a tensor lr and sparse gradients are refused; there is no CPU path (a step on parameters
    that are not on the GPU is an error; state_dict / load_state_dict work anywhere).
  * ``.grad`` tensors are new every step (the backward allocates them), so each step uploads the work list: one copy of
    40 bytes per parameter out of a ring of pinned buffers, a slot of which is rewritten only once the copy that last read it
    has completed.  Beyond that a step allocates nothing on the device after the first one and synchronises nothing.
  * the kernel writes through raw pointers, so ``step()`` bumps the version counter of every parameter it updated
    (PointTransformer keys its cached weight images on them).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

__all__ = ["FusedAdam", "ADAM_CHUNK"]

ADAM_CHUNK = 4096      # SCREAM_ADAM_CHUNK: elements per block
_ROW = 5               # int64 words per row of the work list (SCREAM_ADAM_TENSOR_BYTES / 8): p, grad, m, v, numel
_RING = 4              # pinned staging slots per group


def running_powers(beta1: float, beta2: float, steps: int) -> Tuple[float, float]:
    """beta1^steps and beta2^steps as the kernel accumulates them: by repeated float64 multiplication from 1.0."""
    q1 = q2 = 1.0
    for _ in range(int(steps)):
        q1 *= beta1
        q2 *= beta2
    return q1, q2


def _upload(host: np.ndarray, dev) -> torch.Tensor:
    """A small host array on `dev` without a synchronising copy: through pinned memory, which torch's host allocator hands out
    again only once the copy has completed."""
    t = torch.from_numpy(host)
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.clone()


class _Group:
    """Device state of one param group: the arenas, the scalar state and the staging of its work list."""

    def __init__(self, params: List[torch.Tensor], betas, steps: int = 0):
        if not params:
            raise ValueError("FusedAdam: a param group without parameters")
        dev = params[0].device
        for p in params:
            if p.device != dev:
                raise ValueError("FusedAdam: the parameters of one group must share a device (%s and %s)" % (dev, p.device))
            if p.dtype != torch.float32 or p.is_sparse:
                raise TypeError("FusedAdam updates dense fp32 parameters, got %s" % p.dtype)
        self.params, self.device = list(params), dev
        self.numel = [p.numel() for p in params]
        offsets, at = [], 0
        for n in self.numel:  # every tensor's slice of the arenas begins 16-byte aligned
            offsets.append(at)
            at += (n + 3) // 4 * 4
        self.m = torch.zeros(max(at, 4), device=dev, dtype=torch.float32)
        self.v = torch.zeros(max(at, 4), device=dev, dtype=torch.float32)
        self.m_views = [self.m[o:o + n].view_as(p) for o, n, p in zip(offsets, self.numel, params)]
        self.v_views = [self.v[o:o + n].view_as(p) for o, n, p in zip(offsets, self.numel, params)]
        host = np.zeros(3, dtype=np.float64)  # { q1, q2, (float step, unused) }
        host[0], host[1] = running_powers(float(betas[0]), float(betas[1]), steps)
        host[2:3].view(np.float32)[0] = float(steps)
        self.scalars = _upload(host, dev)
        self.step = self.scalars[2:3].view(torch.float32)[0]
        # static columns of the work list (m, v, numel per parameter); p and grad are read at every step
        self.static = np.array([[m.data_ptr(), v.data_ptr(), n] for m, v, n in zip(self.m_views, self.v_views, self.numel)],
                               dtype=np.int64).reshape(len(params), 3)
        self.table = None     # device int64 [len(params) * _ROW]
        self.ring = []        # [pinned int64 tensor, its numpy view, event of the copy that last read it]
        self.slot = 0
        self.chunks: Dict[tuple, Tuple[torch.Tensor, int, np.ndarray]] = {}

    def powers(self) -> torch.Tensor:
        return self.scalars[:2]

    def _chunks_for(self, active: tuple):
        hit = self.chunks.get(active)
        if hit is None:
            counts = np.array([(self.numel[i] + ADAM_CHUNK - 1) // ADAM_CHUNK for i in active], dtype=np.int64)
            if int(counts.sum()) >= 2 ** 31:
                raise _lib.ScreamHipError("FusedAdam: more than 2^31 - 1 chunks in one group")
            rows = np.repeat(np.arange(len(active), dtype=np.int32), counts)
            first = np.repeat(np.cumsum(counts) - counts, counts)
            inside = (np.arange(rows.shape[0], dtype=np.int64) - first).astype(np.int32)
            host = np.stack([rows, inside], axis=1) if rows.shape[0] else np.zeros((1, 2), dtype=np.int32)
            if len(self.chunks) >= 8:  # the set of parameters that carry a gradient rarely changes
                self.chunks.clear()
            hit = (_upload(np.ascontiguousarray(host), self.device), int(rows.shape[0]), self.static[list(active)])
            self.chunks[active] = hit
        return hit

    def launch(self, lr: float, betas, eps: float, grad_scale: Optional[torch.Tensor], found_inf: Optional[torch.Tensor]) -> List[torch.Tensor]:
        params = self.params
        active = tuple(i for i, p in enumerate(params) if p.grad is not None and self.numel[i] > 0)
        if not active:
            return []
        dev = self.device
        if dev.type != "cuda":
            raise _lib.ScreamHipError("FusedAdam.step needs the parameters on the MI355X (got device %s); there is no CPU path" % dev)
        grads = []
        for i in active:
            p, g = params[i], params[i].grad
            if p.device != dev or g.device != dev:
                raise _lib.ScreamHipError("FusedAdam: a parameter or its gradient left %s after the optimiser's state was created" % dev)
            if g.is_sparse or g.dtype != torch.float32:
                raise TypeError("FusedAdam needs dense fp32 gradients, got %s%s" % ("sparse " if g.is_sparse else "", g.dtype))
            if not p.is_contiguous():
                raise ValueError("FusedAdam: parameters must be contiguous")
            grads.append(g if g.is_contiguous() else g.contiguous())
        chunks, n_chunks, static = self._chunks_for(active)
        T = len(active)
        if self.table is None:
            self.table = torch.empty(len(params) * _ROW, device=dev, dtype=torch.int64)
            for _ in range(_RING):
                pinned = torch.empty(len(params) * _ROW, dtype=torch.int64, pin_memory=True)
                self.ring.append([pinned, pinned.numpy(), None])
        slot = self.ring[self.slot]
        self.slot = (self.slot + 1) % _RING
        if slot[2] is not None and not slot[2].query():
            slot[2].synchronize()  # the host is _RING steps ahead of the device: wait for the copy that still reads this slot
        rows = slot[1][:T * _ROW].reshape(T, _ROW)
        rows[:, 0] = [params[i].data_ptr() for i in active]
        rows[:, 1] = [g.data_ptr() for g in grads]
        rows[:, 2:] = static
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            self.table[:T * _ROW].copy_(slot[0][:T * _ROW], non_blocking=True)
            if slot[2] is None:
                slot[2] = torch.cuda.Event()
            slot[2].record(stream)
            # (the table is a row of int64 per tensor behind a `const void*`: it goes as an address)
            ops.call("scream_adam_step", self.table.data_ptr(), T, chunks, n_chunks, self.scalars, _scalar_ptr(grad_scale, dev, "grad_scale"),
                     _scalar_ptr(found_inf, dev, "found_inf"), lr, betas[0], betas[1], eps, stream.cuda_stream)
        return [params[i] for i in active]


def _scalar_ptr(t: Optional[torch.Tensor], dev, what: str) -> Optional[int]:
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or t.numel() != 1:
        raise _lib.ScreamHipError("FusedAdam: %s must be one fp32 value on %s" % (what, dev))
    return t.data_ptr()


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 amsgrad: bool = False, *, maximize: bool = False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._step_supports_amp_scaling = True  # GradScaler.step hands grad_scale / found_inf over instead of reading found_inf back
        self._groups: Dict[int, _Group] = {}
        for g in self.param_groups:
            self._hyper(g)

    @staticmethod
    def _hyper(group) -> Tuple[float, Tuple[float, float], float]:
        lr, betas, eps = group["lr"], group["betas"], group["eps"]
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam takes lr by value: a tensor lr would have to be read back at every step")
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False) or \
                group.get("decoupled_weight_decay", False):
            raise ValueError("FusedAdam implements weight_decay=0, amsgrad=False, maximize=False only")
        lr, eps, betas = float(lr), float(eps), (float(betas[0]), float(betas[1]))
        if not (0.0 <= lr < float("inf")):
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not (0.0 <= eps < float("inf")):
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        return lr, betas, eps

    def _group_state(self, k: int, steps: int = 0, fresh: bool = False) -> _Group:
        group = self.param_groups[k]
        gs = self._groups.get(k)
        if gs is not None and not fresh and (len(gs.params) != len(group["params"]) or any(a is not b for a, b in zip(gs.params, group["params"]))):
            raise RuntimeError("FusedAdam: the parameters of group %d changed after its state was created" % k)
        if gs is None or fresh:
            gs = self._groups[k] = _Group(group["params"], group["betas"], steps)
            for p, m, v in zip(gs.params, gs.m_views, gs.v_views):
                self.state[p] = {"step": gs.step, "exp_avg": m, "exp_avg_sq": v}
        return gs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for k, group in enumerate(self.param_groups):
            lr, betas, eps = self._hyper(group)
            if not any(p.grad is not None for p in group["params"]):
                continue
            updated = self._group_state(k).launch(lr, betas, eps, grad_scale, found_inf)
            if updated:
                torch.autograd.graph.increment_version(updated)  # host bookkeeping only: nothing is launched
        return loss

    def state_dict(self):
        """torch.optim.Adam's layout (loadable by it and by this class); the tensors are copies, not views of the arenas."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in s.items()} for k, s in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        """From this class or from a torch.optim.Adam.  The parameters of a group must agree on `step` (torch counts per
        parameter, this class per group); the running powers are rebuilt from it by repeated multiplication."""
        super().load_state_dict(state_dict)
        self._step_supports_amp_scaling = True
        self._groups = {}
        for k, group in enumerate(self.param_groups):
            self._hyper(group)
            loaded = [(p, self.state[p]) for p in group["params"] if len(self.state.get(p, {}))]
            steps = sorted({float(s["step"]) for _, s in loaded})
            if len(steps) > 1:
                raise ValueError("FusedAdam keeps one step count per group; the loaded state has %s" % steps)
            step = steps[0] if steps else 0.0
            if step < 0 or step != int(step):
                raise ValueError("FusedAdam: invalid step count %r" % step)
            for p in group["params"]:
                self.state.pop(p, None)
            if not loaded:
                continue  # a group that never stepped: its state is created by its first step, as in torch
            gs = self._group_state(k, int(step), fresh=True)
            index = {id(p): i for i, p in enumerate(gs.params)}
            for p, s in loaded:
                gs.m_views[index[id(p)]].copy_(s["exp_avg"])
                gs.v_views[index[id(p)]].copy_(s["exp_avg_sq"])
