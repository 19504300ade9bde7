"""Point-to-point ICP of raw scans in float64 on the MI355X (csrc/icp_raw.hip): the pose refinement that the reference's
``KITTI_PREDATOR`` runs with ``open3d.registration_icp`` on the UNVOXELISED scans (datasets/kitti.py:105-126: two clouds of about
120 k points spanning +-80 m, point to point, radius 0.2 m, ``max_iteration=50000``).

    T, fit_rmse, iters = icp_raw_batch(srcs, tgts, T_inits)            # lists of [N_i,3] fp32 clouds, [n,4,4] float64 poses
    idx, d2 = raw_nn_batch(srcs, tgts, Ts, 0.2)                        # the loop's search alone, per pair

include/scream_hip.h states the contract: every step one IEEE float64 operation in a fixed order, the nearest target row with
ties to the lowest row, a correspondence iff d2 < r2 strictly, fixed-order sums, exact means, R = V diag(1, 1, det) U^T,
T <- dT . T.  The sparse grid only filters candidates; the search equals the brute force bit for bit, and a pair's result depends
neither on its batch nor on ``piece``.  tests/rawicp_ref.py restates it in numpy.  Parity with open3d itself is unpinned (it is not
installed here).  ``ops.icp_p2p`` stays the tool for the normalised 5-16 k point clouds of the evaluators: it selects in fp32 and
bins into a dense capped grid, neither of which holds at 80 m.  There is no CPU path.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ._lib import ScreamHipError
from .clouds import PackedPairs, check_clouds, pose_stack
from .ops import PiecewiseRun, _p, call, icp_raw_workspace

__all__ = ["icp_raw_batch", "raw_nn_batch", "RawIcpRun"]


def _device():
    if not torch.cuda.is_available():
        raise ScreamHipError("the raw-scan ICP needs the MI355X; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


class _RawClouds(PackedPairs):
    """A call's clouds (torch tensors on the GPU, or float32 numpy arrays, which are uploaded) checked and packed, with the
    workspace both entry points need."""

    def __init__(self, srcs: Sequence, tgts: Sequence):
        srcs, tgts = list(srcs), list(tgts)
        if len(srcs) != len(tgts):
            raise ValueError("%d source clouds for %d target clouds" % (len(srcs), len(tgts)))
        first = next((c for c in srcs + tgts if isinstance(c, torch.Tensor) and c.is_cuda), None)
        dev = first.device if first is not None else _device()
        srcs = [_upload(c, i, "source cloud", dev) for i, c in enumerate(srcs)]
        tgts = [_upload(c, i, "target cloud", dev) for i, c in enumerate(tgts)]
        check_clouds(srcs, "source cloud", op="the raw-scan ICP", builtin_errors=True)
        check_clouds(tgts, "target cloud", op="the raw-scan ICP", builtin_errors=True)
        super().__init__(srcs, tgts, dev, pad=True)  # an all-empty side still needs an address
        self.ws = icp_raw_workspace(self.s_rows, self.t_rows, self.n, dev)

    def head_args(self):
        m = self.meta
        return (_p(self.src), _p(self.tgt), _p(m[0], torch.int32), _p(m[1], torch.int32), _p(m[2], torch.int32), _p(m[3], torch.int32),
                self.n, self.max_s_len, self.max_t_len, self.s_rows, self.t_rows)


def _upload(c, i, what, dev):
    if isinstance(c, np.ndarray):
        if c.dtype != np.float32:
            raise TypeError("%s %d: expected float32, got %s" % (what, i, c.dtype))
        c = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    return c


def _poses(T, n, dev) -> torch.Tensor:
    """float64 [n,4,4] on the device, the caller's own copy: the loop updates it in place."""
    if isinstance(T, torch.Tensor) and T.dtype != torch.float64:
        raise TypeError("poses: expected float64, got %s" % T.dtype)
    return pose_stack(T, n, dev, "poses", ValueError, copy=True)


def _refused(status, what):
    bad = [i for i, s in enumerate(status) if s < 0]
    if bad:
        raise ScreamHipError("%s: pair %s refused (status -1): its target spans more than 2^21 cells of the radius on an axis, a "
                             "coordinate is not finite, or the radius is not a positive finite number" % (what, ", ".join(map(str, bad))))


class RawIcpRun(PiecewiseRun):
    """One batched run of scream_icp_raw_range, enqueued in pieces (ops.PiecewiseRun): a step is one iteration (one search launch
    and one pose launch), max_iter + 1 of them at most.  ``iterations`` counts what was enqueued.  ``T`` / ``fitness_rmse`` /
    ``iters`` are complete for every pair whose flag is set; iters = -1 marks a refused pair, whose T is its start pose."""

    def __init__(self, srcs, tgts, T_inits, max_corr_dist: float = 0.2, max_iter: int = 50000, rel_fitness: float = 1e-6,
                 rel_rmse: float = 1e-6):
        self.pk = _RawClouds(srcs, tgts)
        n, dev = self.pk.n, self.pk.dev
        self.max_iter, self.iterations = int(max_iter), 0
        if self.max_iter < 0:
            raise ValueError("max_iter must not be negative")
        super().__init__(n, self.max_iter + 1, dev, skip_empty=True)
        self.T = _poses(T_inits, n, dev)
        self.fitness_rmse = torch.zeros(max(n, 1), 2, device=dev, dtype=torch.float64)[:n]
        self.iters = torch.zeros(max(n, 1), device=dev, dtype=torch.int32)[:n]
        self._tail = (max_corr_dist, self.max_iter, rel_fitness, rel_rmse, self.T, self.fitness_rmse, self.iters)

    iterations_left = PiecewiseRun.steps_left

    def _enqueue(self, begin: int, end: int) -> None:
        call("scream_icp_raw_range", *self.pk.head_args(), *self._tail, begin, end, self.flags, self.pk.ws, self.pk.ws.numel())
        self.iterations += end - begin


def icp_raw_batch(srcs, tgts, T_inits, max_corr_dist: float = 0.2, max_iter: int = 50000, rel_fitness: float = 1e-6,
                  rel_rmse: float = 1e-6, piece: int = 32, strict: bool = True):
    """Refine T_inits [n,4,4] float64 so that T maps srcs[i] onto tgts[i] ([N,3] fp32, torch tensors on the GPU or numpy arrays).
    Returns (T float64 [n,4,4], fitness_rmse float64 [n,2], iters int32 [n]) on the device, bitwise independent of `piece` and
    of the other pairs.  A refused pair (iters = -1) raises ScreamHipError naming it; with strict=False the call returns
    (T, fitness_rmse, iters, status int32 [n]) instead, a refused pair keeping its start pose."""
    run = RawIcpRun(srcs, tgts, T_inits, max_corr_dist, max_iter, rel_fitness, rel_rmse).run(piece)
    iters = run.iters.cpu()
    status = torch.where(iters < 0, -1, 0).to(torch.int32)
    if strict:
        _refused(status.tolist(), "icp_raw_batch")
        return run.T, run.fitness_rmse, run.iters
    return run.T, run.fitness_rmse, run.iters, status


def raw_nn_batch(srcs, tgts, Ts, radius: float, strict: bool = True):
    """The search of the loop alone: for every row of srcs[i] under Ts[i] (float64 [n,4,4]) the nearest row of tgts[i] with
    d2 < radius^2 strictly.  Returns (list of idx int32 [N_i], -1 for none; list of d2 float64 [N_i], +inf for none) on the
    device; with strict=False also the status array, a refused pair's rows reading -1 / +inf."""
    pk = _RawClouds(srcs, tgts)
    n, dev = pk.n, pk.dev
    if n == 0:
        return ([], []) if strict else ([], [], torch.zeros(0, dtype=torch.int32))
    T = _poses(Ts, n, dev)
    idx = torch.full((max(pk.s_rows, 1),), -1, device=dev, dtype=torch.int32)
    d2 = torch.full((max(pk.s_rows, 1),), float("inf"), device=dev, dtype=torch.float64)
    status = torch.zeros(n, device=dev, dtype=torch.int32)
    call("scream_icp_raw_nn", *pk.head_args(), radius, T, idx, d2, status, pk.ws, pk.ws.numel())
    status = status.cpu()
    out_i, out_d = pk.split_src(idx, clone=False), pk.split_src(d2, clone=False)
    if strict:
        _refused(status.tolist(), "raw_nn_batch")
        return out_i, out_d
    return out_i, out_d, status
