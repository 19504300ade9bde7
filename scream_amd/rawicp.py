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

from typing import List, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import ScreamHipError, check
from .ops import _p, _stream

__all__ = ["icp_raw_batch", "raw_nn_batch", "RawIcpRun"]


def _device():
    if not torch.cuda.is_available():
        raise ScreamHipError("the raw-scan ICP needs the MI355X; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _cloud(c, i, what, dev) -> torch.Tensor:
    if isinstance(c, np.ndarray):
        if c.dtype != np.float32:
            raise TypeError("%s %d: expected float32, got %s" % (what, i, c.dtype))
        c = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
        raise ValueError("%s %d: expected a [N,3] array, got %s" % (what, i, tuple(getattr(c, "shape", ()))))
    if not c.is_cuda:
        raise ScreamHipError("%s %d is on %s; the raw-scan ICP needs tensors on the MI355X (there is no CPU path)" % (what, i, c.device))
    if c.dtype != torch.float32:
        raise TypeError("%s %d: expected torch.float32, got %s" % (what, i, c.dtype))
    return c.detach()


class _Packed:
    """The clouds of a call packed into two [rows,3] arrays with row0 / len per pair."""

    def __init__(self, srcs: Sequence, tgts: Sequence):
        srcs, tgts = list(srcs), list(tgts)
        if len(srcs) != len(tgts):
            raise ValueError("%d source clouds for %d target clouds" % (len(srcs), len(tgts)))
        first = next((c for c in srcs + tgts if isinstance(c, torch.Tensor) and c.is_cuda), None)
        self.dev = first.device if first is not None else _device()
        self.n = len(srcs)
        srcs = [_cloud(c, i, "source cloud", self.dev) for i, c in enumerate(srcs)]
        tgts = [_cloud(c, i, "target cloud", self.dev) for i, c in enumerate(tgts)]
        self.src_len, self.tgt_len = [int(c.shape[0]) for c in srcs], [int(c.shape[0]) for c in tgts]
        self.src_row0 = [int(v) for v in np.concatenate([[0], np.cumsum(self.src_len)[:-1]])] if self.n else []
        self.tgt_row0 = [int(v) for v in np.concatenate([[0], np.cumsum(self.tgt_len)[:-1]])] if self.n else []
        self.src_rows, self.tgt_rows = sum(self.src_len), sum(self.tgt_len)
        pad = torch.zeros(1, 3, device=self.dev, dtype=torch.float32)  # an all-empty side still needs an address
        self.src = torch.cat(srcs + ([pad] if self.src_rows == 0 else []), dim=0).contiguous()
        self.tgt = torch.cat(tgts + ([pad] if self.tgt_rows == 0 else []), dim=0).contiguous()
        self.meta = torch.tensor([self.src_row0, self.src_len, self.tgt_row0, self.tgt_len], dtype=torch.int32).reshape(4, self.n).to(self.dev)
        need = _lib.load().scream_icp_raw_workspace_bytes(self.src_rows, self.tgt_rows, self.n)
        if need < 0:
            raise ScreamHipError("scream_icp_raw_workspace_bytes(%d, %d, %d): invalid argument" % (self.src_rows, self.tgt_rows, self.n))
        self.ws = torch.empty(max(need, 256), device=self.dev, dtype=torch.uint8)

    def head_args(self):
        m = self.meta
        return (_p(self.src), _p(self.tgt), _p(m[0], torch.int32), _p(m[1], torch.int32), _p(m[2], torch.int32), _p(m[3], torch.int32),
                self.n, max(self.src_len), max(self.tgt_len), self.src_rows, self.tgt_rows)


def _poses(T, n, dev) -> torch.Tensor:
    T = torch.as_tensor(np.asarray(T, dtype=np.float64) if not isinstance(T, torch.Tensor) else T)
    if T.dtype != torch.float64:
        raise TypeError("poses: expected float64, got %s" % T.dtype)
    if tuple(T.shape) != (n, 4, 4):
        raise ValueError("poses: expected [%d,4,4], got %s" % (n, tuple(T.shape)))
    return T.detach().to(dev).clone().contiguous()


def _refused(status, what):
    bad = [i for i, s in enumerate(status) if s < 0]
    if bad:
        raise ScreamHipError("%s: pair %s refused (status -1): its target spans more than 2^21 cells of the radius on an axis, a "
                             "coordinate is not finite, or the radius is not a positive finite number" % (what, ", ".join(map(str, bad))))


class RawIcpRun:
    """One batched run of scream_icp_raw_range, enqueued in pieces like ops.IcpRun: ``advance(k)`` enqueues the next k iterations
    (one search launch and one pose launch each) and, behind them, a copy of the per-pair stopped flags into pinned memory with an
    event; ``all_stopped()`` waits for that event only.  ``iterations`` counts what was enqueued.  ``T`` / ``fitness_rmse`` /
    ``iters`` are complete for every pair whose flag is set; iters = -1 marks a refused pair, whose T is its start pose."""

    def __init__(self, srcs, tgts, T_inits, max_corr_dist: float = 0.2, max_iter: int = 50000, rel_fitness: float = 1e-6,
                 rel_rmse: float = 1e-6):
        self.lib = _lib.load()
        self.pk = _Packed(srcs, tgts)
        n, dev = self.pk.n, self.pk.dev
        self.n, self.max_iter, self.next_it, self.iterations = n, int(max_iter), 0, 0
        if self.max_iter < 0:
            raise ValueError("max_iter must not be negative")
        self.T = _poses(T_inits, n, dev)
        self.fitness_rmse = torch.zeros(max(n, 1), 2, device=dev, dtype=torch.float64)[:n]
        self.iters = torch.zeros(max(n, 1), device=dev, dtype=torch.int32)[:n]
        self.flags = torch.zeros(max(n, 1), device=dev, dtype=torch.int32)[:n]
        self.flags_host = torch.zeros(max(n, 1), dtype=torch.int32, pin_memory=True)[:n]
        self._tail = (float(max_corr_dist), self.max_iter, float(rel_fitness), float(rel_rmse), _p(self.T, torch.float64),
                      _p(self.fitness_rmse, torch.float64), _p(self.iters, torch.int32))
        self.event = None

    @property
    def iterations_left(self) -> int:
        return self.max_iter + 1 - self.next_it

    def advance(self, k: int) -> None:
        if self.n == 0:
            self.next_it = self.max_iter + 1
            return
        end = min(self.next_it + int(k), self.max_iter + 1)
        check(self.lib.scream_icp_raw_range(*self.pk.head_args(), *self._tail, self.next_it, end, _p(self.flags, torch.int32),
                                            self.pk.ws.data_ptr(), self.pk.ws.numel(), _stream()), "scream_icp_raw_range")
        self.iterations += end - self.next_it
        self.next_it = end
        self.flags_host.copy_(self.flags, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(self.pk.dev))

    def all_stopped(self) -> bool:
        if self.n == 0:
            return True
        self.event.synchronize()
        return self.iterations_left == 0 or bool(self.flags_host.all())

    def run(self, piece: int = 32) -> "RawIcpRun":
        """Enqueue pieces until every pair has stopped: after each piece the host waits for that piece's flags (its event, not the
        stream) and enqueues the next one only if a pair still runs, so no more than ceil((iters + 1) / piece) pieces are launched."""
        if piece < 1:
            raise ValueError("piece must be at least 1")
        self.advance(piece)
        while not self.all_stopped():
            self.advance(piece)
        return self


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
    pk = _Packed(srcs, tgts)
    n, dev = pk.n, pk.dev
    if n == 0:
        return ([], []) if strict else ([], [], torch.zeros(0, dtype=torch.int32))
    T = _poses(Ts, n, dev)
    idx = torch.full((max(pk.src_rows, 1),), -1, device=dev, dtype=torch.int32)
    d2 = torch.full((max(pk.src_rows, 1),), float("inf"), device=dev, dtype=torch.float64)
    status = torch.zeros(n, device=dev, dtype=torch.int32)
    check(_lib.load().scream_icp_raw_nn(*pk.head_args(), float(radius), _p(T, torch.float64), _p(idx, torch.int32), _p(d2, torch.float64),
                                        _p(status, torch.int32), pk.ws.data_ptr(), pk.ws.numel(), _stream()), "scream_icp_raw_nn")
    status = status.cpu()
    out_i: List[torch.Tensor] = [idx[r:r + m] for r, m in zip(pk.src_row0, pk.src_len)]
    out_d: List[torch.Tensor] = [d2[r:r + m] for r, m in zip(pk.src_row0, pk.src_len)]
    if strict:
        _refused(status.tolist(), "raw_nn_batch")
        return out_i, out_d
    return out_i, out_d, status
