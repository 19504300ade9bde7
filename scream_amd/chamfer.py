"""The Chamfer distance on the MI355X (csrc/chamfer.hip): batched over packed clouds, differentiable, bitwise repeatable.

    loss = chamfer_packed(a, a_row0, a_len, b, b_row0, b_len, max_a_len, max_b_len)    # packed [rows,3] clouds, B pairs
    loss = ChamferDistance()(f, f_)                                                    # the reference's module: [B,N,3], [B,M,3]
    loss.backward()

The reference's ChamferDistance (evaluate_open_gf.py:25-41) is square_distance, two min and two means.  Here the squared distance
is the difference form ((dx dx + dy dy) + dz dz) in fp32, which does not cancel where the expansion -2ab + |a|^2 + |b|^2 does,
ties go to the lowest index, and every sum is float64 in a fixed order (include/scream_hip.h states each operation,
tests/chamfer_ref.py restates them in numpy).  One launch set serves both directions of every pair; the backward is a second
launch set that re-scans the forward's indices, without atomics.  Nothing is copied to the host.  There is no CPU path.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib, ops

__all__ = ["chamfer_packed", "ChamferDistance"]


class _ChamferPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, a_row0, a_len, b_row0, b_len, max_a_len, max_b_len):
        a, b = a.contiguous(), b.contiguous()
        loss, loss_pair, idx_ab, _, idx_ba, _ = ops.chamfer_fwd(a, a_row0, a_len, max_a_len, b, b_row0, b_len, max_b_len)
        ctx.save_for_backward(a, b, a_row0, a_len, b_row0, b_len, idx_ab, idx_ba)
        ctx.max_len = (max_a_len, max_b_len)
        ctx.mark_non_differentiable(loss_pair)
        return loss, loss_pair

    @staticmethod
    def backward(ctx, dout, _dpair):
        a, b, a_row0, a_len, b_row0, b_len, idx_ab, idx_ba = ctx.saved_tensors
        da, db = ops.chamfer_bwd(dout.to(torch.float32).contiguous(), a, a_row0, a_len, ctx.max_len[0], b, b_row0, b_len, ctx.max_len[1],
                                 idx_ab, idx_ba, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (da if ctx.needs_input_grad[0] else None, db if ctx.needs_input_grad[1] else None) + (None,) * 6


def chamfer_packed(a: torch.Tensor, a_row0: torch.Tensor, a_len: torch.Tensor, b: torch.Tensor, b_row0: torch.Tensor,
                   b_len: torch.Tensor, max_a_len: int, max_b_len: int, return_pairs: bool = False):
    """The mean over B pairs of mean_n min_m |a_n - b_m|^2 + mean_m min_n |a_n - b_m|^2.  a [a_rows,3] and b [b_rows,3] are fp32
    packed clouds on the GPU; a_row0 / a_len / b_row0 / b_len int32 [B] on the device name each pair's rows; max_a_len / max_b_len
    are host bounds of the lengths.  A pair with an empty side counts 0 (the reference's `if f.shape[1] == 0: return 0`).
    Returns an fp32 scalar with a grad_fn into whichever of a and b requires one; with return_pairs also the float64 [B] values of
    the pairs (no gradient).  Rows outside every cloud get a zero gradient."""
    for name, t in (("a", a), ("b", b)):
        if not t.is_cuda or t.dtype != torch.float32:
            raise _lib.ScreamHipError("chamfer_packed: %s must be an fp32 tensor on the GPU, got %s on %s" % (name, t.dtype, t.device))
    loss, loss_pair = _ChamferPacked.apply(a, b, a_row0, a_len, b_row0, b_len, int(max_a_len), int(max_b_len))
    return (loss, loss_pair) if return_pairs else loss


class ChamferDistance(nn.Module):
    """The reference's module (evaluate_open_gf.py:25-41) on the packed kernel: forward(f [B,N,3], f_ [B,M,3]) -> the mean over
    the batch, with a grad_fn; f.shape[1] == 0 returns 0."""

    def forward(self, f: torch.Tensor, f_: torch.Tensor):
        if f.shape[1] == 0:
            return 0
        B, N, M = f.shape[0], f.shape[1], f_.shape[1]
        if f_.shape[0] != B or f.shape[2] != 3 or f_.dim() != 3 or f_.shape[2] != 3:
            raise _lib.ScreamHipError("ChamferDistance takes [B,N,3] and [B,M,3], got %s and %s" % (tuple(f.shape), tuple(f_.shape)))
        pair = torch.arange(B, device=f.device, dtype=torch.int32)
        return chamfer_packed(f.reshape(B * N, 3), pair * N, torch.full_like(pair, N), f_.reshape(B * M, 3), pair * M,
                              torch.full_like(pair, M), N, M)
