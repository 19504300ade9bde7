"""Yardstick of train_backend = "bf16" (include/scream_hip.h: one bf16 product per training GEMM, fp32 accumulation): the
arithmetic restated for the CPU oracle, in any dtype.

  r(x)            fp32 -> bf16 -> back, round to nearest even (a float64 value goes through fp32 first, as on the GPU, where
                  every operand IS an fp32 value in memory).
  RoundedProduct  y = r(x) r(W)^T for W [N,K]; backward dx = r(dy) r(W), dW = r(dy)^T r(x).  The products of the rounded values
                  and their sums are taken in the dtype of the operands: exact up to that dtype's own accumulation.
  rounded_gemms() a TorchFunctionMode that routes every `x @ B` whose B is a 2-D matrix with both dimensions >= 64 through
                  RoundedProduct -- the oracle's projections, merge, FFN and coor_mlp.0 / .2.  The K = 3 embedding, the N = 3
                  head and the attention einsums stay exact, as on the GPU.  drop: what to leave UNROUNDED ("x", "w" or "dy"),
                  for the tests that show the bar can see one missing rounding.  order: None (one matmul), or "natural" /
                  "reversed": the contraction summed in 64-wide chunks, first to last or last to first -- two realisations of
                  the same arithmetic that differ in accumulation order alone.

Under the mode tests/train_ref.py's oracle_grads / dem_oracle_grads are the float64 and fp32 restatements of the GPU's
arithmetic; they take masks and signs as before."""
import torch
from torch.overrides import TorchFunctionMode

MIN_DIM = 64


def r(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def r_bits(x: torch.Tensor) -> torch.Tensor:
    """r() of an fp32 tensor on the bit pattern: add 0x7FFF + (bit 16), clear the low 16 bits.  Finite inputs only."""
    assert x.dtype == torch.float32
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)
    return u.view(torch.float32).view(x.shape)


def _mm(a, b, order):
    """a @ b, the contraction (a's last, b's first dimension) in one piece or in 64-wide chunks added in `order`."""
    if order is None:
        return a @ b
    starts = list(range(0, b.shape[0], MIN_DIM))
    out = None
    for c in (starts if order == "natural" else reversed(starts)):
        part = a[..., c:c + MIN_DIM] @ b[c:c + MIN_DIM]
        out = part if out is None else out + part
    return out


class RoundedProduct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, drop, order=None):
        with torch._C.DisableTorchFunction():
            rx = x if "x" in drop else r(x)
            rw = W if "w" in drop else r(W)
            ctx.save_for_backward(rx, rw)
            ctx.drop, ctx.order = drop, order
            return _mm(rx, rw.t(), order)

    @staticmethod
    def backward(ctx, dy):
        with torch._C.DisableTorchFunction():
            rx, rw = ctx.saved_tensors
            rdy = dy if "dy" in ctx.drop else r(dy)
            dx = _mm(rdy, rw, ctx.order)
            dW = _mm(rdy.reshape(-1, rdy.shape[-1]).t(), rx.reshape(-1, rx.shape[-1]), ctx.order)
            return dx, dW, None, None


def point_batch_grads(sd, pairs, dtype, masks):
    """{name: gradient} of the MEAN of point_loss over `pairs` (train_ref.make_pair tuples), each under its own dict of
    `masks`, from ONE backward of that mean -- to be called under rounded_gemms().  Averaging per-pair gradients afterwards
    (train_ref.masked_oracles) restates the fp32-accurate backends, whose backward is linear in the loss's gradient; this
    arithmetic is not: r(dy / 3) is not r(dy) / 3, so the factor 1 / B has to stand where the training loop puts it, on the
    loss, in front of every rounding of the backward pass.  (A power of two commutes with r: one pair, or a GradScaler.)"""
    from oracle import scream_ref as O
    sdx = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in sd.items()}
    c = lambda t: t.to(dtype)
    losses = []
    for (src, tgt, rot, trans), m in zip(pairs, masks):
        relu = {k: v for k, v in m.items() if k != "sign"}
        pred = O.point_transformer_forward(c(src), c(tgt), sdx, c(trans).permute(0, 2, 1), masks=relu)
        losses.append(O.point_loss(pred, c(src), c(rot), c(trans), m["sign"]))
    torch.stack(losses).mean().backward()
    return {k: v.grad for k, v in sdx.items()}


class rounded_gemms(TorchFunctionMode):
    def __init__(self, drop=(), order=None):
        super().__init__()
        self.drop, self.order = tuple(drop), order
        self.routed = 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func in (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__) and len(args) == 2 and not kwargs:
            a, b = args
            if isinstance(b, torch.Tensor) and b.dim() == 2 and min(b.shape) >= MIN_DIM and a.dim() >= 2:
                self.routed += 1
                return RoundedProduct.apply(a, b.t(), self.drop, self.order)
        return func(*args, **(kwargs or {}))
