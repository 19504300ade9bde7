"""The host layer every op on a LIST of clouds shares (voxel.py, dsm.py, overlap.py, prep.py, rawicp.py): what a cloud must be,
the packing of a list into one [rows,3] array with row0 / len per cloud as the C ABI reads it (include/scream_hip.h), the single
upload of those integers, the radius rule and the stack of 4x4 poses.  Pure torch / numpy: nothing here calls the library.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from ._lib import ScreamHipError

__all__ = ["check_clouds", "pack_clouds", "PackedPairs", "check_radius", "pose_stack"]


def check_clouds(clouds: Sequence[torch.Tensor], what: str, dtypes=(torch.float32,), op: str = "this op", builtin_errors: bool = False):
    """Every cloud a [N,3] tensor on the GPU, all of ONE dtype out of `dtypes`; returns that dtype (None for an empty list).
    Raises ScreamHipError naming `what` and the cloud's index -- with builtin_errors a ValueError for a wrong shape and a TypeError
    for a wrong dtype instead (voxel.py and rawicp.py promise those); a cloud that is not on the GPU is always a ScreamHipError."""
    shape_error, dtype_error = (ValueError, TypeError) if builtin_errors else (ScreamHipError, ScreamHipError)
    dtype = None
    for i, c in enumerate(clouds):
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
            raise shape_error("%s %d: expected a [N,3] tensor, got %s" % (what, i, tuple(getattr(c, "shape", ()))))
        if not c.is_cuda:
            raise ScreamHipError("%s needs tensors on the MI355X (%s %d is on %s); there is no CPU path" % (op, what, i, c.device))
        if c.dtype not in dtypes or (dtype is not None and c.dtype != dtype):
            raise dtype_error("%s %d: expected %s%s, got %s" % (what, i, " or ".join(str(d) for d in dtypes),
                                                               " (all clouds alike)" if len(dtypes) > 1 else "", c.dtype))
        dtype = c.dtype
    return dtype


def pack_clouds(clouds: Sequence[torch.Tensor], pad_device=None) -> Tuple[torch.Tensor, List[int], List[int]]:
    """(rows [sum N_i,3], row0, lens): the clouds back to back and, as Python ints, every cloud's first row and length.
    pad_device: a list without a single row packs to ONE zero row on that device, for a call that needs an address anyway."""
    clouds = [c.detach() for c in clouds]
    lens = [int(c.shape[0]) for c in clouds]
    row0 = [0] * len(clouds)
    for i in range(1, len(clouds)):
        row0[i] = row0[i - 1] + lens[i - 1]
    if pad_device is not None and sum(lens) == 0:
        clouds = clouds + [torch.zeros(1, 3, device=pad_device, dtype=torch.float32)]
    if not clouds:
        return torch.zeros(0, 3, dtype=torch.float32), row0, lens
    return torch.cat(clouds, dim=0).contiguous(), row0, lens


class PackedPairs:
    """The two sides of a list of pairs packed (pack_clouds) and their integers uploaded ONCE: meta int32 [4,n] on the device =
    s_row0 | s_len | t_row0 | t_len.  pad: an all-empty side gets one zero row."""

    def __init__(self, srcs: Sequence[torch.Tensor], tgts: Sequence[torch.Tensor], dev, pad: bool = False):
        self.n, self.dev = len(srcs), dev
        self.src, self.s_row0, self.s_len = pack_clouds(srcs, dev if pad else None)
        self.tgt, self.t_row0, self.t_len = pack_clouds(tgts, dev if pad else None)
        self.s_rows, self.t_rows = sum(self.s_len), sum(self.t_len)
        self.meta = torch.tensor([self.s_row0, self.s_len, self.t_row0, self.t_len], dtype=torch.int32).reshape(4, self.n).to(dev)

    @property
    def max_s_len(self) -> int:
        return max(self.s_len, default=0)

    @property
    def max_t_len(self) -> int:
        return max(self.t_len, default=0)

    def split_src(self, rows: torch.Tensor, lens=None, clone: bool = True) -> List[torch.Tensor]:
        """A packed per-source-row result back as one tensor per pair (`lens`: other lengths than the sources')."""
        return _split(rows, self.s_row0, self.s_len if lens is None else lens, clone)

    def split_tgt(self, rows: torch.Tensor, lens=None, clone: bool = True) -> List[torch.Tensor]:
        return _split(rows, self.t_row0, self.t_len if lens is None else lens, clone)


def _split(rows, row0, lens, clone):
    return [rows[r:r + n].clone() if clone else rows[r:r + n] for r, n in zip(row0, lens)]


def check_radius(radius, what: str = "the radius", error=ScreamHipError) -> float:
    """float(radius) if it is positive and finite, else `error` (0, a negative number, inf and nan are all refused)."""
    radius = float(radius)
    if not radius > 0 or radius == float("inf"):
        raise error("%s must be a positive finite number, got %r" % (what, radius))
    return radius


def pose_stack(T, n: int, dev, what: str = "transform", error=ScreamHipError, copy: bool = False) -> torch.Tensor:
    """n 4x4 matrices -- a sequence of arrays or tensors, one [n,4,4] array or one [n,4,4] tensor -- as float64 [n,4,4] on the
    device.  Nothing is rounded (narrower types convert exactly); a tensor that is on the device already stays there.  copy: the
    result never aliases the input (for a caller that updates it in place).  A wrong shape or count raises `error`."""
    if not isinstance(T, (torch.Tensor, np.ndarray)):
        mats = [m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in T]
        for i, m in enumerate(mats):
            if m.shape != (4, 4):
                raise error("%s %d: expected a 4x4 matrix, got %s" % (what, i, m.shape))
        T = np.stack(mats, axis=0) if mats else np.zeros((0, 4, 4))
    if tuple(T.shape) != (n, 4, 4):
        raise error("%s: expected %d 4x4 matrices, got %s" % (what, n, tuple(T.shape)))
    if isinstance(T, np.ndarray):
        T = torch.from_numpy(np.array(T, dtype=np.float64))  # a copy: from_numpy wants a writable array
    out = T.detach().to(device=dev, dtype=torch.float64).contiguous()
    return out.clone() if copy else out
