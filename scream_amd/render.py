"""RegistrationRender: the reference's depth renderer (models/render.py:8-73) on the HIP kernels of csrc/render.hip.

    gen = RegistrationRender(rho=24, w=64)            # six views ("muti"), or view="single" for the identity
    imgs = gen(src_pred, tgt)                          # [n,3], [m,3] on the MI355X -> [V, 2, w, w], differentiable in src_pred

The module owns no parameters and no buffers (the models' state_dict keys stay the reference's) and consumes no random numbers.
``eulers`` is a public list that callers may reassign (the reference's visualize_depth_image.py does); the view matrices follow
it at call time and equal the reference's ``torch.Tensor(Rotation.from_euler('zyx', e).as_matrix())`` bit for bit, built with
scipy's own quaternion arithmetic so that scipy is not needed.  Rules the reference leaves open (ties, zero pixels, flat views)
are stated in include/scream_hip.h.  There is no CPU path: CPU tensors raise ScreamHipError.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib, ops


def _quat_zyx(e) -> Tuple[float, float, float, float]:
    """scipy's Rotation.from_euler('zyx', e) (extrinsic): elementary quaternions composed left to right, (x, y, z, w)."""
    def elem(axis, a):
        q = [0.0, 0.0, 0.0, math.cos(a / 2)]
        q[axis] = math.sin(a / 2)
        return q

    def compose(p, q):  # p * q
        c = (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])
        return [p[3] * q[0] + q[3] * p[0] + c[0], p[3] * q[1] + q[3] * p[1] + c[1], p[3] * q[2] + q[3] * p[2] + c[2],
                p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]]

    r = elem(2, float(e[0]))
    r = compose(elem(1, float(e[1])), r)
    return tuple(compose(elem(0, float(e[2])), r))


def rotation_matrix(e) -> torch.Tensor:
    """fp32 [3,3] equal to torch.Tensor(Rotation.from_euler('zyx', e).as_matrix()) bit for bit (scipy's as_matrix formula)."""
    x, y, z, w = _quat_zyx(e)
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.array([[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                  [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                  [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]])
    return torch.from_numpy(m.astype(np.float32))


def view_eulers(view: str = "muti"):
    """render.py:17-25: six views (rotations about y, then about x) or the identity."""
    if view == "muti":
        return [np.array([0, 0, 0]), np.array([0, np.pi / 2, 0]), np.array([0, np.pi, 0]), np.array([0, np.pi * 3 / 2, 0]),
                np.array([0, 0, np.pi / 2]), np.array([0, 0, np.pi * 3 / 2])]
    return [np.array([0, 0, 0])]


class _RenderPackedFn(torch.autograd.Function):
    """imgs [B*V,2,w,w] of B packed pairs; the backward is the packed scream_render_depth_bwd, which routes each source-image
    pixel's gradient to its argmax point."""

    @staticmethod
    def forward(ctx, src, s_row0, s_len, tgt, t_row0, t_len, max_s_len, max_t_len, rot, w, rho):
        src = src.detach().to(torch.float32).contiguous()
        tgt = tgt.detach().to(torch.float32).contiguous()
        B, V = s_row0.shape[0], rot.shape[0]
        ws = ops.render_workspace(B, V, w, src.shape[0], src.device)
        imgs, argmax = ops.render_depth(src, s_row0, s_len, tgt, t_row0, t_len, max_s_len, max_t_len, rot, w, rho, ws)
        ctx.save_for_backward(src, s_row0, s_len, rot, argmax, ws)
        ctx.geo = (B, V, int(max_s_len), int(w), float(rho))
        return imgs.view(B * V, 2, w, w)

    @staticmethod
    def backward(ctx, dimgs):
        src, s_row0, s_len, rot, argmax, ws = ctx.saved_tensors
        B, V, max_s_len, w, rho = ctx.geo
        dsrc = ops.render_depth_bwd(dimgs.to(torch.float32).contiguous().view(B, V, 2, w, w), argmax, src, s_row0, s_len, max_s_len, rot,
                                    w, rho, ws)
        return (dsrc,) + (None,) * 10


class RegistrationRender(nn.Module):
    def __init__(self, rho, w, view="muti"):
        super().__init__()
        if int(w) != w or w <= 0 or w % 64:
            raise ValueError("RegistrationRender renders in 64 x 64 chunks (render.py:33-34): w must be a positive multiple of 64, "
                             "got %r" % (w,))
        self.rho, self.w = rho, int(w)
        self.eulers = view_eulers(view)
        self._dev_cache: Dict[tuple, torch.Tensor] = {}  # (device, key) -> device tensor (no state_dict entry)

    def view_matrices(self, device=None) -> torch.Tensor:
        """[V,3,3] fp32 of the current ``eulers`` (on `device` when given; cached per euler list)."""
        key = tuple(np.asarray(e, dtype=np.float64).tobytes() for e in self.eulers)
        if not key:
            raise ValueError("RegistrationRender.eulers is empty: at least one view is needed")
        dkey = ("rot", None if device is None else torch.device(device), key)
        t = self._dev_cache.get(dkey)
        if t is None:
            t = torch.stack([rotation_matrix(e) for e in self.eulers])
            t = t.to(device) if device is not None else t
            if len(self._dev_cache) > 64:
                self._dev_cache.clear()
            self._dev_cache[dkey] = t
        return t

    def _meta(self, n: int, m: int, device) -> torch.Tensor:
        """int32 [s_row0, s_len, t_row0, t_len] of one pair on the device (cached per cloud sizes)."""
        dkey = ("meta", torch.device(device), n, m)
        t = self._dev_cache.get(dkey)
        if t is None:
            if len(self._dev_cache) > 64:
                self._dev_cache.clear()
            t = self._dev_cache[dkey] = torch.tensor([0, n, 0, m], dtype=torch.int32).to(device)
        return t

    def forward(self, src_pred, tgt_pcd):
        """src_pred [n,3], tgt_pcd [m,3] -> [V, 2, w, w] (channel 0 the source image, 1 the target image)."""
        if src_pred.dim() != 2 or src_pred.shape[1] != 3 or tgt_pcd.dim() != 2 or tgt_pcd.shape[1] != 3:
            raise ValueError("RegistrationRender takes src_pred [n,3] and tgt_pcd [m,3], got %s and %s"
                             % (tuple(src_pred.shape), tuple(tgt_pcd.shape)))
        if src_pred.shape[0] == 0 or tgt_pcd.shape[0] == 0:
            raise ValueError("every cloud needs at least one point")
        if not src_pred.is_cuda or not tgt_pcd.is_cuda:
            raise _lib.ScreamHipError("RegistrationRender needs tensors on the MI355X (got %s, %s); there is no CPU path"
                                      % (src_pred.device, tgt_pcd.device))
        if torch.is_grad_enabled() and tgt_pcd.requires_grad:
            raise ValueError("RegistrationRender differentiates src_pred only: pass tgt_pcd detached (no caller needs its gradient)")
        n, m, dev = src_pred.shape[0], tgt_pcd.shape[0], src_pred.device
        meta = self._meta(n, m, dev)  # the one pair as a packed batch of one: B * V = V images
        return _RenderPackedFn.apply(src_pred, meta[0:1], meta[1:2], tgt_pcd, meta[2:3], meta[3:4], n, m, self.view_matrices(dev),
                                     self.w, float(self.rho))


def render_packed(src: torch.Tensor, s_row0, s_len, tgt: torch.Tensor, t_row0, t_len, max_s_len: int, max_t_len: int,
                  eulers: Sequence, w: int = 64, rho: float = 24.0) -> torch.Tensor:
    """B pairs in one launch set (no autograd): packed rows as ops.render_depth takes them -> imgs [B, V, 2, w, w]."""
    rot = torch.stack([rotation_matrix(e) for e in eulers]).to(src.device)
    return ops.render_depth(src, s_row0, s_len, tgt, t_row0, t_len, max_s_len, max_t_len, rot, w, rho)[0]


def render_packed_train(src: torch.Tensor, s_row0, s_len, tgt: torch.Tensor, t_row0, t_len, max_s_len: int, max_t_len: int,
                        eulers: Sequence, w: int = 64, rho: float = 24.0, rot: torch.Tensor = None) -> torch.Tensor:
    """render_packed with a grad_fn into the packed source rows `src` (a packed prediction): imgs [B*V, 2, w, w], the batch a
    discriminator takes, pair-major.  The target is data.  rot: the [V,3,3] view matrices already on the device
    (RegistrationRender.view_matrices), instead of building and uploading them from `eulers`."""
    if not src.is_cuda or not tgt.is_cuda:
        raise _lib.ScreamHipError("render_packed_train needs tensors on the MI355X (got %s, %s); there is no CPU path"
                                  % (src.device, tgt.device))
    if rot is None:
        rot = torch.stack([rotation_matrix(e) for e in eulers]).to(src.device)
    return _RenderPackedFn.apply(src, s_row0, s_len, tgt, t_row0, t_len, int(max_s_len), int(max_t_len), rot, int(w), float(rho))
