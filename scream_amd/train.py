"""Training of PointTransformer and DEMTransformer: a forward that keeps its activations, and the backward pass on the
HIP kernels of csrc/backward.hip, wired into torch.autograd.

Three arithmetics for the matrix products, one class each (ARITHMETICS), chosen per model by net.train_backend through gemms();
every other kernel is the same fp32 code:
  "f32"    F32Gemms (default): every product on the fp32-input MFMA: scream_gemm_f32 forward and data gradients, scream_gemm_wgrad_f32.
  "split"  SplitGemms: fp32-accurate products on the 16-bit matrix cores with fp32 accumulation (csrc/split.h, SplitBf3: three
           bf16 planes, six products, scale free -- gradients of any magnitude, a GradScaler's 2^16 included, need no
           exponent): forward and data gradients on scream_gemm_split_f32 against weights packed per step by
           scream_pack_w_split, weight gradients on scream_gemm_wgrad_split_f32.  A data gradient whose summed dimension the
           split GEMM does not take (split_gemm_takes_k: K = 768 of the self layers' q|k|v, K = 512 of the cross layers' k|v)
           runs as K = 256 products added in column order.
  "bf16"   Bf16Gemms: mixed precision, ONE bf16 product per GEMM with fp32 accumulation (csrc/gemm_bf16.hip;
           include/scream_hip.h states the arithmetic), the mirror of the reference's autocast training in bf16 instead of
           fp16.  NOT fp32-accurate.  The operands stay fp32 in memory (saved activations included) and are rounded in
           registers; the weights are read in torch's [N,K] layout by all three products, so nothing is packed or transposed
           per step and every data gradient is one launch: scream_gemm_bf16_f32, scream_gemm_dgrad_bf16_f32, scream_gemm_wgrad_bf16_f32.

The forward is the unfused fp32 chain of the existing kernels (scream_pe_embed + scream_ln_fwd, scream_gemm_f32 with the
elu + 1 / relu / bias + relu epilogues, scream_kv_reduce, scream_attn_apply, scream_ln_fwd, scream_coor_head).  The layers
come from the model's own layer lists (_layer_prefixes).  PointTransformer's stem runs once over ALL packed rows (source and
target clouds share its weights, models/pointnet.py:50-52), so its weight gradients are single sums over both applications.
DEMTransformer's stem runs twice per layer (models/pointnet.py:143-145): stem_dsm.i on the source rows [0, rows_src) and
clouds [0, B), stem_dem.i on the target rows [rows_src, rows_total) and clouds [B, 2B); each side's weights get their
gradients from their own rows only (stem_dem's reach it through the cross layers' key/value path).  The backward runs the
chain in reverse: data gradients dX = dY W are scream_gemm_f32 on transposed weights (scream_transpose_f32), weight
gradients scream_gemm_wgrad_f32, LayerNorm scream_ln_bwd, the linear attention scream_attn_bwd.  Every reduction is a
fixed-order sum, so two identical calls give bitwise identical gradients.

Memory budget: per packed row and block application the forward keeps x (1 KB), Q'|K'|V (3 KB), the attention output (1 KB),
the merge output (1 KB), the LayerNorm1 output (1 KB), the FFN hidden layer (4 KB), the FFN output (1 KB) and the LayerNorm
statistics (16 B): about 12 KB.  A cross layer keeps 2 KB per TARGET row for K'|V instead of 2 KB of the source rows' Q'|K'|V.
A 5 k + 5 k point pair at 6 + 6 layers (stem on 10 k rows, cross stage on 5 k rows) keeps about 6 x 10 k x 12 KB +
12 x 5 k x 10 KB + 6 x 5 k x 2 KB = 1.4 GB until its backward has run.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, ops
from ._lib import SPLIT_BF3
from .ops import EPI_BIAS_RELU, EPI_ELU1, EPI_NONE, EPI_RELU, D_MODEL, _p, _workspace, call
from .packing import PackedBatch


def _ptr(t: torch.Tensor, col: int = 0) -> int:
    return _p(t) + col * 4  # bytes per float


def transpose(W: torch.Tensor) -> torch.Tensor:
    R, C_ = W.shape
    out = torch.empty(C_, R, device=W.device, dtype=torch.float32)
    call("scream_transpose_f32", W, R, C_, out)
    return out


SPLIT_K = 256  # a data gradient whose K scream_gemm_split_f32 does not take runs as products of this depth


def split_gemm_takes_k(K: int) -> bool:  # scream_gemm_split_f32's summed dimension: 64 + 192 j (K_64_PLUS_192, csrc/matrix_front.h)
    return K > 0 and K % 64 == 0 and (K // 32 - 2) % 3 == 0


class Gemms:
    """The matrix products of ONE training step in one arithmetic, a subclass each: fwd = epilogue(A W^T) and dgrad = dY W for
    W [N,K], and the weight gradient, whose body is this one: a subclass names its entry point, its sizer and `name`."""

    def wgrad(self, dY, X, dW, colsum=None, accumulate=False, ldy=None, ldx=None, rows=None) -> torch.Tensor:
        """dW[N,K] (+)= dY^T X over rows; dW any contiguous tensor of N * K floats."""
        return self._wgrad(dY, X, dW, colsum, accumulate, ldy, ldx, rows)

    def _wgrad(self, dY, X, dW, colsum, accumulate, ldy, ldx, rows, *extra) -> torch.Tensor:
        rows = dY.shape[0] if rows is None else rows
        N, K = dY.shape[1], X.shape[1]
        ws = _workspace(self.wgrad_sizer, rows, N, K, device=dY.device)
        call(self.wgrad_entry, dY.data_ptr(), dY.stride(0) if ldy is None else ldy, X.data_ptr(), X.stride(0) if ldx is None else ldx,
             rows, N, K, dW, accumulate, colsum, *extra, ws, ws.numel())
        return dW


class F32Gemms(Gemms):
    """Every product on the fp32-input MFMA; a data gradient is a GEMM against the transposed weight [K,N], which sums over N."""
    name, wgrad_entry, wgrad_sizer = "f32", "scream_gemm_wgrad_f32", "scream_wgrad_workspace_bytes"

    def fwd(self, A, W, epilogue: int = EPI_NONE, n_act: int = 0, bias=None):
        return ops.gemm_f32(A, W, epilogue, n_act=n_act, bias=bias)

    def dgrad(self, dY, W, out=None):
        return ops.gemm_f32(dY, transpose(W), out=out)


class SplitGemms(Gemms):
    """fp32-accurate products on the 16-bit matrix cores (SPLIT_BF3); each weight (and each transpose) is packed where it is used."""
    name, wgrad_entry, wgrad_sizer = "split", "scream_gemm_wgrad_split_f32", "scream_wgrad_split_workspace_bytes"

    def fwd(self, A, W, epilogue: int = EPI_NONE, n_act: int = 0, bias=None):
        return ops.gemm_split(A, ops.pack_w(W, SPLIT_BF3), epilogue, n_act=n_act, bias=bias)

    def dgrad(self, dY, W, out=None):
        Wt, N = transpose(W), W.shape[0]
        if split_gemm_takes_k(N):
            return ops.gemm_split(dY, ops.pack_w(Wt, SPLIT_BF3), out=out)
        if N % SPLIT_K:
            raise _lib.ScreamHipError("the split data gradient sums over N = %d: neither 64 + 192 j nor a multiple of %d" % (N, SPLIT_K))
        out = torch.empty(dY.shape[0], W.shape[1], device=dY.device, dtype=torch.float32) if out is None else out
        tmp = torch.empty_like(out)
        for c in range(0, N, SPLIT_K):  # column blocks of dY in order: a fixed-order sum
            ops.gemm_split(dY[:, c:c + SPLIT_K], ops.pack_w(Wt[:, c:c + SPLIT_K], SPLIT_BF3), out=tmp if c else out)
            if c:
                add_(out, tmp)
        return out

    def wgrad(self, dY, X, dW, colsum=None, accumulate=False, ldy=None, ldx=None, rows=None, split: int = SPLIT_BF3) -> torch.Tensor:
        return self._wgrad(dY, X, dW, colsum, accumulate, ldy, ldx, rows, split)


class Bf16Gemms(Gemms):
    """ONE bf16 product per GEMM, fp32 accumulation; W is read as it is (torch's [N,K]) by all three products."""
    name, wgrad_entry, wgrad_sizer = "bf16", "scream_gemm_wgrad_bf16_f32", "scream_wgrad_bf16_workspace_bytes"

    def fwd(self, A, W, epilogue: int = EPI_NONE, n_act: int = 0, bias=None):
        return ops.gemm_bf16(A, W, epilogue, n_act=n_act, bias=bias)

    def dgrad(self, dY, W, out=None):
        return ops.gemm_dgrad_bf16(dY, W, out=out)


ARITHMETICS = {c.name: c for c in (F32Gemms, SplitGemms, Bf16Gemms)}
wgrad, wgrad_split, wgrad_bf16 = F32Gemms().wgrad, SplitGemms().wgrad, Bf16Gemms().wgrad


def gemms(backend: str) -> Gemms:
    """The arithmetic of net.train_backend = backend; a name the models do not know raises their ValueError."""
    from .model import PointTransformer
    return ARITHMETICS[PointTransformer._check_train_backend(backend)]()


def ln_fwd(a: torch.Tensor, b, gamma, beta, out: torch.Tensor = None):
    rows = a.shape[0]
    y = torch.empty(rows, D_MODEL, device=a.device, dtype=torch.float32) if out is None else out
    mean = torch.empty(rows, device=a.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=a.device, dtype=torch.float32)
    call("scream_ln_fwd", a, b, gamma, beta, y, mean, rstd, rows)
    return y, mean, rstd


def ln_bwd(dy, a, b, mean, rstd, gamma, dz, dsum, dgamma, dbeta, accumulate: bool = False):
    rows = dy.shape[0]
    ws = _workspace("scream_ln_bwd_workspace_bytes", rows, device=dy.device)
    call("scream_ln_bwd", dy, a, b, mean, rstd, gamma, dz, dsum, dgamma, dbeta, accumulate, rows, ws, ws.numel())
    return dz


def attn_bwd(Qf, ldq, q_rows, q_row_base, O, dO, Kf, Vf, ldkv, kv_rows, kv_row_base, kv, batch: PackedBatch,
             q_cloud_begin, n_q, kv_cloud_offset, dq, lddq, dk, dv, lddkv):
    """Pointer-level wrapper of scream_attn_bwd: Qf / Kf / Vf / dq / dk / dv are device addresses (column offsets applied)."""
    ws = _workspace("scream_attn_bwd_workspace_bytes", n_q, batch.max_chunks, device=O.device)
    call("scream_attn_bwd", Qf, ldq, q_rows, q_row_base, O, dO, Kf, Vf, ldkv, kv_rows, kv_row_base, kv, batch.tile_cloud, batch.cloud_row0,
         batch.cloud_len, q_cloud_begin, n_q, kv_cloud_offset, batch.max_chunks, dq, lddq, dk, dv, lddkv, ws, ws.numel())


def relu_bwd(dy, y):
    call("scream_relu_bwd", dy, y, dy.numel())


def add_(y, x):
    call("scream_add_f32", y, x, y.numel())


def grad3(w, s, dW, transpose_w: bool, col_w=None, col_s=None, center=None, tile_cloud=None):
    rows = w.shape[0]
    ws = _workspace("scream_grad3_workspace_bytes", rows, device=w.device)
    call("scream_grad3", w, s, center, tile_cloud, rows, dW, transpose_w, col_w, col_s, 0, ws, ws.numel())


class _Layer:
    """What the backward of one block application needs."""
    __slots__ = ("cross", "prefix", "r0", "rows", "cb", "n", "x", "t", "qkv", "kvp", "kv", "att", "msg", "m1", "hid", "ffn",
                 "s1", "s2")


def _w(P: Dict[str, torch.nn.Parameter], name: str) -> torch.Tensor:
    return P[name].detach()


def _cat(*ws) -> torch.Tensor:
    return torch.cat([w for w in ws], dim=0).contiguous()


def _coor_w(P, k: int) -> torch.Tensor:  # coor_mlp.k's 1 x 1 convolution weight [out, in, 1] as the matrix [out, in]
    return _w(P, "coor_mlp.%d.weight" % k)[:, :, 0].contiguous()


def _block_fwd(P, mm: Gemms, prefix: str, x: torch.Tensor, t, batch: PackedBatch, r0: int, cb: int, n: int,
               out: torch.Tensor = None) -> (torch.Tensor, _Layer):
    """One block (models/transformer.py:74-90) on rows [r0, r0 + x.shape[0]) whose clouds are [cb, cb + n).  t: the target
    features (rows batch.rows_src ..) of a cross layer, None for a self layer.  out: where the block output goes (default:
    a new tensor)."""
    w = lambda s: _w(P, prefix + s)
    L = _Layer()
    L.cross, L.prefix, L.r0, L.rows, L.cb, L.n, L.x, L.t = t is not None, prefix, r0, x.shape[0], cb, n, x, t
    n_clouds = 2 * batch.n_pairs
    if t is None:
        L.qkv = mm.fwd(x, _cat(w("q_proj.weight"), w("k_proj.weight"), w("v_proj.weight")), EPI_ELU1,
                       n_act=2 * D_MODEL)
        L.kvp = None
        L.kv = ops.kv_reduce(L.qkv[:, D_MODEL:], L.qkv[:, 2 * D_MODEL:], 3 * D_MODEL, r0, batch.cloud_row0, batch.cloud_len, cb, n,
                             batch.max_chunks, n_clouds)
        L.att = ops.attn_apply(L.qkv, 3 * D_MODEL, L.kv, batch.tile_cloud[r0 // ops.ROW_TILE:], 0, batch.cloud_len, L.rows)
    else:
        B, rs = batch.n_pairs, batch.rows_src
        L.qkv = mm.fwd(x, w("q_proj.weight").contiguous(), EPI_ELU1, n_act=D_MODEL)
        L.kvp = mm.fwd(t, _cat(w("k_proj.weight"), w("v_proj.weight")), EPI_ELU1, n_act=D_MODEL)
        L.kv = ops.kv_reduce(L.kvp, L.kvp[:, D_MODEL:], 2 * D_MODEL, rs, batch.cloud_row0, batch.cloud_len, B, B, batch.max_chunks,
                             n_clouds)
        L.att = ops.attn_apply(L.qkv, D_MODEL, L.kv, batch.tile_cloud, B, batch.cloud_len, L.rows)
    L.msg = mm.fwd(L.att, w("merge.weight").contiguous())
    L.m1, *L.s1 = ln_fwd(L.msg, x, w("norm1.weight"), w("norm1.bias"))
    L.hid = mm.fwd(L.m1, w("mlp.0.weight").contiguous(), EPI_RELU)
    L.ffn = mm.fwd(L.hid, w("mlp.2.weight").contiguous())
    y, *L.s2 = ln_fwd(L.ffn, x, w("norm2.weight"), w("norm2.bias"), out)
    return y, L


def _block_bwd(P, G, mm: Gemms, L: _Layer, dy: torch.Tensor, batch: PackedBatch, dt) -> None:
    """dy [rows, 256] (the gradient of the block output) is REPLACED by the gradient of the block input; a cross layer adds
    the gradient of its key/value input into dt (the target features' gradient)."""
    w = lambda s: _w(P, L.prefix + s)
    g = lambda s: G[L.prefix + s]
    dev, R = dy.device, L.rows
    dffn = torch.empty(R, D_MODEL, device=dev, dtype=torch.float32)
    ln_bwd(dy, L.ffn, L.x, L.s2[0], L.s2[1], w("norm2.weight"), dffn, None, g("norm2.weight"), g("norm2.bias"))
    mm.wgrad(dffn, L.hid, g("mlp.2.weight"))
    dhid = mm.dgrad(dffn, w("mlp.2.weight"))
    relu_bwd(dhid, L.hid)
    mm.wgrad(dhid, L.m1, g("mlp.0.weight"))
    dm1 = mm.dgrad(dhid, w("mlp.0.weight"))
    del dhid
    dmsg = torch.empty(R, D_MODEL, device=dev, dtype=torch.float32)
    ln_bwd(dm1, L.msg, L.x, L.s1[0], L.s1[1], w("norm1.weight"), dmsg, dffn, g("norm1.weight"), g("norm1.bias"))  # dffn: dz2 + dz1
    del dm1
    mm.wgrad(dmsg, L.att, g("merge.weight"))
    datt = mm.dgrad(dmsg, w("merge.weight"))
    del dmsg
    if not L.cross:
        dqkv = torch.empty(R, 3 * D_MODEL, device=dev, dtype=torch.float32)
        attn_bwd(_ptr(L.qkv), 3 * D_MODEL, R, L.r0, L.att, datt, _ptr(L.qkv, D_MODEL), _ptr(L.qkv, 2 * D_MODEL), 3 * D_MODEL, R, L.r0,
                 L.kv, batch, L.cb, L.n, 0, _ptr(dqkv), 3 * D_MODEL, _ptr(dqkv, D_MODEL), _ptr(dqkv, 2 * D_MODEL), 3 * D_MODEL)
        dW = torch.empty(3 * D_MODEL, D_MODEL, device=dev, dtype=torch.float32)
        mm.wgrad(dqkv, L.x, dW)
        for i, nm in enumerate(("q_proj.weight", "k_proj.weight", "v_proj.weight")):
            G[L.prefix + nm] = dW[i * D_MODEL:(i + 1) * D_MODEL]
        mm.dgrad(dqkv, _cat(w("q_proj.weight"), w("k_proj.weight"), w("v_proj.weight")), out=dy)
    else:
        B, rs = batch.n_pairs, batch.rows_src
        Rt = L.t.shape[0]
        dq = torch.empty(R, D_MODEL, device=dev, dtype=torch.float32)
        dkvp = torch.empty(Rt, 2 * D_MODEL, device=dev, dtype=torch.float32)
        attn_bwd(_ptr(L.qkv), D_MODEL, R, 0, L.att, datt, _ptr(L.kvp), _ptr(L.kvp, D_MODEL), 2 * D_MODEL, Rt, rs, L.kv, batch, 0, B, B,
                 _ptr(dq), D_MODEL, _ptr(dkvp), _ptr(dkvp, D_MODEL), 2 * D_MODEL)
        mm.wgrad(dq, L.x, g("q_proj.weight"))
        dW = torch.empty(2 * D_MODEL, D_MODEL, device=dev, dtype=torch.float32)
        mm.wgrad(dkvp, L.t, dW)
        G[L.prefix + "k_proj.weight"], G[L.prefix + "v_proj.weight"] = dW[:D_MODEL], dW[D_MODEL:]
        mm.dgrad(dq, w("q_proj.weight"), out=dy)
        add_(dt, mm.dgrad(dkvp, _cat(w("k_proj.weight"), w("v_proj.weight"))))
    add_(dy, dffn)


def _layer_prefixes(net) -> Tuple[List[str], Optional[List[str]], List[str]]:
    """(stem, stem_tgt, cross): the state_dict prefixes of the model's layer lists (PointTransformer._layer_modules /
    _stem_tgt_modules).  stem_tgt is None when one stem serves both clouds (PointTransformer); for DEMTransformer stem holds
    stem_dsm.i (source side) and stem_tgt stem_dem.i (target side)."""
    names = {id(m): n + "." for n, m in net.named_modules()}
    mods, tgt = net._layer_modules(), net._stem_tgt_modules()
    ns = net.self_layer_num
    return ([names[id(m)] for m in mods[:ns]], None if tgt is None else [names[id(m)] for m in tgt],
            [names[id(m)] for m in mods[ns:]])


def _stem_passes(net, batch: PackedBatch) -> List[List[Tuple[str, int, int, int, int]]]:
    """Per stem layer, the block applications (prefix, first row, rows, first cloud, clouds) -- csrc/forward.hip's stem split."""
    stem, stem_tgt, _ = _layer_prefixes(net)
    rs, rt, B = batch.rows_src, batch.rows_total, batch.n_pairs
    if stem_tgt is None:  # pointnet.py:50-52: both clouds of every pair in one pass (shared weights)
        return [[(p, 0, rt, 0, 2 * B)] for p in stem]
    return [[(p, 0, rs, 0, B), (q, rs, rt - rs, B, B)] for p, q in zip(stem, stem_tgt)]  # pointnet.py:143-145


def forward_saving(net, batch: PackedBatch):
    """The training forward: packed src_pred [rows_src, 3] and what the backward needs."""
    from .model import pe_dim_t
    mm = gemms(net.train_backend)
    P = dict(net.named_parameters())
    dev = batch.xyz.device
    rs, rt, B = batch.rows_src, batch.rows_total, batch.n_pairs
    z0 = torch.empty(rt, D_MODEL, device=dev, dtype=torch.float32)
    emb_w = _w(P, "embedding.weight")[:, :, 0].contiguous()
    dim_t = pe_dim_t().to(dev)
    call("scream_pe_embed", batch.xyz, batch.tile_cloud, batch.center, dim_t, emb_w, _w(P, "embedding.bias"), z0, rt)
    f, *s0 = ln_fwd(z0, None, _w(P, "pre_norm.weight"), _w(P, "pre_norm.bias"))
    layers = []
    for passes in _stem_passes(net, batch):
        y = torch.empty(rt, D_MODEL, device=dev, dtype=torch.float32)  # every application writes its own rows
        for prefix, r0, rows, cb, n in passes:
            _, L = _block_fwd(P, mm, prefix, f[r0:r0 + rows], None, batch, r0, cb, n, out=y[r0:r0 + rows])
            layers.append(L)
        f = y
    n_stem = len(layers)
    tf = f[rs:]
    sf = f[:rs]
    for j, prefix in enumerate(_layer_prefixes(net)[2]):
        sf, L = _block_fwd(P, mm, prefix, sf, tf if j % 2 else None, batch, 0, 0, B)
        layers.append(L)
    h1 = mm.fwd(sf, _coor_w(P, 0), EPI_BIAS_RELU, bias=_w(P, "coor_mlp.0.bias"))
    h2 = mm.fwd(h1, _coor_w(P, 2), EPI_BIAS_RELU, bias=_w(P, "coor_mlp.2.bias"))
    out = ops.coor_head(h2, _coor_w(P, 4), _w(P, "coor_mlp.4.bias"))
    return out, dict(z0=z0, s0=s0, layers=layers, n_stem=n_stem, sf=sf, h1=h1, h2=h2, mm=mm)


def backward(net, batch: PackedBatch, saved, dout: torch.Tensor) -> List[torch.Tensor]:
    """Gradients of every parameter (named_parameters order) for the packed output gradient dout [rows_src, 3]."""
    P = dict(net.named_parameters())
    G = {n: torch.empty_like(p, dtype=torch.float32) for n, p in P.items()}
    mm = saved["mm"]  # the arithmetic of the forward this backward belongs to (it holds no weights: each is packed where used)
    dev = dout.device
    rs, rt = batch.rows_src, batch.rows_total
    dout = dout.to(torch.float32).contiguous()
    # coor_mlp (models/pointnet.py:27-33,60)
    h1, h2 = saved["h1"], saved["h2"]
    grad3(h2, dout, G["coor_mlp.4.weight"], False, col_s=G["coor_mlp.4.bias"])
    dh2 = torch.empty(rs, D_MODEL, device=dev, dtype=torch.float32)
    call("scream_coor_head_bwd", dout, _coor_w(P, 4), h2, dh2, rs)
    mm.wgrad(dh2, h1, G["coor_mlp.2.weight"], G["coor_mlp.2.bias"])
    dh1 = mm.dgrad(dh2, _coor_w(P, 2))
    relu_bwd(dh1, h1)
    mm.wgrad(dh1, saved["sf"], G["coor_mlp.0.weight"], G["coor_mlp.0.bias"])
    dF = torch.zeros(rt, D_MODEL, device=dev, dtype=torch.float32)  # gradient of the features of all rows
    mm.dgrad(dh1, _coor_w(P, 0), out=dF[:rs])
    del dh1, dh2
    layers, n_stem = saved["layers"], saved["n_stem"]
    for L in reversed(layers[n_stem:]):  # cross stage: source rows; the target features collect every cross layer's gradient
        _block_bwd(P, G, mm, L, dF[:rs], batch, dF[rs:])
    for L in reversed(layers[:n_stem]):  # stem: each application on its own rows (all rows for one shared stem)
        _block_bwd(P, G, mm, L, dF[L.r0:L.r0 + L.rows], batch, None)
    # pre_norm and the embedding (models/pointnet.py:45-48); the position embedding has no parameters
    dz0 = torch.empty(rt, D_MODEL, device=dev, dtype=torch.float32)
    z0, (m0, r0) = saved["z0"], saved["s0"]
    ln_bwd(dF, z0, None, m0, r0, _w(P, "pre_norm.weight"), dz0, None, G["pre_norm.weight"], G["pre_norm.bias"])
    grad3(dz0, batch.xyz, G["embedding.weight"], True, col_w=G["embedding.bias"], center=batch.center, tile_cloud=batch.tile_cloud)
    return [G[n].view(P[n].shape) for n in P]


class PointTransformerFn(torch.autograd.Function):
    """src_pred (packed [rows_src, 3]) = PointTransformer(batch) (DEMTransformer: dem_pred) with the HIP backward.  The
    parameters are inputs so that autograd routes their gradients into param.grad."""

    @staticmethod
    def forward(ctx, net, batch, *params):
        out, saved = forward_saving(net, batch)
        ctx.net, ctx.batch, ctx.saved = net, batch, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.saved is None:
            raise RuntimeError("the model's training graph was already freed by an earlier backward")
        grads = backward(ctx.net, ctx.batch, ctx.saved, dout)
        ctx.saved = None
        return (None, None) + tuple(grads)


def apply(net, batch: PackedBatch) -> torch.Tensor:
    params = [p for _, p in net.named_parameters()]
    for p in params:
        if not p.is_cuda or p.dtype != torch.float32:
            raise _lib.ScreamHipError("training needs fp32 parameters on the MI355X (net.to('cuda:0'))")
    return PointTransformerFn.apply(net, batch, *params)
