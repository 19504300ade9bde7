"""Thin host wrappers: torch device tensors in, one C-ABI call (include/scream_hip.h) each.

torch is plumbing here (device memory + the current HIP stream); all arithmetic happens in
libscream_hip.so.  There is no CPU fallback: a tensor that is not on a HIP device is an error.

Every call goes through call(name, *args), which marshals the arguments by the header's own declaration of the function
(_lib.PROTOTYPES): tensors are passed as they are and checked against the parameter's pointee type.  _p(t, dtype) remains for
the addresses call cannot check: a buffer whose dtype the header does not fix, a column offset, a struct field.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib, scales
from ._lib import SPLIT_BF3, SPLIT_H1, SPLIT_H2, check

EPI_NONE, EPI_ELU1, EPI_RELU, EPI_BIAS_RELU, EPI_RES_LN, EPI_QKV = 0, 1, 2, 3, 4, 5
ROW_TILE = 128
KV_CHUNK = 256
KV_ELEMS = 33 * 32
D_MODEL = 256


def _stream() -> int:
    """The current stream's handle (torch.cuda.current_stream().cuda_stream without building a Stream object for every call)."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _p(t: Optional[torch.Tensor], dtype=torch.float32) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.ScreamHipError("scream_amd ops need tensors on the MI355X (got device %s); there is no CPU path" % t.device)
    if t.dtype != dtype:
        raise TypeError("expected %s, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def _rows(t: torch.Tensor) -> int:
    """Address of a 2-D fp32 device matrix whose rows may be column slices of a wider one (unit column stride; the row
    stride goes to the library as ld*)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("matrix rows must be contiguous")
    return _p(t) if t.is_contiguous() else _p(t[:1]) if t.shape[0] else t.data_ptr()


# what a tensor must hold to be passed for a pointer the header declares with this pointee (void*: images and workspaces)
_DTYPES = {"float": torch.float32, "int32_t": torch.int32, "int64_t": torch.int64, "uint64_t": torch.int64, "uint8_t": torch.uint8,
           "double": torch.float64, "void": torch.uint8}
# name -> (per parameter: int / float for a scalar, the dtype behind a data pointer, the class behind a struct pointer;
#          ends in `void* stream`; returns a size) for every entry point that returns a status or a size
_PLANS = {name: (tuple((float if t in (C.c_float, C.c_double) else int) if pointee is None else _DTYPES.get(pointee, pointee)
                       for t, pointee in zip(p.argtypes, p.pointees)), p.stream, p.restype is C.c_int64)
          for name, p in _lib.PROTOTYPES.items() if p.stream or p.restype is C.c_int64}


def call(name: str, *args):
    """The one path into the library: scream_<name>(*args), every argument marshalled by the header's declaration of its
    parameter.  A scalar becomes int() or float().  For a pointer: a tensor must be on the GPU, contiguous and of the pointee's
    dtype (_DTYPES) and becomes its address; None is NULL; a Python int is an address the caller computed (a column offset,
    _rows, a buffer whose dtype the header cannot know: _p(t, dtype) checks those); a ctypes structure goes by reference.  The
    current stream is appended when the function ends in `void* stream` and the caller left it out.  A status other than 0 and
    a negative size raise ScreamHipError naming the function; the value is returned."""
    try:
        kinds, has_stream, sizer = _PLANS[name]
    except KeyError:
        raise TypeError("%s is not an entry point that returns a status or a size" % name) from None
    if has_stream and len(args) == len(kinds) - 1:
        args += (_stream(),)
    elif len(args) != len(kinds):
        raise TypeError("%s takes %d arguments (%s), got %d" % (name, len(kinds), ", ".join(_lib.PROTOTYPES[name].params), len(args)))
    conv = []
    for kind, a in zip(kinds, args):
        if kind is int or kind is float:
            a = kind(a)
        elif isinstance(a, torch.Tensor):
            if a.dtype != kind or not a.is_cuda or not a.is_contiguous():
                _refuse(name, len(conv), a, kind)
            a = a.data_ptr()
        elif type(a) is kind:
            a = C.byref(a)
        elif a is not None and not isinstance(a, int):
            _refuse(name, len(conv), a, kind)
        conv.append(a)
    rc = getattr(_lib.load(), name)(*conv)
    if not sizer:
        if rc:
            check(rc, name)
    elif rc < 0:
        raise _lib.ScreamHipError("%s(%s): invalid argument" % (name, ", ".join(str(a) for a in args)))
    return rc


def _refuse(name: str, index: int, a, kind):
    """Raise for argument `index` of call(name, ...): _p's exception for a tensor, with the function and the parameter."""
    where = "%s(%s): " % (name, _lib.PROTOTYPES[name].params[index])
    if not isinstance(a, torch.Tensor):
        raise TypeError(where + "expected %s, got %r" % (kind, a))
    try:
        _p(a, kind)
    except (_lib.ScreamHipError, TypeError, ValueError) as e:
        raise type(e)(where + str(e)) from None


def _workspace(name: str, *args, device, floor: int = 16) -> torch.Tensor:
    """Scratch for one call: the uint8 tensor of the size that the library's own `*_workspace_bytes(*args)` asks for (at least
    `floor` bytes, so that it always has an address); a negative size is the library refusing the arguments."""
    return torch.empty(max(call(name, *args), floor), device=device, dtype=torch.uint8)


def gemm_f32(A: torch.Tensor, W: torch.Tensor, epilogue: int = EPI_NONE, n_act: int = 0, bias: Optional[torch.Tensor] = None,
             residual: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = epilogue(A @ W.T); A [M,K] (M % 128 == 0), W [N,K] (N % 256 == 0, K % 32 == 0); A and out may be column slices (_rows)."""
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    call("scream_gemm_f32", _rows(A), A.stride(0), W, _rows(out), out.stride(0), M, N, K, epilogue, n_act, bias,
         residual, residual.stride(0) if residual is not None else 0, gamma, beta)
    return out


def gemm_bf16(A: torch.Tensor, W: torch.Tensor, epilogue: int = EPI_NONE, n_act: int = 0,
              bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = epilogue(bf16(A) @ bf16(W).T), fp32 accumulation (train_backend "bf16"); shapes as gemm_f32, W torch's [N,K] fp32."""
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and W.is_contiguous()
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    call("scream_gemm_bf16_f32", _rows(A), A.stride(0), W, _rows(out), out.stride(0), M, N, K, epilogue, n_act, bias)
    return out


def gemm_dgrad_bf16(dY: torch.Tensor, W: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX = bf16(dY) @ bf16(W) for W [N,K] (torch's layout, read as it is), summed over N in one launch."""
    M, N = dY.shape
    K = W.shape[1]
    assert W.shape[0] == N and W.is_contiguous()
    if out is None:
        out = torch.empty(M, K, device=dY.device, dtype=torch.float32)
    call("scream_gemm_dgrad_bf16_f32", _rows(dY), dY.stride(0), W, _rows(out), out.stride(0), M, N, K)
    return out


@dataclass
class PackedW:
    """A weight matrix [N,K] in the split GEMM's operand image (scream_pack_w_split): `split` planes of 16-bit values,
    [split, K/32, N, 32]; SPLIT_H2: of W * 2^w_exp."""
    data: torch.Tensor
    split: int
    w_exp: int
    N: int
    K: int
    row_l1: Optional[torch.Tensor] = None  # [N] sum_k |W[n, k]| on the host: bounds |A W^T| by max|A| * row_l1 (gemm_qkv's K^T V exponents)

    def data_ptr(self) -> int:
        return self.data.data_ptr()


@dataclass
class PackedTail:
    """merge + mlp.0 + mlp.2 in the layer-tail kernel's 72-stage image (scream_pack_tail) with the exponents it was built for."""
    data: torch.Tensor
    split: int
    exps: _lib.TailExpsT
    next_q: bool = False  # eight more stages: the next layer's query projection (pack_tail(Wq_next=...))

    def data_ptr(self) -> int:
        return self.data.data_ptr()


def default_split() -> int:
    """The operand split behind gemm_backend: 'h2' (default) -> SPLIT_H2, 'x3' -> SPLIT_BF3."""
    return SPLIT_BF3 if os.environ.get("SCREAM_GEMM", "h2") == "x3" else SPLIT_H2


def pack_w(W: torch.Tensor, split: Optional[int] = None, w_exp: Optional[int] = None) -> PackedW:
    """[N,K] fp32 (on the GPU) -> the packed operand of the split GEMMs (scream_pack_w_split).  SPLIT_BF3: planes
    p0 + p1 + p2 == W exactly.  SPLIT_H2: two fp16 planes of W * 2^w_exp (default: the largest exponent max|W| allows)."""
    split = default_split() if split is None else split
    W = W.detach().to(torch.float32).contiguous()
    N, K = W.shape
    if split in (SPLIT_H2, SPLIT_H1) and w_exp is None:
        w_exp = scales.w_exp(W)
    w_exp = int(w_exp or 0)
    dt = torch.float16 if split in (SPLIT_H2, SPLIT_H1) else torch.bfloat16
    out = torch.empty(split, K // 32, N, 32, device=W.device, dtype=dt)
    call("scream_pack_w_split", W, N, K, split, w_exp, _p(out, dt))
    return PackedW(out, split, w_exp, N, K, W.abs().sum(dim=1).cpu() if split != SPLIT_BF3 else None)


LAYOUT_A_FRAG, LAYOUT_C_FRAG = 1, 2


def act_layout(X: torch.Tensor, to_fragment: bool) -> torch.Tensor:
    """[M,256] fp32 row-major <-> fragment-major (SCREAM_ACT_FRAG, include/scream_hip.h); returns a new tensor."""
    M = X.shape[0]
    assert X.shape[1] == D_MODEL
    out = torch.empty_like(X)
    call("scream_act_layout", X, out, M, to_fragment)
    return out


def _a_exp(A: torch.Tensor, Wp, a_exp: Optional[int]) -> int:
    """SPLIT_H2 needs |A| 2^a_exp <= 2^15.  Callers that know a bound pass it; the convenience default measures max|A|
    (a device synchronisation: tests and tools only -- the forward gets its exponents from the weights, scream_amd/scales.py)."""
    if Wp.split == SPLIT_BF3:
        return 0
    return scales.exp_for(A.abs().max().item()) if a_exp is None else int(a_exp)


def gemm_split(A: torch.Tensor, Wp: PackedW, epilogue: int = EPI_NONE, n_act: int = 0, bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, layout: int = 0, a_exp: Optional[int] = None) -> torch.Tensor:
    """gemm_f32's contract on the 16-bit matrix cores by operand splitting (fp32-level accuracy); Wp = pack_w(W).
    layout: LAYOUT_A_FRAG (A is fragment-major) | LAYOUT_C_FRAG (the activated query tile is written fragment-major)."""
    M, K = A.shape
    assert K == Wp.K
    if out is None:
        out = torch.empty(M, Wp.N, device=A.device, dtype=torch.float32)
    call("scream_gemm_split_f32", _rows(A), A.stride(0), Wp.data_ptr(), _rows(out), out.stride(0), M, Wp.N, K, epilogue, n_act,
         bias, residual, residual.stride(0) if residual is not None else 0, gamma, beta, layout, Wp.split, _a_exp(A, Wp, a_exp),
         Wp.w_exp)
    return out


def tail_exps(**kw) -> _lib.TailExpsT:
    e = _lib.TailExpsT()
    for k in ("e_att", "e_wm", "e_m1", "e_w1", "e_h", "e_w2", "e_y", "e_wq", "e_q"):
        setattr(e, k, int(kw.get(k, 0)))
    return e


def pack_tail(Wm: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor, split: Optional[int] = None,
              exps: Optional[_lib.TailExpsT] = None, Wq_next: Optional[torch.Tensor] = None) -> PackedTail:
    """merge.weight [256,256], mlp.0.weight [1024,256], mlp.2.weight [256,1024] -> the weight image of layer_tail.
    SPLIT_H2 needs `exps` (scales.layer_exps / ops.tail_exps): the image carries e_wm, e_w1, e_w2, the kernel the rest.
    Wq_next (fp16 splits): q_proj.weight of the NEXT layer -- layer_tail(..., q_next=...) then also produces that layer's Q'
    (exps.e_y: exponent of this block's output as an operand, exps.e_wq: of Wq_next)."""
    split = default_split() if split is None else split
    Wm, W1, W2 = (w.detach().to(torch.float32).contiguous() for w in (Wm, W1, W2))
    assert Wm.shape == (D_MODEL, D_MODEL) and W1.shape == (4 * D_MODEL, D_MODEL) and W2.shape == (D_MODEL, 4 * D_MODEL)
    if split != SPLIT_BF3 and exps is None:
        raise ValueError("pack_tail on an fp16 split needs the operand exponents (scream_amd/scales.py)")
    exps = exps if exps is not None else tail_exps()
    if Wq_next is not None:
        Wq_next = Wq_next.detach().to(torch.float32).contiguous()
        assert Wq_next.shape == (D_MODEL, D_MODEL)
    # (a negative size: a next-layer query projection needs an fp16 split)
    out = torch.empty(call("scream_tail_image_bytes", split, Wq_next is not None), device=Wm.device, dtype=torch.uint8)
    call("scream_pack_tail", Wm, W1, W2, Wq_next, split, exps, out)
    return PackedTail(out, split, exps, Wq_next is not None)


def kv_finalize_image(partial: torch.Tensor, cloud_row0, cloud_len, row_base: int, cloud_begin: int, n_kv: int,
                   n_clouds: int, out: Optional[torch.Tensor] = None, split: Optional[int] = None) -> torch.Tensor:
    """K^T V partials of gemm_qkv -> the per-cloud operand image of layer_tail ([n_clouds, kv_image_bytes] uint8) for the tail of
    the same `split` (default: default_split()): three bf16 planes, or two fp16 planes with a per-head exponent chosen on the device.
    partial [L, M/128, 8, 1056] (a batched key/value projection of L layers): returns [L, n_clouds, kv_image_bytes]."""
    split = default_split() if split is None else split
    L = partial.shape[0] if partial.dim() == 4 else 1
    img = call("scream_kv_image_bytes")
    if out is None:
        out = torch.zeros((L, n_clouds, img) if partial.dim() == 4 else (n_clouds, img), device=partial.device, dtype=torch.uint8)
    call("scream_kv_finalize_image", partial, cloud_row0, cloud_len, row_base, cloud_begin, n_kv, out, L,
         partial[0].numel() if L > 1 else 0, n_clouds * img if L > 1 else 0, split)
    return out


def layer_tail(Q: torch.Tensor, kv_image: torch.Tensor, tile_cloud, kv_cloud_offset: int, cloud_len, x: torch.Tensor,
               tail: PackedTail, g1, b1, g2, b2, out: Optional[torch.Tensor] = None,
               q_next: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention apply + merge + norm1 + FFN + norm2 of one block in one launch (scream_layer_tail_f32).
    Q, x and the result are FRAGMENT-major [M,256] matrices (act_layout converts).  q_next (images packed with Wq_next): also
    receives elu(y Wq_next^T) + 1, fragment-major; it may be Q itself."""
    M = x.shape[0]
    assert x.shape[1] == D_MODEL and (Q is None or x.shape == Q.shape)  # (Q is required: the library refuses NULL with SCREAM_EINVAL)
    assert (q_next is not None) == tail.next_q, "q_next goes with an image that carries the next layer's query stages"
    if out is None:
        out = torch.empty(M, D_MODEL, device=x.device, dtype=torch.float32)
    call("scream_layer_tail_f32", Q, kv_image, tile_cloud, kv_cloud_offset, cloud_len, x, tail.data_ptr(), g1, b1, g2, b2, out,
         q_next, M, tail.split, tail.exps)
    return out


def _qkv_outputs(x: torch.Tensor, N: int, n_q: int):
    """(Q' or None, kv_partial) for N = n_q + 512 L columns; L > 1 key/value tile pairs (several layers, n_q == 0): [L,M/128,8,1056]."""
    M, L = x.shape[0], (N - n_q) // 512
    Q = torch.empty(M, n_q, device=x.device, dtype=torch.float32) if n_q else None
    part = torch.empty((L, M // ROW_TILE, 8, KV_ELEMS) if L > 1 else (M // ROW_TILE, 8, KV_ELEMS), device=x.device, dtype=torch.float32)
    return Q, part


def _qkv_exps(x: torch.Tensor, row_l1: torch.Tensor, n_q: int, a_exp, k_exp, v_exp):
    """Exponents left at None are measured (a device sync: tests and tools only, as for _a_exp): |k|, |v| <= max|x| * (L1 norm of
    their weight rows); key rows are the first 128 of every 256 behind the queries (include/scream_hip.h)."""
    if a_exp is None or k_exp is None or v_exp is None:
        amax = float(x.abs().max().item())
        rl = row_l1[n_q:].view(-1, 2, 128)
        a_exp = scales.exp_for(amax) if a_exp is None else a_exp
        k_exp = scales.exp_for(1.0 + amax * float(rl[:, 0].max())) if k_exp is None else k_exp
        v_exp = scales.exp_for(amax * float(rl[:, 1].max())) if v_exp is None else v_exp
    return int(a_exp), int(k_exp), int(v_exp)


def gemm_qkv(A: torch.Tensor, W, n_q: int, tile_cloud, cloud_row0, cloud_len, row_base: int, layout: int = 0,
             a_exp: Optional[int] = None, k_exp: Optional[int] = None, v_exp: Optional[int] = None):
    """Fused q/k/v projection (scream_gemm_qkv_f32 / scream_gemm_qkv_split_f32 for W = pack_w(...)).  Returns
    (Q' [M,256] or None, kv_partial [M/128,8,1056]).  layout (split kernel only): LAYOUT_A_FRAG | LAYOUT_C_FRAG."""
    M, K = A.shape
    sp = isinstance(W, PackedW)  # packed operand planes -> the split kernel
    N = W.N if sp else W.shape[0]
    Q, part = _qkv_outputs(A, N, n_q)
    args = (A, A.stride(0), W.data_ptr() if sp else W, Q, n_q, M, N, K, n_q, tile_cloud, cloud_row0, cloud_len, row_base, part)
    if sp:
        # (bf16 x 3 is scale free: no exponent is read)
        a_exp, k_exp, v_exp = (0, 0, 0) if W.split == SPLIT_BF3 else _qkv_exps(A, W.row_l1, n_q, a_exp, k_exp, v_exp)
        call("scream_gemm_qkv_split_f32", *args, layout, W.split, a_exp, W.w_exp, k_exp, v_exp)
    else:
        assert layout == 0
        call("scream_gemm_qkv_f32", *args)
    return Q, part


@dataclass
class PackedProj:
    """A q/k/v (n_q = 256, N = 768) or stacked key/value (n_q = 0, N = 512 L) weight matrix in the ring projection kernel's stage
    image (scream_pack_proj): fp16 planes of W * 2^w_exp, one 32-column chunk over K = 256 per stage."""
    data: torch.Tensor
    split: int
    w_exp: int
    N: int
    n_q: int
    row_l1: Optional[torch.Tensor] = None

    def data_ptr(self) -> int:
        return self.data.data_ptr()


def pack_proj(W: torch.Tensor, n_q: int, split: Optional[int] = None, w_exp: Optional[int] = None) -> PackedProj:
    """[N,256] fp32 in the row order of gemm_qkv -> the stage image of proj_qkv (fp16 splits only)."""
    split = SPLIT_H2 if split is None else split
    W = W.detach().to(torch.float32).contiguous()
    N, K = W.shape
    assert K == D_MODEL
    w_exp = scales.w_exp(W) if w_exp is None else int(w_exp)
    out = torch.empty(call("scream_proj_image_bytes", N, split), device=W.device, dtype=torch.uint8)
    call("scream_pack_proj", W, N, n_q, split, w_exp, out)
    return PackedProj(out, split, w_exp, N, n_q, W.abs().sum(dim=1).cpu())


def proj_qkv(x_frag: torch.Tensor, P: PackedProj, tile_cloud, cloud_row0, cloud_len, row_base: int,
             a_exp: Optional[int] = None, k_exp: Optional[int] = None, v_exp: Optional[int] = None):
    """The fused q/k/v projection on the ring kernel (scream_proj_qkv_f32): x and Q' fragment-major.  Returns (Q' or None,
    kv_partial) like gemm_qkv."""
    M = x_frag.shape[0]
    Q, part = _qkv_outputs(x_frag, P.N, P.n_q)  # (n_q is 0 or the model width)
    a_exp, k_exp, v_exp = _qkv_exps(x_frag, P.row_l1, P.n_q, a_exp, k_exp, v_exp)
    call("scream_proj_qkv_f32", x_frag, P.data_ptr(), Q, M, P.N, P.n_q, tile_cloud, cloud_row0, cloud_len, row_base, part, P.split,
         a_exp, P.w_exp, k_exp, v_exp)
    return Q, part


def kv_finalize(part, cloud_row0, cloud_len, row_base: int, cloud_begin: int, n_kv: int, n_clouds: int) -> torch.Tensor:
    kv = torch.zeros(n_clouds, 8, KV_ELEMS, device=part.device, dtype=torch.float32)
    call("scream_kv_finalize", part, cloud_row0, cloud_len, row_base, cloud_begin, n_kv, kv)
    return kv


def pe_embed_ln(xyz, tile_cloud, center, dim_t, emb_w, emb_b, gamma, beta, frag: bool = False) -> torch.Tensor:
    """A1.  frag=True: the same values in the fragment-major layout (include/scream_hip.h SCREAM_ACT_FRAG; act_layout undoes it)."""
    rows = xyz.shape[0]
    feats = torch.empty(rows, D_MODEL, device=xyz.device, dtype=torch.float32)
    call("scream_pe_embed_ln_frag" if frag else "scream_pe_embed_ln", xyz, tile_cloud, center, dim_t, emb_w, emb_b, gamma, beta, feats,
         rows)
    return feats


def kv_reduce(Kf: torch.Tensor, Vf: torch.Tensor, ld: int, row_base: int, cloud_row0, cloud_len, cloud_begin: int,
              n_kv: int, max_chunks: int, n_clouds: int) -> torch.Tensor:
    """Kf / Vf: views whose data_ptr is column 0 of the keys / values (row stride ld floats)."""
    dev = Kf.device
    partial = torch.empty(max(n_kv * max_chunks * 8 * KV_ELEMS, 1), device=dev, dtype=torch.float32)
    kv = torch.zeros(n_clouds, 8, KV_ELEMS, device=dev, dtype=torch.float32)
    for t in (Kf, Vf):
        if not t.is_cuda or t.dtype != torch.float32:
            raise TypeError("kv_reduce needs fp32 device tensors")
    call("scream_kv_reduce", Kf.data_ptr(), Vf.data_ptr(), ld, row_base, cloud_row0, cloud_len, cloud_begin, n_kv, max_chunks, partial, kv)
    return kv


def attn_apply(Qf: torch.Tensor, ldq: int, kv, tile_cloud, kv_cloud_offset: int, cloud_len, rows: int) -> torch.Tensor:
    out = torch.empty(rows, D_MODEL, device=kv.device, dtype=torch.float32)
    call("scream_attn_apply", Qf.data_ptr(), ldq, kv, tile_cloud, kv_cloud_offset, cloud_len, out, D_MODEL, rows)
    return out


def coor_head(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    rows = X.shape[0]
    out = torch.empty(rows, 3, device=X.device, dtype=torch.float32)
    call("scream_coor_head", X, W, b, out, rows)
    return out


def nn_search(query: torch.Tensor, ref: torch.Tensor, q_row0, q_len, r_row0, r_len, s: torch.Tensor,
              max_q_len: int, max_r_len: int, thresh: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Packed thresholded 1-NN.  Returns (idx int32, dmin fp32, valid uint8), one entry per packed query row."""
    dev = query.device
    qn, rn = query.shape[0], ref.shape[0]
    n_pairs = s.shape[0]
    ref_prep = torch.empty(max(rn, 1), 4, device=dev, dtype=torch.float32)
    keys = torch.empty(max(qn, 1), device=dev, dtype=torch.int64)
    idx = torch.empty(qn, device=dev, dtype=torch.int32)
    dmin = torch.empty(qn, device=dev, dtype=torch.float32)
    valid = torch.empty(qn, device=dev, dtype=torch.uint8)
    call("scream_nn_search", query, ref, q_row0, q_len, r_row0, r_len, s, n_pairs, max_q_len, max_r_len, qn, rn, thresh, ref_prep,
         keys, idx, dmin, valid)
    return idx, dmin, valid


def render_workspace(n_pairs: int, n_views: int, w: int, src_rows_total: int, device) -> torch.Tensor:
    """Scratch of render_depth; render_depth_bwd needs the forward's, untouched (it begins with the depth ranges)."""
    return _workspace("scream_render_workspace_bytes", n_pairs, n_views, w, src_rows_total, device=device)


def render_depth(src: torch.Tensor, s_row0, s_len, tgt: torch.Tensor, t_row0, t_len, max_s_len: int, max_t_len: int,
                 rot: torch.Tensor, w: int, rho: float, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed depth renderer (scream_render_depth): src / tgt packed [rows,3], per-pair row0 / len int32 device arrays, rot
    [V,3,3] fp32 on the device.  Returns (imgs [B,V,2,w,w] fp32, argmax [B,V,2,w,w] int32)."""
    n_pairs, V = s_row0.shape[0], rot.shape[0]
    dev = src.device
    if workspace is None:
        workspace = render_workspace(n_pairs, V, w, src.shape[0], dev)
    imgs = torch.empty(n_pairs, V, 2, w, w, device=dev, dtype=torch.float32)
    argmax = torch.empty(n_pairs, V, 2, w, w, device=dev, dtype=torch.int32)
    call("scream_render_depth", src, s_row0, s_len, tgt, t_row0, t_len, n_pairs, max_s_len, max_t_len, src.shape[0], rot.reshape(V, 9),
         V, w, rho, imgs, argmax, workspace, workspace.numel())
    return imgs, argmax


def render_depth_bwd(dimgs: torch.Tensor, argmax: torch.Tensor, src: torch.Tensor, s_row0, s_len, max_s_len: int,
                     rot: torch.Tensor, w: int, rho: float, workspace: torch.Tensor) -> torch.Tensor:
    """Gradient of the source images with respect to the packed source rows (scream_render_depth_bwd); argmax and workspace are
    those of the render_depth call.  Returns dsrc [rows,3] (zero on rows outside every source cloud)."""
    n_pairs, V = s_row0.shape[0], rot.shape[0]
    dsrc = torch.zeros(src.shape[0], 3, device=src.device, dtype=torch.float32)
    call("scream_render_depth_bwd", src, s_row0, s_len, n_pairs, max_s_len, src.shape[0], rot.reshape(V, 9), V, w, rho, dimgs, argmax,
         workspace, workspace.numel(), dsrc)
    return dsrc


def voxel_down_sample_packed(xyz: torch.Tensor, row0: torch.Tensor, length: torch.Tensor, max_len: int, voxel: torch.Tensor,
                             want_counts: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """scream_voxel_down_sample on packed rows: xyz [rows,3] fp32, row0 / length int32 [B] and voxel float64 [B] on the device.
    Returns (out_xyz [rows,3], out_len int32 [B], out_count int32 [rows] or None), all on the device: cloud c's voxels are rows
    row0[c] .. + out_len[c] of out_xyz (the rows behind are not written), out_len[c] = -1 for a refused cloud.  No host sync."""
    n_clouds, rows, dev = row0.shape[0], xyz.shape[0], xyz.device
    workspace = _workspace("scream_voxel_workspace_bytes", rows, n_clouds, device=dev)
    out_xyz = torch.empty(max(rows, 1), 3, device=dev, dtype=torch.float32)
    out_len = torch.empty(max(n_clouds, 1), device=dev, dtype=torch.int32)
    out_count = torch.empty(max(rows, 1), device=dev, dtype=torch.int32) if want_counts else None
    # (an all-empty batch still reports its lengths)
    call("scream_voxel_down_sample", xyz if rows else out_xyz, row0, length, n_clouds, max_len, voxel, out_xyz, out_len, out_count,
         workspace, workspace.numel())
    return out_xyz[:rows], out_len[:n_clouds], (out_count[:rows] if want_counts else None)


def dsm_extract_packed(patch: torch.Tensor, p_row0: torch.Tensor, p_len: torch.Tensor, max_p_len: int, dem: torch.Tensor,
                       d_row0: torch.Tensor, d_len: torch.Tensor, max_d_len: int, radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """scream_dsm_extract on packed rows: patch [P,3] / dem [D,3] fp32, the four int32 [B] arrays on the device.  Returns
    (out_xyz [D,3], out_idx int32 [D]) on the device; rows of dem outside every cloud are not written.  No host sync."""
    n_clouds, P, D, dev = p_row0.shape[0], patch.shape[0], dem.shape[0], dem.device
    workspace = _workspace("scream_dsm_workspace_bytes", P, n_clouds, max_p_len, device=dev)
    out_xyz = torch.empty(max(D, 1), 3, device=dev, dtype=torch.float32)
    out_idx = torch.empty(max(D, 1), device=dev, dtype=torch.int32)
    patch_p = patch if P else workspace.data_ptr()  # a batch of empty windows: nothing is read through it
    call("scream_dsm_extract", patch_p, p_row0, p_len, max_p_len, P, dem if D else out_xyz, d_row0, d_len, max_d_len, D, n_clouds,
         radius, out_xyz, out_idx, workspace, workspace.numel())
    return out_xyz[:D], out_idx[:D]


def dsm_dem_assemble_packed(dsm: torch.Tensor, dem: torch.Tensor, row0: torch.Tensor, length: torch.Tensor,
                            max_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """scream_dsm_dem_assemble: dsm / dem [rows,3] fp32 at the same rows -> (out [rows,6], centre [B,3]), on the device."""
    n_clouds, rows, dev = row0.shape[0], dem.shape[0], dem.device
    out = torch.empty(max(rows, 1), 6, device=dev, dtype=torch.float32)
    centre = torch.empty(max(n_clouds, 1), 3, device=dev, dtype=torch.float32)
    call("scream_dsm_dem_assemble", dsm if rows else out, dem if rows else out, row0, length, n_clouds, max_len, rows, out, centre)
    return out[:rows], centre[:n_clouds]


def _radius_args(src, s_row0, s_len, max_s_len, tgt, t_row0, t_len, max_t_len, T, radius, dummy):
    """The seventeen leading arguments scream_radius_count and scream_radius_pairs share (an empty side: nothing is read through
    `dummy`)."""
    n_pairs, S, N = s_row0.shape[0], src.shape[0], tgt.shape[0]
    if T.shape[0] != n_pairs or T.numel() != n_pairs * 16:
        raise _lib.ScreamHipError("expected %d 4x4 transforms, got %s" % (n_pairs, tuple(T.shape)))
    return (src if S else dummy, s_row0, s_len, max_s_len, S, tgt if N else dummy, t_row0, t_len, max_t_len, N, T, n_pairs, radius)


def radius_count_packed(src: torch.Tensor, s_row0: torch.Tensor, s_len: torch.Tensor, max_s_len: int, tgt: torch.Tensor,
                        t_row0: torch.Tensor, t_len: torch.Tensor, max_t_len: int, T: torch.Tensor,
                        radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """scream_radius_count on packed rows: src [S,3] / tgt [N,3] fp32, the four int32 [B] arrays and T float64 [B,4,4] on the
    device.  Returns (count int32 [S], workspace): count[row] = the number of target rows of the row's pair with d2 < radius^2
    (0 for rows outside every pair); the workspace holds the targets' cell lists for radius_pairs_packed.  No host sync."""
    n_pairs, S, N, dev = s_row0.shape[0], src.shape[0], tgt.shape[0], src.device
    workspace = _workspace("scream_radius_workspace_bytes", N, n_pairs, max_t_len, device=dev)
    count = torch.zeros(max(S, 1), device=dev, dtype=torch.int32)
    args = _radius_args(src, s_row0, s_len, max_s_len, tgt, t_row0, t_len, max_t_len, T, radius, count.data_ptr())
    call("scream_radius_count", *args, count, workspace, workspace.numel())
    return count[:S], workspace


def radius_pairs_packed(src: torch.Tensor, s_row0: torch.Tensor, s_len: torch.Tensor, max_s_len: int, tgt: torch.Tensor,
                        t_row0: torch.Tensor, t_len: torch.Tensor, max_t_len: int, T: torch.Tensor, radius: float,
                        workspace: torch.Tensor, K: int, offset: torch.Tensor, total: int) -> torch.Tensor:
    """scream_radius_pairs: the same inputs and the workspace of the radius_count_packed call that filled it; offset int64
    [S + 1] on the device (the exclusive prefix sum of min(count, K), K <= 0: no limit) and its last element `total` as a host
    int.  Returns pair_j int32 [total]: per source row its neighbours' target rows (relative to the pair's first) in ascending
    (d2, j).  No host sync."""
    S, dev = src.shape[0], src.device
    if offset.shape[0] != S + 1:
        raise _lib.ScreamHipError("offset: expected %d elements, got %d" % (S + 1, offset.shape[0]))
    pair_j = torch.empty(max(int(total), 1), device=dev, dtype=torch.int32)
    args = _radius_args(src, s_row0, s_len, max_s_len, tgt, t_row0, t_len, max_t_len, T, radius, pair_j.data_ptr())
    call("scream_radius_pairs", *args, workspace, workspace.numel(), K, offset, pair_j)
    return pair_j[:int(total)]


def prep_pairs_packed(raw: torch.Tensor, raw_row0: torch.Tensor, raw_len: torch.Tensor, max_len: int, T: torch.Tensor,
                      perturb: torch.Tensor, side: torch.Tensor, noise_std: float, seed: int, sample_id: torch.Tensor, mode: int,
                      center_rule: int, cloud_row0: torch.Tensor, rows_total: int):
    """scream_prep_pairs: raw [rows,3] fp32 or float64 (every cloud back to back), raw_row0 / raw_len / cloud_row0 int32 [2B]
    (sources, then targets), T / perturb float64 [B,4,4], side int32 [B], sample_id int64 [B], all on the device.  Returns
    (xyz fp32 [rows_total,3], center fp32 [2B,3], rot fp32 [B,3,3], trans fp32 [B,3,1], s float64 [B], c float64 [B,3],
    T_aug float64 [B,4,4]).  No host sync."""
    B, rows, dev = side.shape[0], raw.shape[0], raw.device
    if raw.dtype not in (torch.float32, torch.float64):
        raise TypeError("expected torch.float32 or torch.float64 clouds, got %s" % raw.dtype)
    if B < 1 or raw_row0.shape[0] != 2 * B or raw_len.shape[0] != 2 * B or cloud_row0.shape[0] != 2 * B or T.numel() != 16 * B or \
            perturb.numel() != 16 * B or sample_id.shape[0] != B:
        raise _lib.ScreamHipError("prep_pairs_packed: the per-pair arrays do not describe %d pairs" % B)
    workspace = _workspace("scream_prep_pairs_workspace_bytes", rows, B, max_len, device=dev)
    xyz = torch.empty(int(rows_total), 3, device=dev, dtype=torch.float32)
    center = torch.empty(2 * B, 3, device=dev, dtype=torch.float32)
    rot = torch.empty(B, 3, 3, device=dev, dtype=torch.float32)
    trans = torch.empty(B, 3, 1, device=dev, dtype=torch.float32)
    s = torch.empty(B, device=dev, dtype=torch.float64)
    c = torch.empty(B, 3, device=dev, dtype=torch.float64)
    T_aug = torch.empty(B, 4, 4, device=dev, dtype=torch.float64)
    call("scream_prep_pairs", _p(raw, raw.dtype), raw.dtype == torch.float64, rows, raw_row0, raw_len, max_len, T, perturb, side,
         noise_std, int(seed) & (2 ** 64 - 1), sample_id, mode, center_rule, cloud_row0, B, rows_total, xyz, center, rot, trans, s, c,
         T_aug, workspace, workspace.numel())
    return xyz, center, rot, trans, s, c, T_aug


def _l1_args(pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len):
    rows_src = pred.shape[0]
    if pred.dim() != 2 or pred.shape[1] != 3:
        raise _lib.ScreamHipError("the packed prediction is [rows_src,3], got %s" % (tuple(pred.shape),))
    if target is not None:
        if tuple(target.shape) != tuple(pred.shape):
            raise _lib.ScreamHipError("the packed target must have the prediction's shape %s, got %s" % (tuple(pred.shape), tuple(target.shape)))
    elif xyz.shape[0] < rows_src or rot.numel() != 9 * n_pairs or trans.numel() != 3 * n_pairs:
        raise _lib.ScreamHipError("l1_pairs: xyz / rot / trans do not describe %d pairs over %d source rows" % (n_pairs, rows_src))
    return pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len, rows_src


def l1_pairs_fwd(pred: torch.Tensor, xyz: Optional[torch.Tensor], rot: Optional[torch.Tensor], trans: Optional[torch.Tensor],
                 target: Optional[torch.Tensor], cloud_row0: torch.Tensor, cloud_len: torch.Tensor, n_pairs: int,
                 max_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """scream_l1_pairs_fwd: (loss fp32 scalar, loss_pair float64 [B]) of the packed prediction [rows_src,3] against rot / trans
    applied to the packed xyz, or against the packed `target` [rows_src,3] when it is given.  No host sync."""
    dev = pred.device
    workspace = _workspace("scream_l1_pairs_workspace_bytes", n_pairs, max_len, device=dev)
    loss_pair = torch.empty(n_pairs, device=dev, dtype=torch.float64)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call("scream_l1_pairs_fwd", *_l1_args(pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len), loss_pair, loss,
         workspace, workspace.numel())
    return loss, loss_pair


def l1_pairs_bwd(dout: torch.Tensor, pred: torch.Tensor, xyz, rot, trans, target, cloud_row0: torch.Tensor, cloud_len: torch.Tensor,
                 n_pairs: int, max_len: int) -> torch.Tensor:
    """scream_l1_pairs_bwd: dpred fp32 [rows_src,3] for the upstream gradient `dout` (one fp32 on the device)."""
    dpred = torch.empty_like(pred)
    call("scream_l1_pairs_bwd", dout, *_l1_args(pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len), dpred)
    return dpred


def _chamfer_args(a, a_row0, a_len, max_a_len, b, b_row0, b_len, max_b_len):
    for name, t in (("a", a), ("b", b)):
        if t.dim() != 2 or t.shape[1] != 3:
            raise _lib.ScreamHipError("chamfer: %s is packed [rows,3], got %s" % (name, tuple(t.shape)))
    n_pairs = a_row0.shape[0]
    if not (a_len.shape[0] == b_row0.shape[0] == b_len.shape[0] == n_pairs):
        raise _lib.ScreamHipError("chamfer: row0 / len of a and b must have one entry per pair")
    # (an empty tensor has no address; the library is told 0 rows and reads none)
    one = lambda t: t if t.shape[0] else t.new_zeros(1, 3)
    return one(a), a_row0, a_len, a.shape[0], max_a_len, one(b), b_row0, b_len, b.shape[0], max_b_len, n_pairs


def chamfer_fwd(a: torch.Tensor, a_row0, a_len, max_a_len: int, b: torch.Tensor, b_row0, b_len, max_b_len: int):
    """scream_chamfer_fwd over packed clouds: (loss fp32 scalar, loss_pair float64 [B], idx_ab int32 [a_rows], d_ab fp32 [a_rows],
    idx_ba [b_rows], d_ba [b_rows]).  No host sync."""
    dev = a.device
    args = _chamfer_args(a, a_row0, a_len, max_a_len, b, b_row0, b_len, max_b_len)
    ar, br, n_pairs = a.shape[0], b.shape[0], args[-1]
    chunk = lambda n: (n + 255) // 256
    keys_a = torch.empty(max(ar, 1), device=dev, dtype=torch.int64)
    keys_b = torch.empty(max(br, 1), device=dev, dtype=torch.int64)
    part = torch.empty(max(n_pairs * (chunk(max_a_len) + chunk(max_b_len)), 1), device=dev, dtype=torch.float64)
    idx_ab, d_ab = torch.empty(max(ar, 1), device=dev, dtype=torch.int32), torch.empty(max(ar, 1), device=dev, dtype=torch.float32)
    idx_ba, d_ba = torch.empty(max(br, 1), device=dev, dtype=torch.int32), torch.empty(max(br, 1), device=dev, dtype=torch.float32)
    loss_pair = torch.empty(n_pairs, device=dev, dtype=torch.float64)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call("scream_chamfer_fwd", *args, keys_a, keys_b, part, idx_ab, d_ab, idx_ba, d_ba, loss_pair, loss)
    return loss, loss_pair, idx_ab[:ar], d_ab[:ar], idx_ba[:br], d_ba[:br]


def chamfer_bwd(dout: torch.Tensor, a: torch.Tensor, a_row0, a_len, max_a_len: int, b: torch.Tensor, b_row0, b_len, max_b_len: int,
                idx_ab: torch.Tensor, idx_ba: torch.Tensor, need_a: bool = True, need_b: bool = True):
    """scream_chamfer_bwd: (da, db) fp32 like a and b for the upstream gradient `dout` (one fp32 on the device); None for a side
    that is not needed."""
    args = _chamfer_args(a, a_row0, a_len, max_a_len, b, b_row0, b_len, max_b_len)
    da, db = torch.empty_like(a) if need_a else None, torch.empty_like(b) if need_b else None
    one = lambda t: t if t.shape[0] else t.new_zeros(1)
    call("scream_chamfer_bwd", dout, *args, one(idx_ab), one(idx_ba), da if a.shape[0] else None, db if b.shape[0] else None)
    return da, db


def kabsch_corr(src, ref, src_row0, src_len, ref_row0, idx, valid, s, c) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (T [n_pairs,4,4], n_corr int32 [n_pairs])."""
    n_pairs = s.shape[0]
    T = torch.empty(n_pairs, 4, 4, device=src.device, dtype=torch.float32)
    n_corr = torch.empty(n_pairs, device=src.device, dtype=torch.int32)
    call("scream_kabsch_corr", src, ref, src_row0, src_len, ref_row0, idx, valid, s, c, n_pairs, T, n_corr)
    return T, n_corr


def rigid_transform_3d_dense(A: torch.Tensor, B: torch.Tensor, w: Optional[torch.Tensor], thr: float) -> torch.Tensor:
    bs, K = A.shape[0], A.shape[1]
    T = torch.empty(bs, 4, 4, device=A.device, dtype=torch.float32)
    call("scream_rigid_transform_3d", A if K else None, B if K else None, w, thr, bs, K, T)
    return T


def transformation_error_batched(T_pred: torch.Tensor, T_gt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    n = T_pred.shape[0]
    re = torch.empty(n, device=T_pred.device, dtype=torch.float32)
    te = torch.empty(n, device=T_pred.device, dtype=torch.float32)
    call("scream_transformation_error", T_pred, T_gt, n, re, te)
    return re, te


def point_loss(src_pred: torch.Tensor, src: torch.Tensor, src_row0, src_len, rot: torch.Tensor, trans: torch.Tensor) -> torch.Tensor:
    """models/pointnet.py:93-99 per pair of a packed batch: loss[p] = mean_n sum_xyz |src_pred_n - (rot_p src_n + trans_p)|.
    src_pred / src packed [rows,3]; rot [B,3,3]; trans [B,3,1] or [B,3]."""
    B = rot.shape[0]
    out = torch.empty(B, device=src_pred.device, dtype=torch.float32)
    call("scream_point_loss", src_pred, src, src_row0, src_len, rot.reshape(B, 9).contiguous(), trans.reshape(B, 3).contiguous(), B, out)
    return out


def icp_p2p(src, ref, src_row0, src_len, ref_row0, ref_len, s, c, T_init, max_src_len: int, max_ref_len: int,
            max_corr_dist: float, max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, search: str = "grid"):
    """Batched point-to-point ICP (scream_icp_p2p).  Returns (T [n,4,4], fitness_rmse [n,2], iters int32 [n]).
    search="brute": the yardstick of the tests and of tools/icp_bench.py (scream_icp_p2p_brute_range), the same bits, slower."""
    range_name = _icp_range_name(search)
    n_pairs = s.shape[0]
    dev = src.device
    T = T_init.detach().clone().contiguous().float()
    fr = torch.empty(n_pairs, 2, device=dev, dtype=torch.float32)
    iters = torch.empty(n_pairs, device=dev, dtype=torch.int32)
    ws = _icp_workspace(src, ref, n_pairs)
    args = (src, ref, src_row0, src_len, ref_row0, ref_len, s, c, n_pairs, max_src_len, max_ref_len, src.shape[0], ref.shape[0],
            max_corr_dist, max_iter, rel_fitness, rel_rmse, T, fr, iters)
    if search == "grid":
        call("scream_icp_p2p", *args, ws, ws.numel())
    else:  # the whole schedule, as scream_icp_p2p enqueues it
        call(range_name, *args, 0, int(max_iter) + 2, None, ws, ws.numel())
    return T, fr, iters


def _icp_range_name(search: str) -> str:
    """The entry point that enqueues a piece of an ICP run with this search."""
    if search not in ("grid", "brute"):
        raise ValueError('search must be "grid" or "brute", not %r' % (search,))
    return "scream_icp_p2p_range" if search == "grid" else "scream_icp_p2p_brute_range"


def _icp_workspace(src, ref, n_pairs: int) -> torch.Tensor:
    return _workspace("scream_icp_workspace_bytes", src.shape[0], ref.shape[0], n_pairs, device=src.device)


def icp_raw_workspace(src_rows: int, tgt_rows: int, n_pairs: int, device) -> torch.Tensor:
    """Scratch of scream_icp_raw_range / scream_icp_raw_nn (scream_amd/rawicp.py)."""
    return _workspace("scream_icp_raw_workspace_bytes", src_rows, tgt_rows, n_pairs, device=device, floor=256)


ICP_ASYNC_ITERS = 64  # schedules up to this many iterations are enqueued whole (icp_p2p); longer ones in pieces (IcpRun)


class PiecewiseRun:
    """A LONG schedule of per-pair steps enqueued in pieces, so that launching stops once every pair has stopped WITHOUT the host
    ever waiting inside the C ABI: ``advance(k)`` enqueues the next k steps on the current stream (the subclass's ``_enqueue(begin,
    end)``, one C call) and, behind them, a copy of the per-pair stopped flags into pinned memory + an event; ``all_stopped()``
    waits for THAT event only, not for the stream's later work, and reads the flags.  A pair's result does not depend on the piece
    sizes (tests/test_gpu_evaluate.py, tests/test_gpu_rawicp.py)."""

    def __init__(self, n: int, steps: int, dev, skip_empty: bool = False):
        """n pairs, `steps` steps at most; skip_empty: a run of no pairs enqueues nothing (else the library sees n = 0)."""
        self.n, self.steps, self.next_it = n, steps, 0
        self._dev, self._skip = dev, skip_empty and n == 0
        self.flags = torch.zeros(max(n, 1), device=dev, dtype=torch.int32)[:n]
        self.flags_host = torch.zeros(max(n, 1), dtype=torch.int32, pin_memory=True)[:n]
        self.event = None

    @property
    def steps_left(self) -> int:
        return self.steps - self.next_it

    def advance(self, k: int) -> None:
        end = min(self.next_it + int(k), self.steps)
        if self._skip:
            self.next_it = self.steps
            return
        self._enqueue(self.next_it, end)
        self.next_it = end
        self.flags_host.copy_(self.flags, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(self._dev))

    def all_stopped(self) -> bool:
        if self._skip:
            return True
        self.event.synchronize()
        return self.steps_left == 0 or bool(self.flags_host.all())

    def run(self, piece: int = 32):
        """Enqueue pieces until every pair has stopped: after each piece the host waits for that piece's flags (its event, not the
        stream) and enqueues the next one only if a pair still runs, so no more than ceil(steps taken / piece) pieces are launched."""
        if piece < 1:
            raise ValueError("piece must be at least 1")
        self.advance(piece)
        while not self.all_stopped():
            self.advance(piece)
        return self


class IcpRun(PiecewiseRun):
    """scream_icp_p2p_range in pieces (KITTI: up to 1000 iterations, evaluate_kitti.py:64-70): a step is one launch, max_iter + 2 of
    them.  The caller calls ``all_stopped()`` when it collects the batch, i.e. after the following batches were enqueued.  ``T``
    holds the refined transform of every pair whose flag is set.  Results are those of icp_p2p whatever the piece sizes."""

    def __init__(self, src, ref, src_row0, src_len, ref_row0, ref_len, s, c, T_init, max_src_len: int, max_ref_len: int,
                 max_corr_dist: float, max_iter: int, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, search: str = "grid"):
        self._entry = _icp_range_name(search)  # one search for the whole run
        n = s.shape[0]
        dev = src.device
        self.max_iter = int(max_iter)
        super().__init__(n, self.max_iter + 2, dev)
        self.T = T_init.detach().clone().contiguous().float()
        self.fr = torch.empty(n, 2, device=dev, dtype=torch.float32)
        self.iters = torch.empty(n, device=dev, dtype=torch.int32)
        self.ws = _icp_workspace(src, ref, n)
        self._args = (src, ref, src_row0, src_len, ref_row0, ref_len, s, c, n, max_src_len, max_ref_len, src.shape[0], ref.shape[0],
                      max_corr_dist, max_iter, rel_fitness, rel_rmse, self.T, self.fr, self.iters)

    launches_left = PiecewiseRun.steps_left

    def _enqueue(self, begin: int, end: int) -> None:
        call(self._entry, *self._args, begin, end, self.flags, self.ws, self.ws.numel())


# ---- the adversarial loss (csrc/gan.hip): contiguous NCHW fp32 tensors, torch's [Cout,Cin,4,4] weights
GAN_FWD, GAN_DGRAD, GAN_WGRAD = 0, 1, 2


def _conv_out(h: int, w: int, stride: int) -> Tuple[int, int]:
    return (h - 2) // stride + 1, (w - 2) // stride + 1


def _gan_conv_ws(mode: int, n, cin, cout, h, w, stride, device) -> torch.Tensor:
    return _workspace("scream_gan_conv_workspace_bytes", mode, n, cin, cout, h, w, stride, device=device)


def gan_conv_fwd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int, leaky: bool = False) -> torch.Tensor:
    """scream_gan_conv_fwd: conv(k4, p1, stride) of x [n,cin,h,w] (+ bias, then LeakyReLU 0.2 when asked) -> [n,cout,ho,wo]."""
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = _conv_out(h, w, stride)
    y = torch.empty(n, cout, ho, wo, device=x.device, dtype=torch.float32)
    ws = _gan_conv_ws(GAN_FWD, n, cin, cout, h, w, stride, x.device)
    call("scream_gan_conv_fwd", x, weight, bias, n, cin, cout, h, w, stride, leaky, y, ws, ws.numel())
    return y


def gan_conv_dgrad(dy: torch.Tensor, weight: torch.Tensor, h: int, w: int, stride: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scream_gan_conv_dgrad: the gradient of the [n,cin,h,w] input for dy; `mask` (the input's shape): times (mask > 0 ? 1 : 0.2)."""
    n, cout = dy.shape[0], dy.shape[1]
    cin = weight.shape[1]
    dx = torch.empty(n, cin, h, w, device=dy.device, dtype=torch.float32)
    ws = _gan_conv_ws(GAN_DGRAD, n, cin, cout, h, w, stride, dy.device)
    call("scream_gan_conv_dgrad", dy, weight, mask, n, cin, cout, h, w, stride, dx, ws, ws.numel())
    return dx


def gan_conv_wgrad(x: torch.Tensor, dy: torch.Tensor, stride: int, want_bias: bool = False):
    """scream_gan_conv_wgrad: (dw [cout,cin,4,4], dbias [cout] or None)."""
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    dw = torch.empty(cout, cin, 4, 4, device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if want_bias else None
    ws = _gan_conv_ws(GAN_WGRAD, n, cin, cout, h, w, stride, x.device)
    call("scream_gan_conv_wgrad", x, dy, n, cin, cout, h, w, stride, dw, db, ws, ws.numel())
    return dw, db


def gan_bn_fwd(x: torch.Tensor, gamma, beta, running_mean, running_var, num_batches_tracked, training: bool = True):
    """scream_gan_bn_fwd: BatchNorm2d + LeakyReLU(0.2) of x [n,c,h,w]; the running statistics are updated in place in training
    mode.  Returns (y, mean [c], invstd [c])."""
    n, c = x.shape[0], x.shape[1]
    hw = x.shape[2] * x.shape[3]
    if training and n * hw == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    y = torch.empty_like(x)
    mean = torch.empty(c, device=x.device, dtype=torch.float32)
    invstd = torch.empty(c, device=x.device, dtype=torch.float32)
    call("scream_gan_bn_fwd", x, gamma, beta, running_mean, running_var, num_batches_tracked, n, c, hw, training, y, mean, invstd)
    return y, mean, invstd


def gan_bn_bwd(dy: torch.Tensor, y: torch.Tensor, x: torch.Tensor, gamma, mean, invstd):
    """scream_gan_bn_bwd: (dx, dgamma, dbeta) for dy, the gradient of gan_bn_fwd's y."""
    n, c = x.shape[0], x.shape[1]
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty_like(mean), torch.empty_like(mean)
    sums = torch.empty(2 * c, device=x.device, dtype=torch.float64)
    call("scream_gan_bn_bwd", dy, y, x, gamma, mean, invstd, n, c, x.shape[2] * x.shape[3], sums, dx, dgamma, dbeta)
    return dx, dgamma, dbeta


def gan_loss_g(logits: torch.Tensor) -> torch.Tensor:
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    call("scream_gan_loss_g", logits, logits.numel(), loss)
    return loss


def gan_loss_g_bwd(dout: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    d = torch.empty_like(like)
    call("scream_gan_loss_g_bwd", dout, d.numel(), d)
    return d


def gan_loss_d(real: torch.Tensor, fake: torch.Tensor) -> torch.Tensor:
    loss = torch.empty((), device=real.device, dtype=torch.float32)
    call("scream_gan_loss_d", real, real.numel(), fake, fake.numel(), loss)
    return loss


def gan_loss_d_bwd(dout: torch.Tensor, real: torch.Tensor, fake: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    dr, df = torch.empty_like(real), torch.empty_like(fake)
    call("scream_gan_loss_d_bwd", dout, real, real.numel(), fake, fake.numel(), dr, df)
    return dr, df


def pairs_transform(xyz: torch.Tensor, rot: torch.Tensor, trans: torch.Tensor, tile_cloud: torch.Tensor, n_pairs: int,
                    rows_src: int) -> torch.Tensor:
    """scream_pairs_transform: R_p x + t_p on the packed source rows of every pair, one launch -> [rows_src,3]."""
    out = torch.empty(rows_src, 3, device=xyz.device, dtype=torch.float32)
    call("scream_pairs_transform", xyz, rot.reshape(n_pairs, 9), trans.reshape(n_pairs, 3), tile_cloud, n_pairs, rows_src, out)
    return out


def _gan_struct(cls, fields: dict):
    s = cls()
    for name, value in fields.items():
        if isinstance(value, (list, tuple)):
            arr = getattr(s, name)
            for i, t in enumerate(value):
                arr[i] = t
        else:
            setattr(s, name, value)
    return s


def gan_params(weights, b0, b4, gammas, betas, running_means, running_vars, nbts) -> "_lib.GanParamsT":
    """The scream_gan_params_t of a discriminator's tensors (the caller keeps them alive)."""
    return _gan_struct(_lib.GanParamsT, dict(w=[_p(t) for t in weights], b0=_p(b0), b4=_p(b4), gamma=[_p(t) for t in gammas],
                                             beta=[_p(t) for t in betas], running_mean=[_p(t) for t in running_means],
                                             running_var=[_p(t) for t in running_vars],
                                             num_batches_tracked=[_p(t, torch.int64) for t in nbts]))


def gan_workspace(n: int, cin: int, ndf: int, h: int, w: int, device) -> torch.Tensor:
    return _workspace("scream_gan_workspace_bytes", n, cin, ndf, h, w, device=device)


def gan_forward(x: torch.Tensor, params, ndf: int, training: bool, workspace: torch.Tensor) -> torch.Tensor:
    """scream_gan_forward: logits [n,1,h5,w5]; the workspace keeps the pass's activations for gan_backward."""
    n, cin, h, w = x.shape
    for s in (2, 2, 2, 1, 1):
        h, w = _conv_out(h, w, s)
    logits = torch.empty(n, 1, h, w, device=x.device, dtype=torch.float32)
    call("scream_gan_forward", x, params, n, cin, ndf, x.shape[2], x.shape[3], training, logits, workspace, workspace.numel())
    return logits


def gan_backward(dlogits: torch.Tensor, x: torch.Tensor, params, ndf: int, workspace: torch.Tensor, want_dx: bool, grads):
    """scream_gan_backward: dx (or None); `grads` is a list of the 13 gradient tensors in the order (w x 5, b0, b4, gamma x 3,
    beta x 3) to be written, or None for no parameter gradient."""
    n, cin, h, w = x.shape
    dx = torch.empty_like(x) if want_dx else None
    g = None
    if grads is not None:
        g = _gan_struct(_lib.GanGradsT, dict(w=[_p(t) for t in grads[0:5]], b0=_p(grads[5]), b4=_p(grads[6]),
                                             gamma=[_p(t) for t in grads[7:10]], beta=[_p(t) for t in grads[10:13]]))
    call("scream_gan_backward", dlogits, x, params, n, cin, ndf, h, w, workspace, workspace.numel(), dx, g)
    return dx
