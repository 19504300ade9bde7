"""ctypes binding of libscream_hip.so, derived from include/scream_hip.h.

The header is the one statement of the C ABI: it is parsed once, when this module is imported, into PROTOTYPES (per function:
return type, argument types, parameter names, what every pointer points to, whether it ends in `void* stream`) and SIGNATURES
(name -> (restype, argtypes), what load() gives ctypes).  A prototype the parser cannot read, or a struct pointer without a
class below, raises at import: nothing is skipped.  Only the five ctypes.Structure classes are still written by hand beside
their typedefs.  ops.call marshals every argument by these declarations.

The product path has no CPU fallback: if the library cannot be built/loaded the first use
raises, loudly.  ``SCREAM_NO_BUILD=1`` forbids the lazy hipcc build (the GPU box normally
receives the prebuilt .so with the snapshot).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, NamedTuple, Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCREAM_LIB=<path>: load that build instead (A/B runs of two builds on the same GPU box; never built automatically)
LIB_PATH = os.environ.get("SCREAM_LIB") or os.path.join(_HERE, "libscream_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "scream_hip.h")
ABI_VERSION = 21

SPLIT_H1, SPLIT_H2, SPLIT_BF3 = 1, 2, 3


class TailExpsT(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("e_att", "e_wm", "e_m1", "e_w1", "e_h", "e_w2", "e_y", "e_wq", "e_q")]


class LayerT(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("wqkv", "wq", "wkv", "wm", "w1", "w2", "g1", "b1", "g2", "b2", "tail")] +
                [(n, C.c_int32) for n in ("e_xq", "e_xkv", "e_wqkv", "e_wq", "e_k", "e_v")] +
                [("tail_exps", TailExpsT), ("tail_next_q", C.c_int32), ("proj", C.c_void_p)])


class ModelT(C.Structure):
    _fields_ = [("n_self", C.c_int32), ("n_cross", C.c_int32), ("dim_t", C.c_void_p), ("emb_w", C.c_void_p),
                ("emb_b", C.c_void_p), ("pre_g", C.c_void_p), ("pre_b", C.c_void_p),
                ("layers_host", C.POINTER(LayerT)), ("c0_w", C.c_void_p), ("c0_b", C.c_void_p),
                ("c2_w", C.c_void_p), ("c2_b", C.c_void_p), ("c4_w", C.c_void_p), ("c4_b", C.c_void_p),
                ("stem_tgt_layers_host", C.POINTER(LayerT)), ("gemm_split", C.c_int32),
                ("e_c0x", C.c_int32), ("e_c0w", C.c_int32), ("e_c2x", C.c_int32), ("e_c2w", C.c_int32),
                ("wkv_cross", C.c_void_p), ("e_wkv_cross", C.c_int32), ("e_k_cross", C.c_int32), ("e_v_cross", C.c_int32),
                ("proj_cross", C.c_void_p)]


class BatchT(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("rows_src", C.c_int64), ("rows_total", C.c_int64),
                ("max_chunks", C.c_int32), ("xyz", C.c_void_p), ("center", C.c_void_p),
                ("tile_cloud", C.c_void_p), ("cloud_row0", C.c_void_p), ("cloud_len", C.c_void_p)]


class GanParamsT(C.Structure):
    _fields_ = [("w", C.c_void_p * 5), ("b0", C.c_void_p), ("b4", C.c_void_p), ("gamma", C.c_void_p * 3), ("beta", C.c_void_p * 3),
                ("running_mean", C.c_void_p * 3), ("running_var", C.c_void_p * 3), ("num_batches_tracked", C.c_void_p * 3)]


class GanGradsT(C.Structure):
    _fields_ = [("w", C.c_void_p * 5), ("b0", C.c_void_p), ("b4", C.c_void_p), ("gamma", C.c_void_p * 3), ("beta", C.c_void_p * 3)]


# the structs an entry point takes by pointer (scream_layer_t is reached only through scream_model_t)
STRUCTS = {"scream_tail_exps_t": TailExpsT, "scream_model_t": ModelT, "scream_batch_t": BatchT,
           "scream_gan_params_t": GanParamsT, "scream_gan_grads_t": GanGradsT}
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_POINTEES = ("float", "int32_t", "int64_t", "uint64_t", "uint8_t", "double", "void")
_RETURNS = dict(_SCALARS, **{"void": None, "void*": C.c_void_p, "const char*": C.c_char_p})


class Prototype(NamedTuple):
    restype: object
    argtypes: Tuple
    params: Tuple[str, ...]  # the parameter names
    pointees: Tuple          # per parameter: None (a scalar), the pointee's C type name, or the Structure class of a struct pointer
    stream: bool             # the last parameter is `void* stream`


def parse_header(text: str) -> Dict[str, Prototype]:
    """Every function prototype of a C header in the style of include/scream_hip.h.  What is left of the text without comments,
    preprocessor lines, the extern "C" guard, struct typedefs and enums must be prototypes over the types above, every one;
    anything else raises ValueError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\{[^}]*\}\s*\w+\s*;|enum\s*\{[^}]*\}\s*;", " ", text)
    out = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?) ?\b(\w+) ?\((.*)\)", stmt)
        if m is None or m.group(1) not in _RETURNS or m.group(2) in out:
            raise ValueError("cannot read the prototype %r" % stmt)
        name, argtypes, params, pointees = m.group(2), [], [], []
        for decl in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            p = re.fullmatch(r"(const )?(\w+) ?(\*?) ?(\w+)", decl.strip())
            if p is None:
                raise ValueError("%s: cannot read the parameter %r" % (name, decl.strip()))
            const, base, star, pname = p.groups()
            if not star and not const and base in _SCALARS:
                ctype, pointee = _SCALARS[base], None
            elif star and base in _POINTEES:
                ctype, pointee = C.c_void_p, base  # data pointers travel as integers (tensor.data_ptr())
            elif star and const and base in STRUCTS:
                ctype, pointee = C.POINTER(STRUCTS[base]), STRUCTS[base]
            else:
                raise ValueError("%s: no ctypes class for the parameter %r" % (name, decl.strip()))
            argtypes.append(ctype), params.append(pname), pointees.append(pointee)
        out[name] = Prototype(_RETURNS[m.group(1)], tuple(argtypes), tuple(params), tuple(pointees),
                              bool(params) and params[-1] == "stream" and pointees[-1] == "void")
    return out


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_header(_f.read())
SIGNATURES = {name: (p.restype, list(p.argtypes)) for name, p in PROTOTYPES.items()}  # every symbol the header declares

_lib: Optional[C.CDLL] = None


class ScreamHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (building first if the in-tree .so is missing/stale and hipcc is present)."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("SCREAM_NO_BUILD", "0") != "1" and not os.environ.get("SCREAM_LIB"):
        try:
            from . import build as _build
            _build.build()
        except Exception as e:  # no hipcc on this host: fall through to the prebuilt library
            if not os.path.exists(LIB_PATH):
                raise ScreamHipError("libscream_hip.so is missing and could not be built: %s" % e) from e
    if not os.path.exists(LIB_PATH):
        raise ScreamHipError("libscream_hip.so not found at %s (run `python -m scream_amd.build`)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ScreamHipError("libscream_hip.so does not export %s" % name) from e
        fn.restype = res
        fn.argtypes = args
    if lib.scream_abi_version() != ABI_VERSION:
        raise ScreamHipError("libscream_hip.so ABI %d != binding ABI %d" % (lib.scream_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc == -1:
        raise ScreamHipError("%s: invalid argument (SCREAM_EINVAL)" % what)
    if rc == -2:
        raise ScreamHipError("%s: unsupported shape (SCREAM_EUNSUPPORTED)" % what)
    raise ScreamHipError("%s: HIP error %d" % (what, rc))
