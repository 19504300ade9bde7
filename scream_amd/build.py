"""Build libscream_hip.so (gfx950) in-tree with hipcc.  No torch headers are involved: the library
is a plain C-ABI shared object (include/scream_hip.h) loaded with ctypes."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from . import asm_check

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libscream_hip.so")
OBJDIR = os.path.join(HERE, "build")
ARCH = "gfx950"

# parity-critical files keep every fp32 operation individually rounded (see the file headers)
SOURCES = {
    "gemm_f32.hip": [],
    "gemm_split.hip": [],
    # train_backend "bf16": one bf16 product per GEMM (forward, data gradient, weight gradient)
    "gemm_bf16.hip": [],
    # the MFMA results of this kernel are consumed by vector instructions (every chunk's epilogue rides under the next chunk's
    # matrix instructions) while its row operand planes fill the whole AGPR file: accumulators in VGPRs, no moves between the files
    "proj_ring.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    # several code instances of the same arithmetic (an attention apply in the open / riding under another stage) must round
    # identically, whatever hipcc makes of each: no fma contraction in this file
    "tail_split.hip": ["-ffp-contract=off"],
    "embed.hip": [],
    "attention.hip": [],
    "backward.hip": [],
    "forward.hip": [],
    "nn_search.hip": ["-ffp-contract=off"],
    "kabsch.hip": ["-ffp-contract=off"],
    "icp_p2p.hip": ["-ffp-contract=off"],
    "icp_grid.hip": ["-ffp-contract=off"],
    "render.hip": ["-ffp-contract=off"],
    "voxel.hip": ["-ffp-contract=off"],
    "dsm.hip": ["-ffp-contract=off"],
    "radius.hip": ["-ffp-contract=off"],
    "prep.hip": ["-ffp-contract=off"],
    # every step of the raw-scan ICP is one IEEE float64 operation in a documented order (the file header)
    "icp_raw.hip": ["-ffp-contract=off"],
    # the Adam update is one IEEE float64 operation per step of its contract, restated in numpy by tests/adam_ref.py
    "optim.hip": ["-ffp-contract=off"],
    # the discriminator's BatchNorm and loss steps are individually rounded operations restated by tests/gan_ref.py
    "gan.hip": ["-ffp-contract=off"],
    # the Chamfer distance is one rounded fp32 operation per step forward, one float64 operation per step backward, restated by
    # tests/chamfer_ref.py
    "chamfer.hip": ["-ffp-contract=off"],
}
# The gate: what asm_check.gate() must pass on a file's generated code before the library is linked, as (asm loads, no scratch).
# asm loads: the file requests operands with inline asm and waits for them with hand-counted s_waitcnt vmcnt(N); whether hipcc's
# register allocation respects that is a property of the generated code, not of the source, so the build proves it on the very code
# it ships (same flags, assembly instead of an object) and FAILS if any instruction touches a register whose load is outstanding.
# no scratch: kernels (name fragments) that must not touch scratch at all.
GATE = {
    "gemm_split.hip": (True, ()),
    # a spill inside a ring stage costs a round trip per stage, and hipcc orders a scratch reload against the LDS-DMA in flight with
    # vmcnt(0) -- the ring would drain once per stage (the layer tail's history)
    "tail_split.hip": (True, ("tail_kernelINS_7SplitH2", "tail_kernelINS_7SplitH1")),
    "proj_ring.hip": (True, ("proj_ring_kernel",)),
    # the raw-scan ICP search keeps its eight stepped binary searches and its best candidate in registers (a spill would sit inside
    # the dependent-load chain that bounds it)
    "icp_raw.hip": (False, ("raw_search_kernel", "raw_nn_kernel")),
    # the bf16 training GEMMs hold a 32 x 256 accumulator tile and both operands' next k-tile in registers
    "gemm_bf16.hip": (False, ("gemm_bf16_kernel", "wgrad_split_partial_kernel")),
    # the scan carries four queries' coordinates, minima and indices per thread in registers; the re-scan of the backward its sums
    "chamfer.hip": (False, ("chamfer_scan_kernel", "chamfer_bwd_kernel")),
}
COMMON = ["-O3", "-std=c++17", "--offload-arch=" + ARCH, "-fPIC", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libscream_hip.so")
    return exe


def _stale(target: str) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "scream_hip.h"), __file__]
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src: str, out: str, flags=None, asm: bool = False, verbose: bool = False) -> str:
    """The one hipcc command line of a source (a file of csrc/ by name, or an absolute path): the object the library is linked from, or with
    asm=True the assembly of the same device code.  flags: instead of the file's own in SOURCES."""
    flags = SOURCES[os.path.basename(src)] if flags is None else list(flags)
    cmd = [_hipcc()] + COMMON + flags + (["-S", "--cuda-device-only"] if asm else ["-c"]) + [os.path.join(CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), r.stderr))
    if verbose and r.stderr.strip():
        print(r.stderr, file=sys.stderr)
    return out


def assembly(src: str, flags=None, out: str = None, force: bool = False) -> str:
    """Path of the gfx950 assembly of a source: by default with the shipped flags, as scream_amd/build/<name>.s -- the file the gate
    reads and the CPU tests assert on, generated once and again only when a source, the header or this file is newer.  With flags
    or out (experiment builds, test fixtures) it is generated on every call."""
    shipped = flags is None and out is None
    out = out or os.path.join(OBJDIR, os.path.basename(src).replace(".hip", ".s"))
    if force or not shipped or _stale(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        os.replace(_compile(src, out + ".tmp", flags, asm=True), out)
    return out


def build(force: bool = False, verbose: bool = False, out: str = None) -> str:
    """out: write the library there instead of scream_amd/libscream_hip.so (experiment builds loaded with SCREAM_LIB=)."""
    lib, force = out or LIB, force or bool(out)
    if not force and not _stale(lib):
        return lib
    os.makedirs(OBJDIR, exist_ok=True)

    def gate(src):
        return asm_check.gate(assembly(src, force=force), *GATE[src])

    with ThreadPoolExecutor(max_workers=4) as ex:
        checks = [ex.submit(gate, src) for src in GATE] if os.environ.get("SCREAM_BUILD_VERIFY", "1") != "0" else []
        objs = list(ex.map(lambda src: _compile(src, os.path.join(OBJDIR, src.replace(".hip", ".o")), verbose=verbose), SOURCES))
        for c in checks:
            c.result()
    r = subprocess.run([_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib + ".tmp"] + objs, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n%s" % r.stderr)
    os.replace(lib + ".tmp", lib)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
