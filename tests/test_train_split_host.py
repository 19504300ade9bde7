"""The split-arithmetic training surface that needs no GPU: the train_backend attribute of PointTransformer / DEMTransformer and
the host-side argument checks of scream_gemm_wgrad_split_f32 (include/scream_hip.h)."""
import os
import subprocess
import sys

import pytest

from scream_amd import _lib
from scream_amd.model import DEMTransformer, PointTransformer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_backend_defaults_to_f32_and_validates_on_assignment():
    for cls in (PointTransformer, DEMTransformer):
        net = cls(256, 1, 1)
        assert net.train_backend == "f32"
        net.train_backend = "split"
        assert net.train_backend == "split"
        assert cls(256, 1, 1).train_backend == "f32"  # per model, not per class
        for bad in ("h1", "bogus", "h2", None):
            with pytest.raises(ValueError, match="'f32', 'split'"):
                net.train_backend = bad
        assert net.train_backend == "split"  # a refused assignment changes nothing
        net.train_backend = "f32"
        assert net.train_backend == "f32"
        assert net.train() is net and net._trains()


def _child(env_value, code):
    env = dict(os.environ, SCREAM_TRAIN_GEMM=env_value, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_environment_sets_the_class_default():
    r = _child("split", "from scream_amd.model import PointTransformer, DEMTransformer\n"
                        "n = PointTransformer(256, 1, 1)\n"
                        "assert n.train_backend == 'split' and DEMTransformer(256, 1, 1).train_backend == 'split'\n"
                        "n.train_backend = 'f32'\n"
                        "assert n.train_backend == 'f32' and PointTransformer(256, 1, 1).train_backend == 'split'\n"
                        "n.train()\n")
    assert r.returncode == 0, r.stderr


def test_bad_environment_value_raises_at_the_first_train():
    r = _child("bogus", "from scream_amd.model import PointTransformer\n"
                        "n = PointTransformer(256, 1, 1)\n"
                        "n.eval()\n"  # inference never looks at it
                        "try:\n"
                        "    n.train()\n"
                        "except ValueError as e:\n"
                        "    assert \"'f32', 'split'\" in str(e) and 'bogus' in str(e)\n"
                        "else:\n"
                        "    raise SystemExit('train() accepted SCREAM_TRAIN_GEMM=bogus')\n")
    assert r.returncode == 0, r.stderr + r.stdout


def test_split_wgrad_entry_point_checks_its_arguments_on_the_host():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.scream_abi_version() == 21
    ws = lib.scream_wgrad_split_workspace_bytes(330000, 256, 256)
    assert ws > 0 and ws % ((256 * 256 + 256) * 4) == 0  # one partial slab of N x K (+ N column sums) per row slice
    assert lib.scream_wgrad_split_workspace_bytes(128, 256, 256) == (256 * 256 + 256) * 4
    assert lib.scream_wgrad_split_workspace_bytes(330000, 200, 256) == -1
    assert lib.scream_wgrad_split_workspace_bytes(0, 256, 256) == 0
    EINVAL, EUNSUPPORTED = -1, -2
    BF3, H2, H1 = _lib.SPLIT_BF3, _lib.SPLIT_H2, _lib.SPLIT_H1
    # NULL operands
    assert lib.scream_gemm_wgrad_split_f32(None, 256, None, 256, 128, 256, 256, None, 0, None, BF3, None, 0, None) == EINVAL
    # non-NULL (never dereferenced: every check below fails before a launch) operands with a split other than bf16 x 3
    p = 1 << 20
    for split in (H2, H1, 0, 4):
        assert lib.scream_gemm_wgrad_split_f32(p, 256, p, 256, 128, 256, 256, p, 0, None, split, p, ws, None) == EINVAL
    assert lib.scream_gemm_wgrad_split_f32(p, 256, p, 256, 128, 200, 256, p, 0, None, BF3, p, ws, None) == EUNSUPPORTED
    assert lib.scream_gemm_wgrad_split_f32(p, 128, p, 256, 128, 256, 256, p, 0, None, BF3, p, ws, None) == EINVAL  # ldy < N
    assert lib.scream_gemm_wgrad_split_f32(p, 256, p, 256, 128, 256, 256, p, 0, None, BF3, None, 0, None) == EINVAL  # no workspace
    assert lib.scream_gemm_wgrad_split_f32(p, 256, p, 256, 128, 256, 256, p, 0, None, BF3, p, 16, None) == EINVAL  # too small


def test_split_wgrad_kernel_code_is_bf16_mfma_without_scratch(tmp_path):
    """The generated gfx950 code of the new kernel: bf16 matrix instructions, no scratch traffic, 16-byte LDS accesses."""
    from scream_amd import build
    asm = str(tmp_path / "backward.s")
    r = subprocess.run([build._hipcc(), "-O3", "-std=c++17", "--offload-arch=" + build.ARCH, "-S", "--cuda-device-only",
                        os.path.join(build.CSRC, "backward.hip"), "-o", asm], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = open(asm).read().splitlines()
    begin = [i for i, l in enumerate(lines) if "wgrad_split_partial_kernel" in l and l.rstrip().endswith(":") or
             ("wgrad_split_partial_kernel" in l and l.startswith("_Z") and ":" in l)]
    assert begin, "kernel not found in the assembly"
    end = next(i for i in range(begin[0], len(lines)) if "s_endpgm" in lines[i])
    body = [l.split(";")[0] for l in lines[begin[0]:end]]
    assert sum("v_mfma_f32_32x32x16_bf16" in l for l in body) == 48  # 2 steps x 4 tile pairs x 6 products per chunk
    assert not any("scratch_" in l for l in body)
    assert not any(l.strip().startswith("s_") and "store" in l for l in body)
    assert any("ds_read_b128" in l or "ds_load_b128" in l for l in body) and any("ds_write_b128" in l or "ds_store_b128" in l for l in body)
    meta = "\n".join(lines)
    sym = lines[begin[0]].split(":")[0]
    assert ("%s.private_seg_size, 0" % sym) in meta or ".private_segment_fixed_size: 0" in meta
