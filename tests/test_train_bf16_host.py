"""train_backend = "bf16" where no GPU is needed: the yardstick's rounding (tests/bf16_ref.py) against the bit pattern, the
host-side argument checks of the three entry points of csrc/gemm_bf16.hip, the ways the backend is selected, and the
yardstick held to its own rule: two fp32 realisations of the restated arithmetic that differ in accumulation order alone stay
within a factor 2 of each other against the float64 restatement, per tensor -- the ratio the GPU tests grant the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_ref as B
import train_ref as T
from scream_amd import _lib
from scream_amd.model import DEMTransformer, PointTransformer
from scream_amd.synthetic import make_state_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


# ------------------------------------------------------------------------------------- r
def test_r_is_round_to_nearest_even_of_the_bit_pattern():
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.standard_normal(200000) * np.exp2(rng.integers(-40, 40, 200000))).astype(np.float32))
    assert torch.equal(B.r(x), B.r_bits(x))
    # exact ties: 1 + (2 k + 1) 2^-8 lies halfway between the bf16 neighbours 1 + 2 k 2^-7 and 1 + (2 k + 2) 2^-7
    k = torch.arange(0, 64, dtype=torch.float32)
    ties = torch.cat([1 + (2 * k + 1) * 2.0 ** -8, -(1 + (2 * k + 1) * 2.0 ** -8), (1 + (2 * k + 1) * 2.0 ** -8) * 2.0 ** -100])
    got = B.r(ties)
    assert torch.equal(got, B.r_bits(ties))
    down, up = 1 + 2 * k * 2.0 ** -8, 1 + (2 * k + 2) * 2.0 ** -8  # the neighbours; the EVEN one has an even 7-bit mantissa
    even = torch.where((k % 2) == 0, down, up)
    assert torch.equal(got[:64], even) and torch.equal(got[64:128], -even) and torch.equal(got[128:], even * 2.0 ** -100)
    # values of bf16 pass unchanged, float64 goes through fp32
    assert torch.equal(B.r(got), got)
    assert torch.equal(B.r(x.double()), B.r(x).double())
    # one ulp of fp32 either side of a tie goes to its side
    t = ties[:64]
    assert torch.equal(B.r(torch.nextafter(t, torch.tensor(0.0))), down) and torch.equal(B.r(torch.nextafter(t, torch.tensor(4.0))), up)


def test_rounded_product_is_what_it_says():
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((1, 70, 128))).requires_grad_()
    W = torch.from_numpy(rng.standard_normal((64, 128))).requires_grad_()
    small = torch.from_numpy(rng.standard_normal((3, 128)))
    dy = torch.from_numpy(rng.standard_normal((1, 70, 64)))
    with B.rounded_gemms() as mode:
        y = x @ W.t()
        exact = x @ small.t()  # N = 3: not a training GEMM
        y.backward(dy)
    assert mode.routed == 1
    assert torch.equal(exact, x.detach() @ small.t())
    assert torch.equal(y.detach(), B.r(x.detach()) @ B.r(W.detach()).t())
    assert torch.equal(x.grad, B.r(dy) @ B.r(W.detach()))
    assert torch.equal(W.grad, B.r(dy)[0].t() @ B.r(x.detach())[0])
    for order in ("natural", "reversed"):
        with B.rounded_gemms(order=order):
            y2 = x @ W.t()
        assert T.rel(y2, y) < 1e-14


# ------------------------------------------------------------------------------------- the entry points' host checks
def test_bf16_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.scream_abi_version() == 21
    p = 1 << 20  # never dereferenced: every call below fails before a launch
    fwd = lambda A=p, lda=256, W=p, C=p, ldc=256, M=128, N=256, K=256, epi=0, n_act=0, bias=None: \
        lib.scream_gemm_bf16_f32(A, lda, W, C, ldc, M, N, K, epi, n_act, bias, None)
    assert fwd(A=None) == EINVAL and fwd(W=None) == EINVAL and fwd(C=None) == EINVAL
    assert fwd(N=200) == EUNSUPPORTED and fwd(N=128) == EUNSUPPORTED and fwd(K=100, lda=100) == EUNSUPPORTED and fwd(K=32) == EUNSUPPORTED
    assert fwd(M=100) == EUNSUPPORTED and fwd(M=-128) == EUNSUPPORTED
    assert fwd(lda=128) == EINVAL and fwd(ldc=128) == EINVAL and fwd(lda=258) == EINVAL and fwd(A=p + 4) == EINVAL
    assert fwd(epi=3) == EINVAL  # bias + relu without a bias
    assert fwd(epi=1, n_act=100) == EUNSUPPORTED and fwd(epi=4) == EUNSUPPORTED and fwd(epi=9) == EINVAL
    dg = lambda dY=p, ldy=256, W=p, dX=p, ldx=256, M=128, N=256, K=256: lib.scream_gemm_dgrad_bf16_f32(dY, ldy, W, dX, ldx, M, N, K, None)
    assert dg(dY=None) == EINVAL and dg(W=None) == EINVAL and dg(dX=None) == EINVAL
    assert dg(K=200) == EUNSUPPORTED and dg(N=100, ldy=128) == EUNSUPPORTED and dg(M=64) == EUNSUPPORTED
    assert dg(N=768, ldy=512) == EINVAL and dg(K=512, ldx=256) == EINVAL and dg(dX=p + 8) == EINVAL
    # the weight gradient: the sizes and refusals of scream_gemm_wgrad_f32
    size = lib.scream_wgrad_bf16_workspace_bytes
    for shape in ((0, 256, 256), (1, 128, 128), (128, 256, 256), (330000, 256, 256), (300, 128, 128), (9000, 1024, 256)):
        assert size(*shape) == lib.scream_wgrad_workspace_bytes(*shape), shape
    assert size(128, 256, 256) == (256 * 256 + 256) * 4 and size(0, 256, 256) == 0
    for bad in ((-1, 256, 256), (128, 200, 256), (128, 256, 200), (128, 0, 256), (128, 256, 0)):
        assert size(*bad) == -1, bad
    ws = size(128, 256, 256)
    wg = lambda dY=p, ldy=256, X=p, ldx=256, rows=128, N=256, K=256, dW=p, w=p, wb=ws: \
        lib.scream_gemm_wgrad_bf16_f32(dY, ldy, X, ldx, rows, N, K, dW, 0, None, w, wb, None)
    assert wg(dY=None) == EINVAL and wg(X=None) == EINVAL and wg(dW=None) == EINVAL
    assert wg(N=200) == EUNSUPPORTED and wg(K=64) == EUNSUPPORTED and wg(rows=-1) == EUNSUPPORTED
    assert wg(ldy=128) == EINVAL and wg(ldx=254) == EINVAL
    assert wg(w=None, wb=0) == EINVAL and wg(wb=ws - 1) == EINVAL and wg(wb=16) == EINVAL and wg(w=p + 4) == EINVAL


# ------------------------------------------------------------------------------------- selecting the backend
def test_bf16_is_a_train_backend_by_attribute():
    assert PointTransformer.TRAIN_BACKENDS == ("f32", "split", "bf16") == DEMTransformer.TRAIN_BACKENDS
    for cls in (PointTransformer, DEMTransformer):
        net = cls(256, 1, 1)
        assert net.train_backend == "f32"
        net.train_backend = "bf16"
        assert net.train_backend == "bf16" and cls(256, 1, 1).train_backend == "f32"
        for bad in ("h1", "h2", "fp16", None):
            with pytest.raises(ValueError, match="'f32', 'split', 'bf16'"):
                net.train_backend = bad
        assert net.train_backend == "bf16"
        assert net.train() is net and net._trains()


def test_bf16_is_a_train_backend_by_environment():
    env = dict(os.environ, SCREAM_TRAIN_GEMM="bf16", PYTHONPATH=REPO)
    code = ("from scream_amd.model import PointTransformer, DEMTransformer\n"
            "n = PointTransformer(256, 1, 1)\n"
            "assert n.train_backend == 'bf16' and DEMTransformer(256, 1, 1).train_backend == 'bf16'\n"
            "n.train()\n")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr


@pytest.mark.parametrize("driver", ["train_3d_match", "train_kitti", "train_open_gf"])
def test_the_drivers_take_the_backend(driver, monkeypatch):
    mod = __import__(driver)
    seen = []
    monkeypatch.setattr(mod, "train", lambda *a, **k: seen.append(a))
    mod.main(["--train-backend", "bf16", "--synthetic", "2"])
    assert seen and seen[0][2] == "bf16"
    with pytest.raises(SystemExit):
        mod.main(["--train-backend", "fp16"])


def test_train_wrappers_dispatch_the_bf16_arm_without_a_gpu(monkeypatch):
    """train.gemms(backend) is the one dispatch point, and what forward_saving takes for a model with that train_backend; a
    weight gradient whose N the library refuses raises from the bf16 sizer."""
    from scream_amd import train
    net = PointTransformer(256, 1, 1)
    taken, plain = [], train.gemms

    class Taken(Exception):
        pass

    def recording(backend):  # forward_saving chooses its arithmetic first: stop it there, before it needs a batch
        taken.append(plain(backend))
        raise Taken

    for backend in ("f32", "split", "bf16"):
        net.train_backend = backend
        monkeypatch.setattr(train, "gemms", recording)
        with pytest.raises(Taken):
            train.forward_saving(net, None)
        monkeypatch.setattr(train, "gemms", plain)
        for mm in (train.gemms(backend), taken.pop()):
            assert type(mm) is train.ARITHMETICS[backend] and mm.name == backend
    assert not taken
    with pytest.raises(_lib.ScreamHipError, match=r"scream_wgrad_bf16_workspace_bytes\(300, 200, 256\)"):
        train.wgrad_bf16(torch.zeros(300, 200), torch.zeros(300, 256), None)


# ------------------------------------------------------------------------------------- the yardstick against itself
@pytest.mark.parametrize("ns,nc,n,m", [(1, 1, 300, 280), (2, 2, 129, 127)])
def test_the_restatement_meets_its_own_rule(ns, nc, n, m):
    """Float64 restatement against two fp32 restatements (contraction in natural / reversed 64-wide chunks) under ONE set of
    masks.  What is left between any two of them is fp32 accumulation order and the roundings it flips (an operand within fp32
    rounding of a bf16 tie goes the other way and moves by a bf16 ulp).  Per tensor the two fp32 errors stay within a factor 2
    of each other: the ratio the GPU is held to is one the reference meets against itself.  Measured: errors 5e-4 .. 1.6e-3,
    largest ratio 1.19."""
    sd = make_state_dict(40 + ns, 256, ns, nc)
    pair = T.make_pair(40 + ns, n, m)
    masks = {}
    with B.rounded_gemms() as mode:
        T.oracle_grads(sd, *pair, torch.float64, record=masks)
        g64 = T.oracle_grads(sd, *pair, torch.float64, masks=masks)[1]
    assert mode.routed >= 2 * 6 * (ns + nc)  # two passes, at least six products per layer
    g32 = {}
    for order in ("natural", "reversed"):
        with B.rounded_gemms(order=order):
            g32[order] = T.oracle_grads(sd, *pair, torch.float32, masks=masks)[1]
    g64x = T.oracle_grads(sd, *pair, torch.float64, masks=masks)[1]  # unrounded, same masks
    worst = 0.0
    for k in g64:
        a, b = T.rel(g32["natural"][k], g64[k]), T.rel(g32["reversed"][k], g64[k])
        ratio = max(a, b) / max(min(a, b), T.FLOOR)
        worst = max(worst, ratio)
        assert ratio < 2, (k, a, b)
    far = [T.rel(g64[k], g64x[k]) for k in g64]
    print("(%d,%d): largest ratio between the two fp32 restatements %.3f; restatement against the unrounded float64 oracle %.2g .. %.2g"
          % (ns, nc, worst, min(far), max(far)))
    assert max(far) > 1e-4  # the restatement IS another arithmetic than the oracle's
