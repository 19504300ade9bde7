"""The split that is named is the split that runs: every entry point that goes from the runtime `split` to a kernel instantiation
(split.h: with_split), at its smallest launches.  The pack kernels write into images with a guard behind them; the GEMM, the ring
projection and the layer tail run h1 / h2 / x3 on one seeded input, where the fp32-accurate splits meet the tolerances the suite
already holds them to, the single-plane split does not, and no two give the same bytes.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import scream_ref as O
from scream_amd import _lib, ops, scales
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLITS = {"h1": ops.SPLIT_H1, "h2": ops.SPLIT_H2, "x3": ops.SPLIT_BF3}
EPILOGUES = {"none": ops.EPI_NONE, "elu1": ops.EPI_ELU1, "relu": ops.EPI_RELU, "bias_relu": ops.EPI_BIAS_RELU, "res_ln": ops.EPI_RES_LN}
PATTERN = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def dev(x):
    return torch.as_tensor(x).to(DEV)


# ------------------------------------------------------------------------------------- pack kernels, behind a guard
def pack_images():
    """name -> (buffer, image bytes): each pack kernel's image for every split its entry point takes, written at the front of a
    buffer as long as the LARGEST image any instantiation of that kernel writes and filled with PATTERN -- another instantiation
    than the one named shows in the guard (or in planes left unwritten), never as a store out of bounds."""
    lib, g = _lib.load(), torch.Generator().manual_seed(41)
    out = {}

    def run(name, nbytes, room, call):
        assert 0 < nbytes <= room, (name, nbytes, room)
        buf = torch.full((room + 4096,), PATTERN, dtype=torch.uint8, device=DEV)
        ops.check(call(ops._p(buf, torch.uint8)), name)
        out[name] = (buf.cpu(), nbytes)

    W = dev(torch.randn(256, 64, generator=g))
    for s, split in SPLITS.items():
        run("pack_w/" + s, split * 256 * 64 * 2, 3 * 256 * 64 * 2,
            lambda p: lib.scream_pack_w_split(ops._p(W), 256, 64, split, scales.w_exp(W) if split != ops.SPLIT_BF3 else 0, p, ops._stream()))
    for N, n_q in ((768, 256), (1024, 0)):
        Wp = dev(torch.randn(N, 256, generator=g) / 16)
        for s in ("h1", "h2"):
            run("pack_proj/%d/%s" % (N, s), lib.scream_proj_image_bytes(N, SPLITS[s]), 3 * lib.scream_proj_image_bytes(N, ops.SPLIT_H1),
                lambda p: lib.scream_pack_proj(ops._p(Wp), N, n_q, SPLITS[s], scales.w_exp(Wp), p, ops._stream()))
    Wm, W1, W2, Wq = (dev(torch.randn(n, k, generator=g) / k ** 0.5) for n, k in ((256, 256), (1024, 256), (256, 1024), (256, 256)))
    ex = ops.tail_exps(e_wm=scales.w_exp(Wm), e_w1=scales.w_exp(W1), e_w2=scales.w_exp(W2), e_wq=scales.w_exp(Wq))
    room = 3 * lib.scream_tail_image_bytes(ops.SPLIT_H1, 1)  # three planes of every stage, the next layer's query stages included
    for s, split in SPLITS.items():
        for nq in ((0, 1) if split != ops.SPLIT_BF3 else (0,)):
            run("pack_tail/%s%s" % (s, "/next_q" if nq else ""), lib.scream_tail_image_bytes(split, nq), room,
                lambda p: lib.scream_pack_tail(ops._p(Wm), ops._p(W1), ops._p(W2), ops._p(Wq) if nq else None, split, C.byref(ex), p, ops._stream()))
    torch.cuda.synchronize()
    return out


def test_pack_kernels_write_their_image_and_nothing_behind_it():
    images = pack_images()
    assert len(images) == 3 + 4 + 5
    for name, (buf, nbytes) in images.items():
        assert bool((buf[nbytes:] == PATTERN).all()), "%s: the guard behind the image was written" % name
        vectors = buf[:nbytes].view(-1, 16)  # every plane in full: no 16-byte vector of the image is still the pattern
        assert not bool((vectors == PATTERN).all(dim=1).any()), "%s: part of the image was not written" % name


# ------------------------------------------------------------------------------------- gemm_split
def gemm_outputs():
    """(split, epilogue) -> C on the CPU, and epilogue -> the float64 result: M = 128, N = 256, K = 64, one seeded input."""
    g = torch.Generator().manual_seed(7)
    M, N, K = 128, 256, 64
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    ref = A.double() @ W.double().t()
    want = {"none": ref, "elu1": torch.nn.functional.elu(ref) + 1, "relu": ref.clamp_min(0), "bias_relu": (ref + bias.double()).clamp_min(0),
            "res_ln": torch.nn.functional.layer_norm(ref + res.double(), (N,), gamma.double(), beta.double(), 1e-5)}
    kw = {"none": {}, "elu1": dict(n_act=N), "relu": {}, "bias_relu": dict(bias=dev(bias)),
          "res_ln": dict(residual=dev(res), gamma=dev(gamma), beta=dev(beta))}
    got = {}
    for s, split in SPLITS.items():
        Wp = ops.pack_w(dev(W), split)
        for e, epi in EPILOGUES.items():
            got[s, e] = ops.gemm_split(dev(A), Wp, epi, **kw[e]).cpu()
    return got, want


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _close(a, b, rtol, atol):
    return bool(torch.isclose(a.double(), b.double(), rtol=rtol, atol=atol).all())


def test_gemm_split_runs_the_split_it_is_given_under_every_epilogue():
    got, want = gemm_outputs()
    tol = dict(rtol=1e-5, atol=2e-5)  # test_gemm_plain_and_activations, test_gemm_residual_layernorm
    for e in EPILOGUES:
        h1, h2, x3 = (got[s, e] for s in ("h1", "h2", "x3"))
        assert not _same_bytes(h1, h2) and not _same_bytes(h1, x3) and not _same_bytes(h2, x3), e
        torch.testing.assert_close(h2.double(), want[e], **tol)
        torch.testing.assert_close(x3.double(), want[e], **tol)
        assert not _close(h1, want[e], **tol), "%s: one fp16 plane cannot be this close to float64" % e


# ------------------------------------------------------------------------------------- proj_qkv, layer_tail
def _one_cloud():
    """One 128-row tile holding one cloud of 100 rows (garbage in the padding rows), a block's weights, its float64-free oracle."""
    sd, pre = make_state_dict(21, 256, 1, 1), "stem.0."
    rng = np.random.default_rng(11)
    xc = torch.from_numpy(rng.normal(size=(100, 256)).astype(np.float32))
    x = torch.full((128, 256), 3.0)
    x[:100] = xc
    q, k, v = (sd[pre + "%s_proj.weight" % n] for n in "qkv")
    W = torch.cat([q, k[:128], v[:128], k[128:], v[128:]], dim=0)
    tc, cr, cl = (dev(torch.tensor([n], dtype=torch.int32)) for n in (0, 0, 100))
    return sd, pre, xc, x, q, v, W, tc, cr, cl


def proj_outputs():
    """split -> (Q' row-major, K^T V | Ksum of the cloud) of the ring projection and of the eight-wave GEMM, same operands and
    exponents for both splits."""
    sd, pre, xc, x, q, v, W, tc, cr, cl = _one_cloud()
    xf = ops.act_layout(dev(x), True)
    w_exp = scales.w_exp(W)
    rl = W.abs().sum(dim=1)[256:].view(-1, 2, 128)
    kw = dict(a_exp=scales.exp_for(float(x.abs().max())), k_exp=scales.exp_for(1.0 + 6.0 * float(rl[:, 0].max())),
              v_exp=scales.exp_for(6.0 * float(rl[:, 1].max())))
    ring, gemm = {}, {}
    for s in ("h1", "h2"):
        Q, part = ops.proj_qkv(xf, ops.pack_proj(dev(W), 256, SPLITS[s], w_exp), tc, cr, cl, 0, **kw)
        ring[s] = (ops.act_layout(Q, False).cpu()[:100], ops.kv_finalize(part, cr, cl, 0, 0, 1, 1).cpu())
        Q, part = ops.gemm_qkv(xf, ops.pack_w(dev(W), SPLITS[s], w_exp), 256, tc, cr, cl, 0, layout=ops.LAYOUT_A_FRAG | ops.LAYOUT_C_FRAG, **kw)
        gemm[s] = (ops.act_layout(Q, False).cpu()[:100], ops.kv_finalize(part, cr, cl, 0, 0, 1, 1).cpu())
    return ring, gemm


def test_ring_projection_runs_the_split_it_is_given():
    ring, gemm = proj_outputs()
    for s in ("h1", "h2"):  # against the eight-wave GEMM of the same split: test_ring_projection_vs_oracle_and_vs_the_eight_wave_gemm
        (Q, kv), (Qg, kvg) = ring[s], gemm[s]
        assert torch.equal(Q, Qg) or s == "h2" and (Q - Qg).abs().max() < 2e-6
        torch.testing.assert_close(kv, kvg, rtol=2e-5, atol=2e-5)
    assert not _same_bytes(ring["h1"][0], ring["h2"][0]) and not _same_bytes(ring["h1"][1], ring["h2"][1])
    assert not (ring["h1"][0] - gemm["h2"][0]).abs().max() < 2e-6  # one plane is not two
    assert not _close(ring["h1"][1], gemm["h2"][1], rtol=2e-5, atol=2e-5)


def tail_outputs():
    """name -> y (row-major, the cloud's rows) of the layer tail on h2, h2 with the next layer's query projection, h1 and x3 -- and
    that projection, with the GEMM it must equal; `want`: the oracle block.  The fp16 tails read the SAME Q' and K^T V image (the
    h2 GEMM's), so only the tail's own split tells them apart."""
    sd, pre, xc, x, q, v, W, tc, cr, cl = _one_cloud()
    xf = ops.act_layout(dev(x), True)
    FR = ops.LAYOUT_A_FRAG | ops.LAYOUT_C_FRAG
    exd = scales.tail_exps(sd[pre + "merge.weight"], sd[pre + "mlp.0.weight"], sd[pre + "mlp.2.weight"], sd[pre + "norm1.weight"],
                           sd[pre + "norm1.bias"], float((x @ v.t()).abs().max()) * 1.01, float((x @ q.t()).abs().max()) * 1.01)
    mats = [dev(sd[pre + n]) for n in ("merge.weight", "mlp.0.weight", "mlp.2.weight")]
    norms = [dev(sd[pre + n]) for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")]
    out, src = {}, {}
    for s in ("h2", "x3"):
        Q, part = ops.gemm_qkv(xf, ops.pack_w(dev(W), SPLITS[s]), 256, tc, cr, cl, 0, FR)
        src[s] = (Q, ops.kv_finalize_image(part, cr, cl, 0, 0, 1, 1, split=SPLITS[s]))
    src["h1"] = src["h2"]
    for s in ("h2", "h1", "x3"):
        img = ops.pack_tail(*mats, SPLITS[s], ops.tail_exps(**exd))
        out[s] = ops.layer_tail(src[s][0], src[s][1], tc, 0, cl, xf, img, *norms)
    Wq_next = sd["cross.1.layer.q_proj.weight"]
    e_y, e_wq = scales.exp_for(scales.ln_bound(sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])), scales.w_exp(Wq_next)
    img = ops.pack_tail(*mats, ops.SPLIT_H2, ops.tail_exps(e_y=e_y, e_wq=e_wq, **exd), Wq_next=dev(Wq_next))
    q_next = torch.full_like(xf, float("nan"))
    out["h2/next_q"] = ops.layer_tail(src["h2"][0], src["h2"][1], tc, 0, cl, xf, img, *norms, q_next=q_next)
    q_want = ops.gemm_split(out["h2"], ops.pack_w(dev(Wq_next), ops.SPLIT_H2, e_wq), ops.EPI_ELU1, n_act=256, layout=FR, a_exp=e_y)
    out = {k: ops.act_layout(t, False).cpu()[:100] for k, t in out.items()}
    out["q_next"], out["q_next/gemm"] = ops.act_layout(q_next, False).cpu()[:100], ops.act_layout(q_want, False).cpu()[:100]
    return out, O.mh_attention(xc[None], xc[None], xc[None], sd, pre)[0]


def test_layer_tail_runs_the_split_and_the_variant_it_is_given():
    out, want = tail_outputs()
    tol = dict(rtol=2e-4, atol=5e-5)  # test_fused_layer_tail_vs_oracle_block
    h2, h1, x3 = out["h2"], out["h1"], out["x3"]
    assert not _same_bytes(h1, h2) and not _same_bytes(h1, x3) and not _same_bytes(h2, x3)
    torch.testing.assert_close(h2, want, **tol)
    torch.testing.assert_close(x3, want, **tol)
    assert not _close(h1, want, **tol), "one fp16 plane cannot be this close to the oracle"
    # test_layer_tail_with_the_next_layers_query_projection: the same y bit for bit, and Q'_next is the projection GEMM of it
    assert torch.equal(out["h2/next_q"], h2)
    torch.testing.assert_close(out["q_next"], out["q_next/gemm"], rtol=2e-6, atol=2e-6)
