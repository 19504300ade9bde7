"""The rides of the ring projection (csrc/proj_ring.hip): every epilogue piece stands behind a matrix instruction of the next
stage, by hand.  Where a piece stands must not change one bit, so the smallest launches in which every ride variant and every
hand-over between two rides occurs are held to what test_ring_projection_vs_oracle_and_vs_the_eight_wave_gemm
(tests/test_gpu_parity.py) asks, with its thresholds: Q' bit for bit the 8-wave GEMM's (up to its other internal order of the
same products: 2e-6), K^T V and Ksum per cloud against that GEMM and against the float64 oracle.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import scream_ref as O
from scream_amd import ops, scales
from scream_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# clouds of 100, 129 and 256 rows in 128 + 256 + 256 packed rows: five 128-row tiles, so the last 256-row tile has two idle waves;
# cloud 0 ends in a masked tile (its second wave holds 36 rows), cloud 1 in a tile of one row (its second wave is all padding)
LENS, ROW0, ROWS = [100, 129, 256], [0, 128, 384], 640
TILE_CLOUD = [0, 1, 1, 2, 2]


def dev(x):
    return torch.as_tensor(x).to(DEV)


@pytest.fixture(scope="module")
def case():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from scream_amd import _lib
    _lib.load()
    sd = make_state_dict(9, 256, 1, 1)
    rng = np.random.default_rng(5)
    xs = [torch.from_numpy(rng.normal(size=(n, 256)).astype(np.float32)) for n in LENS]
    x = torch.zeros(ROWS, 256)
    for r0, xc in zip(ROW0, xs):
        x[r0:r0 + xc.shape[0]] = xc
    x[100:128] = 3.0  # garbage in padding rows must not reach the reduction
    x[128 + 129:384] = -2.5
    q, k, v = (sd["stem.0.%s_proj.weight" % n] for n in "qkv")
    W = torch.cat([q, k[:128], v[:128], k[128:], v[128:]], dim=0)
    want = []
    for xc in xs:
        w = {}
        O.mh_attention(xc[None], xc[None], xc[None], sd, "stem.0.", w)
        want.append(w)
    c = dict(xs=xs, W=W, want=want, xf=ops.act_layout(dev(x), True), a_exp=scales.exp_for(float(x.abs().max())),
             tile_cloud=dev(torch.tensor(TILE_CLOUD, dtype=torch.int32)), crow0=dev(torch.tensor(ROW0, dtype=torch.int32)),
             clen=dev(torch.tensor(LENS, dtype=torch.int32)))
    return c


def _exps(P, n_q):
    rl = P.row_l1[n_q:].view(-1, 2, 128)
    return scales.exp_for(1.0 + 6.0 * float(rl[:, 0].max())), scales.exp_for(6.0 * float(rl[:, 1].max()))


def _vs_oracle(kv, want):
    kvt = kv[:, :1024].reshape(8, 32, 32)  # [h][v][d]
    torch.testing.assert_close(kvt.permute(0, 2, 1), want["KV"][0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(kv[:, 1024:], want["Ksum"][0], rtol=1e-5, atol=1e-4)


def _with_queries(c, xf, tile_cloud, crow0, clen, clouds):
    """N = 768, n_q = 256: query -> key -> value -> the next tile's query rides, store_kv behind a query stage."""
    W, n = c["W"], len(clouds)
    w_exp = scales.w_exp(W)
    P = ops.pack_proj(dev(W), 256, ops.SPLIT_H2, w_exp)
    k_exp, v_exp = _exps(P, 256)
    kw = dict(a_exp=c["a_exp"], k_exp=k_exp, v_exp=v_exp)
    Qf, part = ops.proj_qkv(xf, P, tile_cloud, crow0, clen, 0, **kw)
    Qf2, part2 = ops.proj_qkv(xf, P, tile_cloud, crow0, clen, 0, **kw)
    assert torch.equal(Qf2, Qf) and torch.equal(part2, part)  # twice, bit for bit
    Qg, partg = ops.gemm_qkv(xf, ops.pack_w(dev(W), ops.SPLIT_H2, w_exp), 256, tile_cloud, crow0, clen, 0,
                             layout=ops.LAYOUT_A_FRAG | ops.LAYOUT_C_FRAG, **kw)
    Q, Qg = ops.act_layout(Qf, False).cpu(), ops.act_layout(Qg, False).cpu()
    kv = ops.kv_finalize(part, crow0, clen, 0, 0, n, n).cpu()
    kvg = ops.kv_finalize(partg, crow0, clen, 0, 0, n, n).cpu()
    for ci, cloud in enumerate(clouds):
        r0, m = int(crow0[ci]), LENS[cloud]
        assert torch.equal(Q[r0:r0 + m], Qg[r0:r0 + m]) or (Q[r0:r0 + m] - Qg[r0:r0 + m]).abs().max() < 2e-6
        torch.testing.assert_close(kv[ci], kvg[ci], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(Q[r0:r0 + m].reshape(m, 8, 32), c["want"][cloud]["Q"][0], rtol=1e-5, atol=1e-5)
        _vs_oracle(kv[ci], c["want"][cloud])


def _keys_and_values_only(c, xf, tile_cloud, crow0, clen, clouds):
    """N = 1024, n_q = 0, two layers: value -> key rides with store_kv, and the pipeline's end in the open."""
    W, n = c["W"], len(clouds)
    Wkv = torch.cat([W[256:], 2.0 * W[256:].flip(0)])
    w_exp = scales.w_exp(Wkv)
    P = ops.pack_proj(dev(Wkv), 0, ops.SPLIT_H2, w_exp)
    k_exp, v_exp = _exps(P, 0)
    kw = dict(a_exp=c["a_exp"], k_exp=k_exp, v_exp=v_exp)
    _, part = ops.proj_qkv(xf, P, tile_cloud, crow0, clen, 0, **kw)
    _, part2 = ops.proj_qkv(xf, P, tile_cloud, crow0, clen, 0, **kw)
    assert torch.equal(part2, part)
    _, partg = ops.gemm_qkv(xf, ops.pack_w(dev(Wkv), ops.SPLIT_H2, w_exp), 0, tile_cloud, crow0, clen, 0, layout=ops.LAYOUT_A_FRAG, **kw)
    assert part.shape == partg.shape == (2, xf.shape[0] // 128, 8, 1056)
    for l in range(2):
        a = ops.kv_finalize(part[l], crow0, clen, 0, 0, n, n).cpu()
        b = ops.kv_finalize(partg[l], crow0, clen, 0, 0, n, n).cpu()
        torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-5)
        if l == 0:  # layer 0 carries the stem's own key / value weights
            for ci, cloud in enumerate(clouds):
                _vs_oracle(a[ci], c["want"][cloud])


def test_rides_with_queries_on_five_tiles(case):
    _with_queries(case, case["xf"], case["tile_cloud"], case["crow0"], case["clen"], [0, 1, 2])


def test_rides_of_two_key_value_layers_on_five_tiles(case):
    _keys_and_values_only(case, case["xf"], case["tile_cloud"], case["crow0"], case["clen"], [0, 1, 2])


@pytest.mark.parametrize("form", ["qkv", "kv"])
def test_rides_on_a_single_tile(case, form):
    """M = 128: one tile, fewer units than blocks, two idle waves, a masked second wave."""
    xf = case["xf"][:128].contiguous()
    tc, cr, cl = (dev(torch.tensor(v, dtype=torch.int32)) for v in ([0], [0], [LENS[0]]))
    (_with_queries if form == "qkv" else _keys_and_values_only)(case, xf, tc, cr, cl, [0])
