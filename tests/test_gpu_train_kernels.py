"""The backward entry points of include/scream_hip.h ("Training") one by one against float64, at the shapes, options and edges
the training step drives them with (scream_amd/train.py): optional pointers NULL and set, accumulate on and off, one row, a
partial block, 300 000 rows, leading dimensions wider than the matrix, padded rows; then the data gradients of train.gemms()
on both arithmetics and one block (train._block_fwd + train._block_bwd) end to end.

Bars: an elementwise kernel equals the fp32 expression bit for bit; a reduction is held to <= max(2 x the error of the same
expression in fp32 on the CPU, 5e-6) against float64 (the rule of test_gpu_train.py::test_wgrad_against_float64).  Every test
prints its figures before it asserts.  Needs an MI355X: run with `pytest -m gpu`."""

import numpy as np
import pytest
import torch

import train_ref as T
from oracle import scream_ref as O
from scream_amd import _lib, ops, train
from scream_amd._lib import check
from scream_amd.ops import _p, _stream
from scream_amd.packing import PackedBatch
from scream_amd.synthetic import make_state_dict
from train_ref import FLOOR, packed_rows, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def held(what, got, want64, cpu32):
    """got (GPU) against want64 within max(2 x the fp32 CPU expression's error, FLOOR)."""
    e, e32 = rel(got, want64), rel(cpu32, want64)
    print("%s: error %.3g, the fp32 CPU expression %.3g" % (what, e, e32))
    assert e <= max(2 * e32, FLOOR), (what, e, e32)


def ragged_batch(src_len, tgt_len, rng=None, centers=None):
    """A PackedBatch with random coordinates on the real rows (zeros on padded rows) and the given centres [2B,3]."""
    B = len(src_len)
    lens, row0, rs, rt, tile_cloud, max_chunks = PackedBatch.layout(src_len, tgt_len)
    xyz = torch.zeros(rt, 3)
    if rng is not None:
        for i in range(2 * B):
            xyz[row0[i]:row0[i] + lens[i]] = torch.from_numpy(rng.uniform(-1, 1, size=(int(lens[i]), 3)).astype(np.float32))
    center = torch.zeros(2 * B, 3) if centers is None else centers
    return PackedBatch(B, list(src_len), list(tgt_len), row0, lens, rs, rt, max_chunks, xyz.to(DEV), center.to(DEV),
                       torch.from_numpy(tile_cloud).to(DEV), torch.from_numpy(row0).to(DEV), torch.from_numpy(lens).to(DEV))


def real_rows(batch):
    on = torch.zeros(batch.rows_total, dtype=torch.bool)
    for r0, n in zip(batch.cloud_row0_host, batch.cloud_len_host):
        on[int(r0):int(r0) + int(n)] = True
    return on


# ------------------------------------------------------------------------------------- elementwise: exact
# 20 000 x 1024 is the FFN hidden layer of a 20 k-row batch: 5.12 M float4, above the launch's 4096 blocks x 256 threads, so the
# grid-stride loop runs five times; n = 4 is one float4.
@pytest.mark.parametrize("shape", [(20000, 1024), (4,)])
def test_relu_bwd_is_the_mask_of_its_output(shape):
    rng = np.random.default_rng(101)
    y = torch.relu(randn(rng, *shape))  # a relu output: about half exact zeros
    dy = randn(rng, *shape)
    flat_y, flat_dy = y.view(-1), dy.view(-1)
    flat_y[1], flat_dy[1] = -0.0, -2.5  # y == -0.0 with a negative gradient: masked
    flat_y[2], flat_dy[2] = 0.0, -1.5  # y == +0.0
    flat_y[3], flat_dy[3] = 2e-38, -3.0  # a positive output near the smallest normal number stays on
    assert torch.isfinite(dy).all() and (flat_y[:3] <= 0).any()
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    got = dy.to(DEV)
    train.relu_bwd(got, y.to(DEV))
    assert torch.equal(got.cpu(), want)
    assert float(got.view(-1)[1]) == 0 and float(got.view(-1)[2]) == 0 and float(got.view(-1)[3]) == -3.0


@pytest.mark.parametrize("shape", [(20000, 1024), (4,)])
def test_add_is_the_fp32_sum(shape):
    rng = np.random.default_rng(102)
    y, x = randn(rng, *shape), randn(rng, *shape) * 1e-3
    got = y.to(DEV)
    train.add_(got, x.to(DEV))
    assert torch.equal(got.cpu(), y + x)


# every weight shape of a block (q|k|v 768 x 256, k|v 512 x 256, merge 256 x 256, FFN 1024 x 256 and 256 x 1024), and R, C
# that are not multiples of the 32 x 32 tile
@pytest.mark.parametrize("R,C", [(256, 256), (1024, 256), (256, 1024), (768, 256), (512, 256), (3, 256), (33, 65), (1, 1)])
def test_transpose_is_exact(R, C):
    W = randn(np.random.default_rng(103), R, C)
    got = train.transpose(W.to(DEV))
    assert got.shape == (C, R) and torch.equal(got.cpu(), W.t().contiguous())


# ------------------------------------------------------------------------------------- the head's data gradient
# 1 and 4: one block, partly and fully used; 700: a partial last block; 9000: above 2048 blocks x 4 rows, the grid-stride loop
@pytest.mark.parametrize("rows", [1, 4, 700, 9000])
def test_coor_head_bwd_against_float64(rows):
    rng = np.random.default_rng(104 + rows)
    dout, W = randn(rng, rows, 3), randn(rng, 3, 256) / 16
    H = torch.relu(randn(rng, rows, 256))
    assert (H == 0).any() and (H > 0).any()
    want = (dout.double() @ W.double()) * (H > 0)
    cpu32 = (dout @ W) * (H > 0)
    dH = torch.full((rows, 256), 7.0, device=DEV)
    dout_d, W_d, H_d = dout.to(DEV), W.to(DEV), H.to(DEV)  # named: the launch reads them after this line has run
    check(_lib.load().scream_coor_head_bwd(_p(dout_d), _p(W_d), _p(H_d), _p(dH), rows, _stream()), "scream_coor_head_bwd")
    assert (dH.cpu()[H == 0] == 0).all()
    held("coor_head_bwd rows %d" % rows, dH, want, cpu32)


# ------------------------------------------------------------------------------------- the 3-wide weight gradients
def grad3(w, s, dW, transpose_w, col_w=None, col_s=None, center=None, tile_cloud=None, accumulate=False):
    lib, rows = _lib.load(), w.shape[0]
    ws = ops._workspace("scream_grad3_workspace_bytes", rows, device=w.device)
    check(lib.scream_grad3(_p(w), _p(s), _p(center), _p(tile_cloud, torch.int32), rows, _p(dW), int(transpose_w), _p(col_w),
                           _p(col_s), int(accumulate), ws.data_ptr(), ws.numel(), _stream()), "scream_grad3")


# rows 1; 700: one full block of 512 and a partial one; 300 000: 586 partials for the reduce launch
@pytest.mark.parametrize("rows", [1, 700, 300000])
@pytest.mark.parametrize("transpose_w", [False, True])
def test_grad3_plain_against_float64(rows, transpose_w):
    """The coor_mlp.4 call (transpose_w = 0, col_s) and every other combination of col_w / col_s NULL and set, accumulate off
    and on, without a centre."""
    rng = np.random.default_rng(110 + rows % 97)
    w, s = randn(rng, rows, 256), randn(rng, rows, 3)
    want = s.double().t() @ w.double()  # [3,256]
    cpu32 = s.t() @ w
    shape = (256, 3) if transpose_w else (3, 256)
    lay = (lambda p: p.t()) if transpose_w else (lambda p: p)
    wd, sd_ = w.to(DEV), s.to(DEV)
    for use_w, use_s in ((False, False), (True, False), (False, True), (True, True)):
        dW = torch.full(shape, 7.0, device=DEV)
        cw = torch.full((256,), 7.0, device=DEV) if use_w else None
        cs = torch.full((3,), 7.0, device=DEV) if use_s else None
        grad3(wd, sd_, dW, transpose_w, cw, cs)
        what = "grad3 rows %d transpose_w %d col_w %d col_s %d" % (rows, transpose_w, use_w, use_s)
        held(what, dW, lay(want), lay(cpu32))
        if use_w:
            held(what + " col_w", cw, w.double().sum(0), w.sum(0))
        if use_s:
            held(what + " col_s", cs, s.double().sum(0), s.sum(0))
        first = [t.clone() for t in (dW, cw, cs) if t is not None]
        dW2 = torch.full(shape, 7.0, device=DEV)
        cw2, cs2 = (None if t is None else torch.full_like(t, 7.0) for t in (cw, cs))
        grad3(wd, sd_, dW2, transpose_w, cw2, cs2)
        assert all(torch.equal(a, b) for a, b in zip(first, [t for t in (dW2, cw2, cs2) if t is not None])), what + ": two calls differ"
        grad3(wd, sd_, dW, transpose_w, cw, cs, accumulate=True)  # on top of the first call
        held(what + " accumulated", dW, 2 * lay(want), 2 * lay(cpu32))
        if use_w:
            held(what + " col_w accumulated", cw, 2 * w.double().sum(0), 2 * w.sum(0))
        if use_s:
            held(what + " col_s accumulated", cs, 2 * s.double().sum(0), 2 * s.sum(0))


@pytest.mark.parametrize("rows", [2000, 300000])
def test_grad3_column_sums_of_equal_terms_against_float64(rows):
    """coor_mlp.4.bias of a model whose prediction lies to one side of its target (DEMTransformer before training): col_s
    adds the L1 loss's gradient, the SAME number 1 / N on every row of a column (here: one column all +, one all -, one
    mixed).  A running fp32 sum of equal terms rounds the same way at every step: over 512 rows of 1 / 2000 it is off by
    5.3e-6 relative, and that kept coor_mlp.4.bias of the (6, 6) DEMTransformer at 5.31e-6 against a bar of 5e-6 (fp32 CPU
    oracle: 5.1e-8) until the kernel summed these three columns in double."""
    rng = np.random.default_rng(115)
    sign = np.stack([np.ones(rows), -np.ones(rows), rng.choice([-1.0, 1.0], size=rows)], 1).astype(np.float32)
    s = torch.from_numpy(sign) * (torch.tensor(1.0) / rows)
    w = randn(rng, rows, 256)
    wd, sdv = w.to(DEV), s.to(DEV)
    dW, cs = torch.full((3, 256), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
    grad3(wd, sdv, dW, False, None, cs)
    held("grad3 equal terms rows %d" % rows, dW, s.double().t() @ w.double(), s.t() @ w)
    held("grad3 equal terms rows %d col_s" % rows, cs, s.double().sum(0), s.sum(0))


def test_grad3_with_centres_on_a_ragged_batch_against_float64():
    """The embedding's call (train.backward): s = xyz - center[cloud of the row] with nonzero centres, transpose_w = 1, col_w;
    the gradient is zero on padded rows, where xyz - center is not."""
    rng = np.random.default_rng(120)
    centers = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(6, 3)).astype(np.float32))
    batch = ragged_batch([1, 129, 700], [255, 256, 257], rng, centers)
    on = real_rows(batch)
    w = randn(rng, batch.rows_total, 256) * on[:, None]
    cloud = torch.from_numpy(np.repeat(batch.tile_cloud.cpu().numpy(), 128)).long()
    xyz = batch.xyz.cpu()
    s64 = xyz.double() - centers.double()[cloud]
    s32 = xyz - centers[cloud]
    assert (s32[~on].abs().sum(1) > 0).all()
    wd = w.to(DEV)
    for transpose_w in (False, True):
        lay = (lambda p: p.t()) if transpose_w else (lambda p: p)
        dW = torch.full((256, 3) if transpose_w else (3, 256), 7.0, device=DEV)
        cw, cs = torch.full((256,), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
        grad3(wd, batch.xyz, dW, transpose_w, cw, cs, batch.center, batch.tile_cloud)
        what = "grad3 with centres, transpose_w %d" % transpose_w
        held(what, dW, lay(s64.t() @ w.double()), lay(s32.t() @ w))
        held(what + " col_w", cw, w.double().sum(0), w.sum(0))
        held(what + " col_s", cs, s64.sum(0), s32.sum(0))  # all packed rows, as the header says
        dW2 = torch.full_like(dW, 7.0)
        grad3(wd, batch.xyz, dW2, transpose_w, None, None, batch.center, batch.tile_cloud)
        assert torch.equal(dW, dW2)
        grad3(wd, batch.xyz, dW2, transpose_w, None, None, batch.center, batch.tile_cloud, accumulate=True)
        held(what + " accumulated", dW2, 2 * lay(s64.t() @ w.double()), 2 * lay(s32.t() @ w))


# ------------------------------------------------------------------------------------- the embedding sum
def _embed_inputs(seed, scale=1.0, zero_weights=False):
    from scream_amd.model import pe_dim_t
    rng = np.random.default_rng(seed)
    sd = make_state_dict(3, 256, 1, 1)
    centers = torch.zeros(4, 3)
    centers[0] = torch.tensor([0.1, -0.2, 0.05])
    centers[1] = torch.tensor([-0.3, 0.0, 0.2])
    batch = ragged_batch([150, 129], [70, 256], rng, centers)
    batch.xyz.mul_(scale)
    w = sd["embedding.weight"][:, :, 0].contiguous()
    b = sd["embedding.bias"]
    if zero_weights:
        w, b = torch.zeros_like(w), torch.zeros_like(b)
    return sd, batch, pe_dim_t().to(DEV), w, b


def pe_embed(batch, dim_t, w, b):
    z = torch.full((batch.rows_total, 256), 7.0, device=DEV)
    w_d, b_d = w.to(DEV), b.to(DEV)  # named: the launch reads them after this line has run
    check(_lib.load().scream_pe_embed(_p(batch.xyz), _p(batch.tile_cloud, torch.int32), _p(batch.center), _p(dim_t), _p(w_d),
                                      _p(b_d), _p(z), batch.rows_total, _stream()), "scream_pe_embed")
    return z


def test_pe_embed_then_ln_fwd_is_pe_embed_ln():
    """The training forward's scream_pe_embed + scream_ln_fwd against the inference kernel scream_pe_embed_ln on the same
    ragged batch with nonzero centres.  Observed: not bitwise equal, largest difference 7.2e-7
    (values up to 3); held to the fp32 bar of test_gpu_parity.py::test_pe_embed_prenorm_vs_oracle (rtol 1e-4, atol 2e-5)."""
    sd, batch, dim_t, w, b = _embed_inputs(130)
    g, be = sd["pre_norm.weight"].to(DEV), sd["pre_norm.bias"].to(DEV)
    z = pe_embed(batch, dim_t, w, b)
    y, _, _ = train.ln_fwd(z, None, g, be)
    fused = ops.pe_embed_ln(batch.xyz, batch.tile_cloud, batch.center, dim_t, w.to(DEV), b.to(DEV), g, be)
    print("pe_embed + ln_fwd against pe_embed_ln: bitwise equal %s, largest difference %.3g"
          % (torch.equal(y, fused), float((y - fused).abs().max())))
    torch.testing.assert_close(y, fused, rtol=1e-4, atol=2e-5)
    # and against the float64 oracle, cloud by cloud
    xyz, on = batch.xyz.cpu(), real_rows(batch)
    cloud = torch.from_numpy(np.repeat(batch.tile_cloud.cpu().numpy(), 128)).long()
    sd64 = {k: v.double() for k, v in sd.items()}
    want = O.embed_prenorm(xyz.double(), xyz.double() - batch.center.cpu().double()[cloud], sd64)
    torch.testing.assert_close(y.cpu()[on].double(), want[on], rtol=1e-4, atol=2e-5)


def test_pe_embed_against_float64():
    """scream_pe_embed alone.  With zero 1x1-conv weights it is the sine embedding: against float64 from the reference's fp32
    argument on, at the three coordinate scales and the 1.2e-6 of test_gpu_parity.py::test_pe_sine_embedding_against_float64
    (there through a LayerNorm, here without).  With the embedding's weights and nonzero centres: the fp32 bar of
    test_pe_embed_prenorm_vs_oracle."""
    for scale in (1.0, 300.0, 5000.0):
        _, batch, dim_t, w, b = _embed_inputs(131, scale, zero_weights=True)
        z = pe_embed(batch, dim_t, w, b).cpu().double()
        x32 = batch.xyz.cpu()
        p = ((x32 * np.float32(2 * np.pi))[:, :, None] / dim_t.cpu()[None, None, :]).double()
        pe = torch.stack([p[:, :, 0::2].sin(), p[:, :, 1::2].cos()], dim=3).flatten(2).flatten(1)
        pe = torch.cat([pe, torch.zeros(pe.shape[0], 4, dtype=torch.float64)], dim=1)
        on = real_rows(batch)
        err = float((z[on] - pe[on]).abs().max())
        print("pe_embed, coordinates x %g: largest error %.3g" % (scale, err))
        assert err <= 1.2e-6, (scale, err)
    sd, batch, dim_t, w, b = _embed_inputs(132)
    z = pe_embed(batch, dim_t, w, b).cpu().double()
    xyz, on = batch.xyz.cpu().double(), real_rows(batch)
    cloud = torch.from_numpy(np.repeat(batch.tile_cloud.cpu().numpy(), 128)).long()
    want = O.pe_sine(xyz, 256) + (xyz - batch.center.cpu().double()[cloud]) @ w.double().t() + b.double()
    torch.testing.assert_close(z[on], want[on], rtol=1e-4, atol=2e-5)


# ------------------------------------------------------------------------------------- LayerNorm
def _ln64(a, b, g, be, dy):
    a64, g64, be64 = (t.double().requires_grad_() for t in (a, g, be))
    y = torch.nn.functional.layer_norm(a64 if b is None else a64 + b.double(), (256,), g64, be64, 1e-5)
    y.backward(dy.double())
    return y.detach(), a64.grad, g64.grad, be64.grad


def _ln32(a, b, g, be, dy):
    a32, g32, be32 = (t.clone().requires_grad_() for t in (a, g, be))
    y = torch.nn.functional.layer_norm(a32 if b is None else a32 + b, (256,), g32, be32, 1e-5)
    y.backward(dy)
    return y.detach(), a32.grad, g32.grad, be32.grad


# rows: one; 3 (a partly used block of the forward's four rows); 127; 1280 (three blocks of the backward's 512 rows, the last
# partial); 300 000.  b NULL is how pre_norm calls both kernels (train.forward_saving / backward), dsum NULL how norm2 and
# pre_norm call the backward.
@pytest.mark.parametrize("rows", [1, 3, 127, 1280, 300000])
@pytest.mark.parametrize("with_b", [False, True])
def test_layernorm_options_against_float64(rows, with_b):
    rng = np.random.default_rng(140 + rows % 89 + with_b)
    a, dy = randn(rng, rows, 256), randn(rng, rows, 256)
    b = randn(rng, rows, 256) if with_b else None
    g = torch.from_numpy(1 + 0.1 * rng.standard_normal(256).astype(np.float32))
    be = torch.from_numpy(0.1 * rng.standard_normal(256).astype(np.float32))
    y64, dz64, dg64, db64 = _ln64(a, b, g, be, dy)
    y32, dz32, dg32, db32 = _ln32(a, b, g, be, dy)
    ad, bd, gd, bed, dyd = (None if t is None else t.to(DEV) for t in (a, b, g, be, dy))
    what = "LayerNorm rows %d b %s" % (rows, "set" if with_b else "NULL")
    y, mean, rstd = train.ln_fwd(ad, bd, gd, bed)
    held(what + " forward", y, y64, y32)
    x64 = a.double() if b is None else a.double() + b.double()
    held(what + " mean", mean, x64.mean(1), x64.float().mean(1))
    held(what + " rstd", rstd, 1 / (x64.var(1, unbiased=False) + 1e-5).sqrt(), 1 / (x64.float().var(1, unbiased=False) + 1e-5).sqrt())
    outs = []
    for _ in range(2):  # dsum NULL, accumulate 0; twice
        dz = torch.full((rows, 256), 7.0, device=DEV)
        dg, db = torch.full((256,), 7.0, device=DEV), torch.full((256,), 7.0, device=DEV)
        train.ln_bwd(dyd, ad, bd, mean, rstd, gd, dz, None, dg, db)
        outs.append((dz, dg, db))
    assert all(torch.equal(p, q) for p, q in zip(*outs)), what + ": two identical calls differ"
    dz, dg, db = outs[0]
    held(what + " dz", dz, dz64, dz32)
    held(what + " dgamma", dg, dg64, dg32)
    held(what + " dbeta", db, db64, db32)
    # dsum set: dsum += dz with the same dz; accumulate = 1 on top of the first call: twice the parameter gradients
    dsum0 = randn(rng, rows, 256)
    dsum, dz2 = dsum0.to(DEV), torch.full((rows, 256), 7.0, device=DEV)
    train.ln_bwd(dyd, ad, bd, mean, rstd, gd, dz2, dsum, dg, db, accumulate=True)
    assert torch.equal(dz2, dz)
    assert torch.equal(dsum.cpu(), dsum0 + dz.cpu())
    held(what + " dgamma accumulated", dg, 2 * dg64, 2 * dg32)
    held(what + " dbeta accumulated", db, 2 * db64, 2 * db32)


def test_layernorm_constant_rows_with_zero_gradient_add_nothing():
    """What a padded row looks like to the LayerNorm kernels: a constant row (variance 0, rstd = 1 / sqrt(1e-5)) with dy = 0.
    Its dz is exactly zero, dsum stays what it was, and dgamma / dbeta are bit for bit those of the real rows alone -- also
    when the constant rows add whole blocks of 512 to the backward's grid."""
    rng = np.random.default_rng(150)
    R, pad = 700, 900  # 700 real rows (two blocks), then 900 constant ones (the second block's tail and two more blocks)
    a, b, dy = randn(rng, R + pad, 256), randn(rng, R + pad, 256), randn(rng, R + pad, 256)
    value = torch.tensor([0.0, 3.0, -0.7, 1e-3]).repeat(pad // 4)[:, None]
    a[R:], b[R:], dy[R:] = value, 0.5 * value, 0.0
    g = torch.from_numpy(1 + 0.1 * rng.standard_normal(256).astype(np.float32)).to(DEV)
    be = torch.from_numpy(0.1 * rng.standard_normal(256).astype(np.float32)).to(DEV)
    ad, bd, dyd = a.to(DEV), b.to(DEV), dy.to(DEV)

    def run(rows, with_b):
        bb = bd[:rows] if with_b else None
        y, mean, rstd = train.ln_fwd(ad[:rows], bb, g, be)
        dz, dsum = torch.full((rows, 256), 7.0, device=DEV), torch.full((rows, 256), 2.0, device=DEV)
        dg, db = torch.full((256,), 7.0, device=DEV), torch.full((256,), 7.0, device=DEV)
        train.ln_bwd(dyd[:rows], ad[:rows], bb, mean, rstd, g, dz, dsum, dg, db)
        return y, mean, rstd, dz, dsum, dg, db

    for with_b in (False, True):
        y, mean, rstd, dz, dsum, dg, db = run(R + pad, with_b)
        _, _, _, dz_r, dsum_r, dg_r, db_r = run(R, with_b)
        x = a[R:, 0] + (b[R:, 0] if with_b else 0)
        assert torch.equal(mean[R:].cpu(), x), "the mean of a constant row is its value"
        assert rel(rstd[R:], torch.full((pad,), 1e-5, dtype=torch.float64).rsqrt()) <= 1e-6
        assert torch.equal(y[R:], be[None].expand(pad, 256)), "a constant row normalises to beta"
        assert (dz[R:] == 0).all() and (dsum[R:] == 2.0).all()
        assert torch.equal(dz[:R], dz_r) and torch.equal(dsum[:R], dsum_r)
        assert torch.equal(dg, dg_r) and torch.equal(db, db_r)


# ------------------------------------------------------------------------------------- weight gradients at the q|k|v shapes
@pytest.mark.parametrize("split", [False, True])
def test_wgrad_at_the_qkv_shapes_and_wide_leading_dimensions(split):
    """768 x 256 (the self layers' q|k|v) and 512 x 256 (the cross layers' k|v) as train._block_bwd calls them: dY [rows, N]
    with zero padded rows, X the block input, one dW whose row slices become the three (two) parameter gradients.  Then N x K
    = 256 x 256 out of the MIDDLE of wider matrices (ldy = 768, ldx = 512, both pointers offset), where every other column must
    stay out of the sum."""
    fn = train.wgrad_split if split else train.wgrad
    rng = np.random.default_rng(160 + split)
    lens = [700, 1, 129, 500]
    for N in (768, 512):
        dY, X = packed_rows(lens, rng, N), packed_rows(lens, rng, 256, pad_value=3.0)
        want, cpu32 = dY.double().t() @ X.double(), dY.t() @ X
        dW = torch.full((N, 256), 7.0, device=DEV)
        fn(dY.to(DEV), X.to(DEV), dW)
        held("wgrad%s %d x 256" % ("_split" if split else "", N), dW, want, cpu32)
        for i in range(N // 256):  # each parameter's slice on its own
            sl = slice(256 * i, 256 * (i + 1))
            held("  rows %d.. of it" % (256 * i), dW[sl], want[sl], cpu32[sl])
        again = torch.full((N, 256), 7.0, device=DEV)
        fn(dY.to(DEV), X.to(DEV), again)
        assert torch.equal(dW, again)
    wideY, wideX = packed_rows(lens, rng, 768), packed_rows(lens, rng, 512, pad_value=3.0)
    dYs, Xs = wideY.to(DEV)[:, 256:512], wideX.to(DEV)[:, 128:384]
    assert dYs.stride(0) == 768 and Xs.stride(0) == 512 and not dYs.is_contiguous()
    want, cpu32 = wideY[:, 256:512].double().t() @ wideX[:, 128:384].double(), wideY[:, 256:512].t() @ wideX[:, 128:384]
    dW, cs = torch.full((256, 256), 7.0, device=DEV), torch.full((256,), 7.0, device=DEV)
    fn(dYs, Xs, dW, cs)
    held("wgrad%s 256 x 256 of ldy 768, ldx 512" % ("_split" if split else ""), dW, want, cpu32)
    held("  its column sums", cs, wideY[:, 256:512].double().sum(0), wideY[:, 256:512].sum(0))


# ------------------------------------------------------------------------------------- data gradients
def gemms(split):
    return train.gemms("split" if split else "f32")


@pytest.mark.parametrize("split", [False, True])
def test_data_gradients_at_the_five_weight_shapes_against_float64(split):
    """The arithmetic's dgrad, dX = dY W, for the weights of a block.  Under "split", 768 and 512 summed columns run as K = 256
    products added in column order (scream_add_f32): twice, bitwise equal."""
    rng = np.random.default_rng(170 + split)
    mm = gemms(split)
    lens = [700, 1, 129, 500]
    for N, K in ((768, 256), (512, 256), (256, 256), (1024, 256), (256, 1024)):
        dY = packed_rows(lens, rng, N)
        W = randn(rng, N, K) / 16
        want, cpu32 = dY.double() @ W.double(), dY @ W
        got = mm.dgrad(dY.to(DEV), W.to(DEV))
        held("dgrad %s %d x %d" % ("split" if split else "f32", N, K), got, want, cpu32)
        out = torch.full_like(got, 7.0)
        assert mm.dgrad(dY.to(DEV), W.to(DEV), out=out) is out and torch.equal(out, got)  # out=, and a second call


def test_gemm_f32_and_gemm_split_take_row_strided_views():
    """A = columns 256..511 of a [256, 768] matrix (two row tiles: a wrong row stride shows between them), out = the same
    columns of another; every other column of both holds 7.0.  The result equals the call on contiguous copies bit for bit,
    the columns outside the slice stay 7.0, and a view with column stride 2 raises before any launch."""
    rng = np.random.default_rng(175)
    wideA = torch.full((256, 768), 7.0)
    wideA[:, 256:512] = randn(rng, 256, 256)
    wideA, W = wideA.to(DEV), (randn(rng, 256, 256) / 16).to(DEV)
    Wp = ops.pack_w(W, _lib.SPLIT_BF3)
    A = wideA[:, 256:512]
    assert A.stride() == (768, 1) and not A.is_contiguous()
    for what, gemm in (("gemm_f32", lambda a, out: ops.gemm_f32(a, W, out=out)), ("gemm_split", lambda a, out: ops.gemm_split(a, Wp, out=out))):
        wide_out = torch.full((256, 768), 7.0, device=DEV)
        out = wide_out[:, 256:512]
        assert gemm(A, out) is out
        want = gemm(A.contiguous(), torch.empty(256, 256, device=DEV))
        assert torch.equal(out, want), what
        assert (wide_out[:, :256] == 7.0).all() and (wide_out[:, 512:] == 7.0).all(), what
        before = wide_out.clone()
        with pytest.raises(ValueError):
            gemm(wideA[:, 0:512:2], torch.empty(256, 256, device=DEV))
        with pytest.raises(ValueError):
            gemm(A, wide_out[:, 0:512:2])
        assert torch.equal(wide_out, before), what


# ------------------------------------------------------------------------------------- one block end to end
BLOCK_WEIGHTS = ["q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "norm1.weight", "norm1.bias", "mlp.0.weight",
                 "mlp.2.weight", "norm2.weight", "norm2.bias"]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("cross", [False, True])
def test_one_block_forward_and_backward_against_float64(cross, split):
    """train._block_fwd + train._block_bwd on a ragged packed batch against float64 autograd of O.mh_attention per cloud, under
    the block's own relu mask (hid > 0): the input gradient dx, the target features' gradient dt of a cross layer, and the
    ten weight gradients, each at the rule of tests/train_ref.py; dx (and dt) exactly zero on padded rows.  A self block
    runs over all packed rows and clouds, as PointTransformer's stem does; a cross block on the source rows against the
    target rows."""
    rng = np.random.default_rng(180 + 2 * cross + split)
    prefix = "cross.1.layer." if cross else "stem.0."
    sd = {k[len(prefix):]: v for k, v in make_state_dict(21, 256, 1, 1).items() if k.startswith(prefix)}
    assert sorted(sd) == sorted(BLOCK_WEIGHTS)
    batch = ragged_batch([1, 129, 300], [255, 256, 257])
    B, rs, rt, row0, lens = 3, batch.rows_src, batch.rows_total, batch.cloud_row0_host, batch.cloud_len_host
    on = real_rows(batch)
    feats = randn(rng, rt, 256)  # padded rows hold finite features too
    dy = randn(rng, rt, 256) * on[:, None]  # ... and carry no gradient
    P = {prefix + k: torch.nn.Parameter(v.to(DEV)) for k, v in sd.items()}
    G = {n: torch.full_like(p, 7.0) for n, p in P.items()}
    mm = gemms(split)
    fd = feats.to(DEV)
    if cross:
        x, t, n_rows, clouds = fd[:rs], fd[rs:], rs, [(p, B + p) for p in range(B)]
        y, L = train._block_fwd(P, mm, prefix, x, t, batch, 0, 0, B)
        dt = torch.zeros(rt - rs, 256, device=DEV)
    else:
        x, t, n_rows, clouds = fd, None, rt, [(c, c) for c in range(2 * B)]
        y, L = train._block_fwd(P, mm, prefix, x, None, batch, 0, 0, 2 * B)
        dt = None
    dx = dy[:n_rows].to(DEV).clone()
    train._block_bwd(P, G, mm, L, dx, batch, dt)
    hid_on = (L.hid > 0).cpu()
    rows_of = lambda c: slice(int(row0[c]), int(row0[c]) + int(lens[c]))

    def oracle(dtype):
        w = {prefix + k: v.to(dtype).requires_grad_() for k, v in sd.items()}
        f = feats.to(dtype).requires_grad_()
        outs, total = torch.zeros(n_rows, 256, dtype=dtype), 0
        for qc, kc in clouds:
            o = O.mh_attention(f[rows_of(qc)][None], f[rows_of(kc)][None], f[rows_of(kc)][None], w, prefix,
                               relu_mask=hid_on[rows_of(qc)][None])[0]
            outs[rows_of(qc)] = o.detach()
            total = total + (o * dy[rows_of(qc)].to(dtype)).sum()
        total.backward()
        return outs, f.grad, {k: v.grad for k, v in w.items()}

    y64, df64, g64 = oracle(torch.float64)
    y32, df32, g32 = oracle(torch.float32)
    what = "%s block, %s" % ("cross" if cross else "self", "split" if split else "f32")
    real = on[:n_rows]
    held(what + " output", y.cpu()[real], y64[real], y32[real])
    got = {n: g.detach().cpu() for n, g in G.items()}
    got["dx"], g64["dx"], g32["dx"] = dx.cpu(), df64[:n_rows], df32[:n_rows]
    assert (dx.cpu()[~real] == 0).all(), "the input gradient of a padded row is not zero"
    if cross:
        got["dt"], g64["dt"], g32["dt"] = dt.cpu(), df64[rs:], df32[rs:]
        assert (dt.cpu()[~on[rs:]] == 0).all(), "the target gradient of a padded row is not zero"
    assert len(got) == 10 + 1 + cross
    bad = T.rule(what, got, g64, g32)
    assert not bad, bad
