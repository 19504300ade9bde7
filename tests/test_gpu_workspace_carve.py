"""Every op whose workspace size is its carve on a null base (voxel, raw ICP, prep, render, wgrad on both arithmetics, attn_bwd),
run with EXACTLY the bytes its size function reports, from the middle of a larger tensor: the bytes on either side keep their
fill, what the workspace held before (0x00, 0xFF) changes no output bit, the outputs are the public op's on a workspace of its
own, and one byte less is SCREAM_EINVAL with outputs and buffer untouched.  The margin in front is 272 bytes -- a multiple of 16,
which these ops ask of the pointer, and not of 256, which the Carver's pieces are multiples of -- and 512 for the raw ICP, which
asks for 256.  The model is test_icp_run_stays_inside_exactly_the_workspace_it_asks_for.  Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import prep_ref as PR
import rawicp_ref as RR
from scream_amd import _lib, ops, train
from scream_amd.prep import prepare_pairs, sample_perturbations
from scream_amd.rawicp import _RawClouds, icp_raw_batch, raw_nn_batch
from scream_amd.render import rotation_matrix, view_eulers
from test_gpu_train_kernels import ragged_batch, randn, real_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN, MARGIN_RAW = 272, 512
SENTINEL = 7


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


class Exact:
    """While active, the wrappers' scratch (ops._workspace) is exactly the size function's bytes, MARGIN bytes into a tensor
    filled with `fill`, and every call into the library is recorded with its arguments."""

    def __init__(self, monkeypatch):
        self.mp, self.lib, self.fill, self.calls, self.big, self.need = monkeypatch, _lib.load(), 0, [], None, None
        self.short = 0  # bytes withheld from the size function's answer

    def __enter__(self):
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()
        me = self

        class Recorder:
            def __getattr__(_, name):
                fn = getattr(me.lib, name)

                def call(*args):
                    me.calls.append((name, args))
                    return fn(*args)
                return call

        def workspace(name, *args, device, floor=16):
            assert me.big is None, "one workspace per run"
            me.need = getattr(me.lib, name)(*args) - me.short
            assert me.need >= floor, (name, args, me.need)
            me.big = torch.full((MARGIN + me.need + MARGIN,), me.fill, dtype=torch.uint8, device=device)
            return me.big[MARGIN:MARGIN + me.need]

        m.setattr(_lib, "load", lambda: Recorder())
        m.setattr(ops, "_workspace", workspace)
        m.setattr(train, "_workspace", workspace)
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)

    def run(self, fill, fn):
        """fn() under a fresh big tensor of `fill`; afterwards the margins still hold it."""
        self.fill, self.big, self.calls = fill, None, []
        out = fn()
        torch.cuda.synchronize()
        assert self.big is not None
        assert bool((self.big[:MARGIN] == fill).all()) and bool((self.big[MARGIN + self.need:] == fill).all()), fill
        return out

    def refuse(self, outputs, need=None):
        """Every recorded call that was given the workspace, once more on one byte less than `need` (default: what the size
        function said) and on outputs full of SENTINEL."""
        need = self.need if need is None else need
        ptr = self.big.data_ptr() + MARGIN
        took = [(name, args) for name, args in self.calls if ptr in args]
        assert took
        for o in outputs:
            assert any(o.data_ptr() in args for _, args in took)  # what the library wrote, not a copy of it
            o.fill_(SENTINEL)
        self.big.zero_()
        for name, args in took:
            k = args.index(ptr)
            assert args[k + 1] == self.need, name
            assert getattr(self.lib, name)(*args[:k + 1], need - 1, *args[k + 2:]) == -1, name  # SCREAM_EINVAL
        torch.cuda.synchronize()
        for o in outputs:
            assert bool((o == SENTINEL).all())
        assert not bool(self.big.any())


def same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))  # bit for bit, whatever the type


def exact_workspace(monkeypatch, fn):
    """fn() -> tuple of output tensors, through the public op.  The whole rule of this file for one op."""
    want = fn()
    with Exact(monkeypatch) as ex:
        for fill in (0x00, 0xFF):
            got = ex.run(fill, fn)
            same(got, want)
        ex.refuse(got)


def test_voxel_stays_inside_exactly_the_workspace_it_asks_for(monkeypatch):
    """Three clouds of 257, 0 and 300 points, voxel 0.05, in one call.
    scream_voxel_down_sample is told max_len, not the rows of the call: it refuses a workspace below the size for max_len rows and
    takes the rows it was sized for from the bytes it is given (the largest row count whose carve fits).  So one byte below the
    size for 557 rows is not SCREAM_EINVAL -- that holds before and after the carve became the size -- but a workspace for fewer
    rows: the cloud whose rows end beyond them reports -1, the others are bit for bit what they were, and the margins stand.
    SCREAM_EINVAL with everything untouched is asserted where the entry point draws it, one byte below the size for 300 rows."""
    rng = np.random.default_rng(5)
    lens = [257, 0, 300]
    xyz = dev(rng.uniform(-1, 1, size=(sum(lens), 3)).astype(np.float32))
    row0, length = dev([0, 257, 257], torch.int32), dev(lens, torch.int32)
    voxel = dev([0.05] * 3, torch.float64)
    gather = lambda t, n: t[torch.cat([torch.arange(r, r + max(k, 0)) for r, k in zip((0, 257, 257), n)]).to(DEV)].contiguous()

    def fn():
        out, out_len, cnt = fn.raw = ops.voxel_down_sample_packed(xyz, row0, length, max(lens), voxel, want_counts=True)
        fn.n = out_len.cpu().tolist()
        return gather(out, fn.n), out_len, gather(cnt, fn.n)  # (the rows behind a cloud's voxels are not written)

    want = fn()
    n = fn.n
    assert n[1] == 0 and 0 < n[0] <= 257 and 0 < n[2] <= 300
    with Exact(monkeypatch) as ex:
        for fill in (0x00, 0xFF):
            same(ex.run(fill, fn), want)
        ex.short = 1
        out, out_len, cnt = ex.run(0xFF, fn)
        assert fn.n == [n[0], 0, -1]
        same((out, cnt), (want[0][:n[0]], want[2][:n[0]]))
        ex.refuse(fn.raw, need=ex.lib.scream_voxel_workspace_bytes(max(lens), 3))


@pytest.mark.parametrize("mode", ["ball", "bbox"])
def test_prep_stays_inside_exactly_the_workspace_it_asks_for(monkeypatch, mode):
    """Three float64 pairs of (257, 300), (40, 40) and (300, 129) points, no noise, centre rule "mean" (the one that uses
    part_cen); ball runs the radius launch, bbox does not.  Bit for bit tests/prep_ref.py's, as test_prepare_pairs_bit_for_bit."""
    from test_gpu_prep import compare, ref_prepare, same_bits
    raws = [PR.raw_pair(80 + i, n, m, np.float64) for i, (n, m) in enumerate([(257, 300), (40, 40), (300, 129)])]
    perturb, _ = sample_perturbations(3, 0.1, 5)
    side = [0, 1, 0]
    srcs, tgts, T = [dev(r[0]) for r in raws], [dev(r[1]) for r in raws], np.stack([r[2] for r in raws])
    packed, alive = ops.prep_pairs_packed, []  # the arrays prepare_pairs packs stay allocated until the refused call has returned
    monkeypatch.setattr(ops, "prep_pairs_packed", lambda *a: (alive.append(a), packed(*a))[1])

    def fn():
        p = prepare_pairs(srcs, tgts, T, mode=mode, center="mean", perturb=perturb, side=side)
        fn.last = p
        return p.batch.xyz, p.batch.center, p.rot, p.trans, p.s, p.c, p.T_aug

    exact_workspace(monkeypatch, fn)
    fn()
    want = ref_prepare(raws, mode, "mean", perturb, side)
    compare(fn.last, want, same_bits, mode)
    same_bits(fn.last.s, np.array([w["s"] for w in want]), "s")
    same_bits(fn.last.c, np.stack([w["c"] for w in want]), "c")
    same_bits(fn.last.T_aug, np.stack([w["T_aug"] for w in want]), "T_aug")


def test_render_stays_inside_exactly_the_workspace_it_asks_for(monkeypatch):
    """Two pairs (300 + 70 and 40 + 257 points), 2 views, w = 64: the forward, then the backward on the same slice."""
    g = torch.Generator().manual_seed(9)
    s_len, t_len = [300, 40], [70, 257]
    S, T = (torch.rand(340, 3, generator=g) * 1.8 - 0.9).to(DEV), (torch.rand(327, 3, generator=g) * 1.8 - 0.9).to(DEV)
    s_row0, t_row0 = dev([0, 300], torch.int32), dev([0, 70], torch.int32)
    s_n, t_n = dev(s_len, torch.int32), dev(t_len, torch.int32)
    rot = torch.stack([rotation_matrix(e) for e in view_eulers("muti")[:2]]).to(DEV)
    up = torch.randn(2, 2, 2, 64, 64, generator=g).to(DEV)

    def fn():
        ws = ops.render_workspace(2, 2, 64, S.shape[0], DEV)
        imgs, amax = ops.render_depth(S, s_row0, s_n, T, t_row0, t_n, 300, 257, rot, 64, 24, ws)
        dsrc = ops.render_depth_bwd(up, amax, S, s_row0, s_n, 300, rot, 64, 24, ws)
        return imgs, amax, dsrc

    want = fn()
    assert bool((want[1] >= 0).any()) and bool(want[2].any())
    exact_workspace(monkeypatch, fn)


@pytest.mark.parametrize("split", [False, True])
def test_wgrad_stays_inside_exactly_the_workspace_it_asks_for(monkeypatch, split):
    """Rows = 300, N = K = 128 with column sums: three row slices, part and colpart both in use."""
    rng = np.random.default_rng(11)
    dY, X = randn(rng, 300, 128).to(DEV), randn(rng, 300, 128).to(DEV)
    assert _lib.load().scream_wgrad_workspace_bytes(300, 128, 128) == 3 * (128 * 128 + 128) * 4
    op = train.wgrad_split if split else train.wgrad

    def fn():
        dW, col = torch.empty(128, 128, device=DEV), torch.empty(128, device=DEV)
        op(dY, X, dW, col)
        return dW, col

    exact_workspace(monkeypatch, fn)


def test_attn_bwd_stays_inside_exactly_the_workspace_it_asks_for(monkeypatch):
    """Two query clouds of 300 and 40 rows, max_chunks = 2, attending to themselves (a self layer on the source rows):
    dq | dk | dv equal a run on a generous workspace."""
    rng = np.random.default_rng(13)
    batch = ragged_batch([300, 40], [129, 1])
    B, rs, D = 2, batch.rows_src, 256
    assert batch.max_chunks == 2 and rs == 384 + 128
    on = real_rows(batch)[:rs, None]
    qkv = (randn(rng, rs, 3 * D).abs() + 0.1).to(DEV)  # Q' and K' are elu + 1 > 0
    dO = (randn(rng, rs, D) * on).to(DEV)
    kv = ops.kv_reduce(qkv[:, D:], qkv[:, 2 * D:], 3 * D, 0, batch.cloud_row0, batch.cloud_len, 0, B, batch.max_chunks, 2 * B)
    att = ops.attn_apply(qkv, 3 * D, kv, batch.tile_cloud, 0, batch.cloud_len, rs)
    p = lambda t, col=0: t.data_ptr() + 4 * col

    def call(dqkv):
        train.attn_bwd(p(qkv), 3 * D, rs, 0, att, dO, p(qkv, D), p(qkv, 2 * D), 3 * D, rs, 0, kv, batch, 0, B, 0, p(dqkv), 3 * D,
                       p(dqkv, D), p(dqkv, 2 * D), 3 * D)
        return (dqkv,)

    fn = lambda: call(torch.empty(rs, 3 * D, device=DEV))
    generous = torch.empty(rs, 3 * D, device=DEV)
    need = _lib.load().scream_attn_bwd_workspace_bytes(B, batch.max_chunks)
    with monkeypatch.context() as m:
        m.setattr(train, "_workspace", lambda *a, device, **k: torch.zeros(4 * need, dtype=torch.uint8, device=device))
        call(generous)
    assert bool(generous.any()) and bool((generous[~on[:, 0].to(DEV)] == 0).all())
    same(fn(), (generous,))
    exact_workspace(monkeypatch, fn)


def test_raw_icp_stays_inside_exactly_the_workspace_it_asks_for():
    """Two pairs, sources of 257 and 40 rows against targets of 300 and 70: three iterations of scream_icp_raw_range, then one
    scream_icp_raw_nn on the same workspace, 512 bytes into the big tensor (the entry points ask for 256-byte alignment)."""
    a, b = RR.ring_pair(n=300, seed=1), RR.ring_pair(n=70, seed=2)
    srcs, tgts, T0, radius = [a[0][:257], b[0][:40]], [a[1], b[1]], np.stack([a[2], b[2]]), 0.2
    want = icp_raw_batch(srcs, tgts, T0, radius, 3, 1e-6, 1e-6, strict=False)[:3]
    wi, wd, wstatus = raw_nn_batch(srcs, tgts, want[0], radius, strict=False)
    assert want[2].cpu().tolist() == [3, 3] and wstatus.tolist() == [0, 0] and bool((torch.cat(wi) >= 0).any())
    want_nn = (torch.cat(wi), torch.cat(wd))
    lib, pk = _lib.load(), _RawClouds(srcs, tgts)
    assert (pk.s_rows, pk.t_rows, pk.n) == (297, 370, 2)
    need = lib.scream_icp_raw_workspace_bytes(pk.s_rows, pk.t_rows, pk.n)
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()

    def run(ws, ws_bytes, outs):
        T, fr, iters, idx, d2, status = outs
        rc = lib.scream_icp_raw_range(*pk.head_args(), radius, 3, 1e-6, 1e-6, ptr(T), ptr(fr), ptr(iters), 0, 4, None, ws, ws_bytes, stream)
        if rc == 0:
            rc = lib.scream_icp_raw_nn(*pk.head_args(), radius, ptr(T), ptr(idx), ptr(d2), ptr(status), ws, ws_bytes, stream)
        torch.cuda.synchronize()
        return rc

    def outputs(T_fill=None):
        T = dev(T0) if T_fill is None else torch.full((2, 4, 4), float(T_fill), dtype=torch.float64, device=DEV)
        return (T, torch.full((2, 2), float(SENTINEL), dtype=torch.float64, device=DEV), torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV),
                torch.full((297,), SENTINEL, dtype=torch.int32, device=DEV), torch.full((297,), float(SENTINEL), dtype=torch.float64, device=DEV),
                torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV))

    for fill in (0x00, 0xFF):
        big = torch.full((MARGIN_RAW + need + MARGIN_RAW,), fill, dtype=torch.uint8, device=DEV)
        assert (big.data_ptr() + MARGIN_RAW) % 256 == 0
        outs = outputs()
        assert run(big.data_ptr() + MARGIN_RAW, need, outs) == 0
        assert bool((big[:MARGIN_RAW] == fill).all()) and bool((big[MARGIN_RAW + need:] == fill).all()), fill
        same(outs[:3], want)
        same(outs[3:5], want_nn)
        assert outs[5].tolist() == [0, 0]
    big = torch.zeros(MARGIN_RAW + need + MARGIN_RAW, dtype=torch.uint8, device=DEV)
    outs = outputs(T_fill=SENTINEL)
    assert run(big.data_ptr() + MARGIN_RAW, need - 1, outs) == -1  # SCREAM_EINVAL from the first call; the second is not made
    assert lib.scream_icp_raw_nn(*pk.head_args(), radius, ptr(outs[0]), ptr(outs[3]), ptr(outs[4]), ptr(outs[5]), big.data_ptr() + MARGIN_RAW,
                                 need - 1, stream) == -1
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert not bool(big.any())
