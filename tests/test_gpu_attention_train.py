"""The five fp32 kernels every attention block runs in training -- scream_kv_reduce and scream_attn_apply (csrc/attention.hip) and the
four launches of scream_attn_bwd (csrc/backward.hip) -- held to float64 ELEMENT BY ELEMENT, against tests/attn_ref.py:

    |got - want| <= n 2^-24 A + n 2^-149

with A the magnitude companion of the element and n its chain count, both derived there from the formulas and the kernels'
operation counts; no tolerance here comes from a measured error.  One packed batch of nine pairs whose lengths sit on both sides of
every edge of the kernels (attn_ref.SRC_LEN / TGT_LEN), heads whose Q' or K' or both are tiny, a loss-scaled and a vanishing head
of dO, in the three forms train._block_fwd / _block_bwd call the kernels in:

  self    all 2B clouds; one [rows, 768] buffer holds Q'|K'|V and one dq|dk|dv: leading dimension 768, pointers offset by 256 and
          512 columns, row bases 0
  cross   queries: clouds [0, B) at leading dimension 256; keys: leading dimension 512, kv_row_base = rows_src, kv_cloud_offset = B
  tself   the self layer of DEMTransformer's target-side stem: q_cloud_begin = B, both row bases rows_src, buffers starting there

Needs an MI355X: run with `pytest -m gpu`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_ref as R
from scream_amd import _lib, ops, train
from scream_amd.packing import PackedBatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 7.0    # what the gradient buffers hold before a call
GUARD = 128   # rows of FILL before and after the rows a call owns
PAD = 3.0     # finite garbage in the padded rows of every input
B = len(R.SRC_LEN)
OUT = ("dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Rig:
    """One packed batch on the GPU and the three entry points in one of the call forms."""

    def __init__(self, src_len, tgt_len):
        lens, row0, rs, rt, tile_cloud, max_chunks = PackedBatch.layout(src_len, tgt_len)
        n = len(src_len)
        self.batch = PackedBatch(n, list(src_len), list(tgt_len), row0, lens, rs, rt, max_chunks, torch.zeros(rt, 3, device=DEV),
                                 torch.zeros(2 * n, 3, device=DEV), _dev(tile_cloud), _dev(row0), _dev(lens))
        self.lay = R.Layout(lens, row0, rs, rt)

    def geom(self, form):
        n = self.lay.B
        (q0, q1), (k0, k1) = self.lay.row_ranges(form)
        qcb, nq, koff = {"self": (0, 2 * n, 0), "cross": (0, n, n), "tself": (n, n, 0)}[form]
        return SimpleNamespace(q0=q0, q1=q1, k0=k0, k1=k1, qcb=qcb, nq=nq, koff=koff)

    def load(self, form, Q, K, V):
        """The form's input buffers from packed [rows_total, 256] arrays."""
        g = self.geom(form)
        if form == "cross":
            qb, kb = _dev(Q[g.q0:g.q1]), _dev(np.concatenate([K[g.k0:g.k1], V[g.k0:g.k1]], 1))
            return SimpleNamespace(g=g, form=form, Qt=qb, ldq=256, Kt=kb, Vt=kb[:, 256:], ldkv=512)
        b = _dev(np.concatenate([Q, K, V], 1)[g.q0:g.q1])
        return SimpleNamespace(g=g, form=form, Qt=b, ldq=768, Kt=b[:, 256:], Vt=b[:, 512:], ldkv=768)

    def reduce(self, x):
        g, b = x.g, self.batch
        kv = ops.kv_reduce(x.Kt, x.Vt, x.ldkv, g.k0, b.cloud_row0, b.cloud_len, g.qcb + g.koff, g.nq, b.max_chunks, 2 * self.lay.B)
        return kv.cpu().numpy()

    def apply(self, x, img):
        """O in packed rows [rows_total, 256]; zero outside the rows the call owns."""
        g, b = x.g, self.batch
        att = ops.attn_apply(x.Qt, x.ldq, _dev(img), b.tile_cloud[g.q0 // 128:], g.koff, b.cloud_len, g.q1 - g.q0)
        out = np.zeros((self.lay.rt, 256), np.float32)
        out[g.q0:g.q1] = att.cpu().numpy()
        return out

    def bwd(self, x, O, dO, img):
        """dq, dk, dv in packed rows [rows_total, 256] (zero outside the rows the call owns), and 'outside': whether everything
        in the gradient buffers beside what the call owns still holds FILL."""
        g, b = x.g, self.batch
        Rq, Rk = g.q1 - g.q0, g.k1 - g.k0
        Od, dOd, kv = _dev(O[g.q0:g.q1]), _dev(dO[g.q0:g.q1]), _dev(img)
        if x.form == "cross":
            gq = torch.full((Rq + 2 * GUARD, 256), FILL, device=DEV)
            gk = torch.full((Rk + 2 * GUARD, 512), FILL, device=DEV)
            pq, pk, lddq, lddkv = gq[GUARD:].data_ptr(), gk[GUARD:].data_ptr(), 256, 512
            pv = pk + 256 * 4
        else:
            gq = gk = torch.full((Rq + 2 * GUARD, 768), FILL, device=DEV)
            pq, lddq, lddkv = gq[GUARD:].data_ptr(), 768, 768
            pk, pv = pq + 256 * 4, pq + 512 * 4
        train.attn_bwd(x.Qt.data_ptr(), x.ldq, Rq, g.q0, Od, dOd, x.Kt.data_ptr(), x.Vt.data_ptr(), x.ldkv, Rk, g.k0, kv, b,
                       g.qcb, g.nq, g.koff, pq, lddq, pk, pv, lddkv)
        torch.cuda.synchronize()
        hq, hk = gq.cpu().numpy(), gk.cpu().numpy()
        outside = all((h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all() for h in (hq, hk))
        cols = {"dq": (hq, 0), "dk": (hk, 0), "dv": (hk, 256)} if x.form == "cross" else \
               {"dq": (hq, 0), "dk": (hq, 256), "dv": (hq, 512)}
        res = dict(outside=bool(outside))
        for k, (h, c) in cols.items():
            r0, r1 = (g.q0, g.q1) if k == "dq" else (g.k0, g.k1)
            res[k] = np.zeros((self.lay.rt, 256), np.float32)
            res[k][r0:r1] = h[GUARD:-GUARD, c:c + 256]
        return res


def _with_padding(lay, a, value):
    a = a.copy()
    for c in range(2 * lay.B):
        a[lay.pad(c)] = value
    return a


@pytest.fixture(scope="module")
def S():
    """The batch of nine, its inputs (padded rows hold PAD), the float64 forward rounded once, and per form one run of each entry
    point alone: kv_reduce, attn_apply fed the rounded float64 image, attn_bwd fed the rounded float64 O and image."""
    rig = Rig(R.SRC_LEN, R.TGT_LEN)
    lay = rig.lay
    assert rig.batch.max_chunks == 3
    x = {k: _with_padding(lay, v, PAD) for k, v in R.make_inputs(lay.rt).items() if k in ("Q", "K", "V", "dO")}
    s = SimpleNamespace(rig=rig, lay=lay, x=x, f={})
    for form in R.FORMS:
        img, O32 = R.forward_rounded(lay, form, x["Q"], x["K"], x["V"])
        O32 = _with_padding(lay, O32, PAD)
        dev = rig.load(form, x["Q"], x["K"], x["V"])
        s.f[form] = SimpleNamespace(img=img, O=O32, dev=dev, kv=rig.reduce(dev), att=rig.apply(dev, img),
                                    bwd=rig.bwd(dev, O32, x["dO"], img))
    return s


def _clouds(lay, form):
    pairs = lay.pairs(form)
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _hold(what, lay, got, want, A, n, rows=None):
    """Every element (of the rows given) inside the bar; prints the worst err / (2^-24 A) and where it is."""
    if rows is not None:
        idx = np.flatnonzero(rows)
        got, want, A, n = got[idx], want[idx], A[idx], (n[idx] if np.ndim(n) else n)
    ratio, at = R.worst(got, want, A)
    if rows is not None:
        c, r = lay.where(int(idx[at[0]]))
        where = "cloud %d (%d rows), head %d, row %d, column %d" % (c, lay.lens[c], at[1] // 32, r, at[1] % 32)
    else:
        where = "cloud %d (%d rows), head %d, element %d" % (at[0], lay.lens[at[0]], at[1], at[2])
    bound = float(np.broadcast_to(n, got.shape)[at])
    print("%s: worst err / (2^-24 A) %.2f (bar %d) at %s" % (what, ratio, bound, where))
    bad = R.misses(got, want, A, n)
    assert not bad.any(), "%s: %d elements outside the bar, the worst at %.3g x 2^-24 A (bar %d), %s" % (
        what, int(bad.sum()), ratio, bound, where)


def _hold_bwd(what, lay, form, got, ref):
    qc, kc = _clouds(lay, form)
    for k in OUT:
        want, A, n = ref[k]
        _hold("%s, %s form, %s" % (what, form, k), lay, got[k], want, A, n, lay.real(qc if k == "dq" else kc))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------- 1, 2, 3: the bar
@pytest.mark.parametrize("form", R.FORMS)
def test_backward_alone_meets_the_bar(S, form):
    """scream_attn_bwd handed the float64 O and kv rounded once: dq, dk, dv at every element of every real row."""
    f, x = S.f[form], S.x
    print()
    _hold_bwd("attn_bwd alone", S.lay, form, f.bwd, R.ref_bwd(S.lay, form, x["Q"], x["K"], x["V"], f.O, x["dO"], f.img))


@pytest.mark.parametrize("form", R.FORMS)
def test_reduce_and_apply_alone_meet_the_bar(S, form):
    """scream_kv_reduce on K', V; scream_attn_apply on Q' and the rounded float64 image."""
    f, x, lay = S.f[form], S.x, S.lay
    print()
    want, A, n = R.ref_reduce(lay, form, x["K"], x["V"])
    _hold("kv_reduce, %s form, kv" % form, lay, f.kv, want, A, n)
    other = sorted(set(range(2 * B)) - set(_clouds(lay, form)[1]))
    assert (f.kv[other] == 0).all()  # clouds that are no key cloud of the call stay as ops.kv_reduce made them
    want, A = R.ref_apply(lay, form, x["Q"], f.img)
    _hold("attn_apply, %s form, O" % form, lay, f.att, want, A, R.chain("O"), lay.real(_clouds(lay, form)[0]))


@pytest.mark.parametrize("form", R.FORMS)
def test_chain_as_training_runs_it_meets_the_bar(S, form):
    """The GPU's own kv and O go into scream_attn_bwd; the restatement is evaluated from those same fp32 arrays."""
    f, x, rig = S.f[form], S.x, S.rig
    att = rig.apply(f.dev, f.kv)
    got = rig.bwd(f.dev, att, x["dO"], f.kv)
    print()
    _hold_bwd("kv_reduce -> attn_apply -> attn_bwd", S.lay, form, got, R.ref_bwd(S.lay, form, x["Q"], x["K"], x["V"], att, x["dO"], f.kv))


# ------------------------------------------------------------------------------------- 4, 5: padding
def _assert_padding_zero(lay, form, got):
    qc, kc = _clouds(lay, form)
    assert got["outside"], "%s form: a gradient buffer changed outside the rows and columns the call owns" % form
    for k in OUT:
        for c in (qc if k == "dq" else kc):
            assert (got[k][lay.pad(c)] == 0).all(), "%s form: %s is not zero on the padded rows of cloud %d" % (form, k, c)


@pytest.mark.parametrize("form", R.FORMS)
def test_padded_rows_are_zero_and_nothing_else_is_written(S, form):
    _assert_padding_zero(S.lay, form, S.f[form].bwd)


@pytest.mark.parametrize("form", R.FORMS)
def test_nan_in_the_padding_changes_nothing(S, form):
    """NaN in the padded rows of Q', K', V, O and dO: every real-row output of the three entry points bit for bit as without,
    padded gradients still exactly zero."""
    f, lay, rig = S.f[form], S.lay, S.rig
    nan = lambda a: _with_padding(lay, a, np.nan)
    dev = rig.load(form, nan(S.x["Q"]), nan(S.x["K"]), nan(S.x["V"]))
    qc, kc = _clouds(lay, form)
    assert _same_bits(rig.reduce(dev), f.kv), "kv_reduce"
    assert _same_bits(rig.apply(dev, f.img)[lay.real(qc)], f.att[lay.real(qc)]), "attn_apply"
    got = rig.bwd(dev, nan(f.O), nan(S.x["dO"]), f.img)
    for k in OUT:
        rows = lay.real(qc if k == "dq" else kc)
        assert _same_bits(got[k][rows], f.bwd[k][rows]), "attn_bwd: %s" % k
    _assert_padding_zero(lay, form, got)


# ------------------------------------------------------------------------------------- 6, 7: batching, determinism
@pytest.mark.parametrize("i", range(B))
def test_a_pair_alone_gets_the_rows_it_gets_in_the_batch(S, i):
    """Pair i as a batch of one (its own max_chunks, row bases and cloud numbers), in self and cross form: bit for bit."""
    lay = S.lay
    rig1 = Rig([R.SRC_LEN[i]], [R.TGT_LEN[i]])
    lay1 = rig1.lay
    twin = ((0, i), (1, B + i))  # (cloud of the batch of one, cloud of the batch of nine)

    def take(a):
        out = np.full((lay1.rt, 256), PAD, np.float32)
        for c1, c9 in twin:
            out[lay1.rows(c1)] = a[lay.rows(c9)]
        return out

    Q, K, V, dO = (take(S.x[k]) for k in ("Q", "K", "V", "dO"))
    for form in ("self", "cross"):
        f = S.f[form]
        img = np.stack([f.img[c9] for _, c9 in twin])
        dev = rig1.load(form, Q, K, V)
        kv, att, got = rig1.reduce(dev), rig1.apply(dev, img), rig1.bwd(dev, take(f.O), dO, img)
        qc, kc = _clouds(lay1, form)
        for c1, c9 in twin:
            if c1 in kc:
                assert _same_bits(kv[c1], f.kv[c9]), (form, "kv", c9)
                assert _same_bits(got["dk"][lay1.rows(c1)], f.bwd["dk"][lay.rows(c9)]), (form, "dk", c9)
                assert _same_bits(got["dv"][lay1.rows(c1)], f.bwd["dv"][lay.rows(c9)]), (form, "dv", c9)
            if c1 in qc:
                assert _same_bits(att[lay1.rows(c1)], f.att[lay.rows(c9)]), (form, "O", c9)
                assert _same_bits(got["dq"][lay1.rows(c1)], f.bwd["dq"][lay.rows(c9)]), (form, "dq", c9)


@pytest.mark.parametrize("form", R.FORMS)
def test_two_identical_calls_are_bitwise_equal(S, form):
    f, rig = S.f[form], S.rig
    assert _same_bits(rig.reduce(f.dev), f.kv)
    assert _same_bits(rig.apply(f.dev, f.img), f.att)
    got = rig.bwd(f.dev, f.O, S.x["dO"], f.img)
    assert all(_same_bits(got[k], f.bwd[k]) for k in OUT)
