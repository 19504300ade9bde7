"""tests/attn_ref.py, the float64 restatement that tests/test_gpu_attention_train.py holds the training attention kernels to, held
itself: against float64 autograd of the oracle, evaluated in fp32 numpy inside its own bar, against ten wrong restatements that
the bar must catch, and clear of subnormals and overflow.  No GPU needed."""
import numpy as np
import pytest
import torch

import attn_ref as R
from oracle import scream_ref as O
from scream_amd.packing import PackedBatch

OUT = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def case():
    lens, row0, rs, rt, _, max_chunks = PackedBatch.layout(R.SRC_LEN, R.TGT_LEN)
    assert max_chunks == 3
    lay = R.Layout(lens, row0, rs, rt)
    x = R.make_inputs(rt)
    ref = {}
    for form in R.FORMS:  # what assertion 1 of the GPU file compares with: O and kv are the float64 values rounded once
        img, O32 = R.forward_rounded(lay, form, x["Q"], x["K"], x["V"])
        ref[form] = dict(img=img, O=O32, kv=R.ref_reduce(lay, form, x["K"], x["V"]), att=R.ref_apply(lay, form, x["Q"], img),
                         bwd=R.ref_bwd(lay, form, x["Q"], x["K"], x["V"], O32, x["dO"], img))
    return lay, x, ref


def pair(case, form, qc, kc=None):
    """The arrays of one (query cloud, key cloud) of a form and its backward: what the wrong restatements are compared with."""
    lay, x, ref = case
    kc = dict(lay.pairs(form))[qc] if kc is None else kc
    ql, kl = lay.rows(qc), lay.rows(kc)
    KV, ks = R.kv_unimage(ref[form]["img"][kc])
    p = dict(Q=x["Q"][ql], K=x["K"][kl], V=x["V"][kl], O=ref[form]["O"][ql], dO=x["dO"][ql], KV=KV, ks=ks, L=lay.lens[qc], S=lay.lens[kc])
    p["want"] = R.attn_bwd(p["Q"], p["K"], p["V"], p["O"], p["dO"], KV, ks)
    return p


# ------------------------------------------------------------------------------------- against float64 autograd
class _Elu1:
    """What F.elu returns inside the oracle for this test: `+ 1` gives elu(x) + 1 = x + 1 for x > 0 and exp(x) otherwise, with the same
    derivative.  torch's own exp(x) - 1 + 1 is that function with an absolute error of 2^-54 in float64: a relative error of
    2^-54 / Q', which at Q' ~ exp(-8) already exceeds the 2 n 2^-53 of this test, and at exp(-36) ~ 2^-52 leaves no digit."""

    def __init__(self, x):
        self.x = x

    def __add__(self, one):
        assert one == 1
        return torch.where(self.x > 0, self.x + 1, torch.exp(self.x))


class _F:
    elu = staticmethod(_Elu1)


def test_patched_elu_is_the_oracles_elu_where_float64_can_tell(monkeypatch):
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(1, 40, 8, 32, generator=g, dtype=torch.float64) for _ in range(3))
    plain = O.linear_attention(q, k, v)
    monkeypatch.setattr(O, "F", _F)
    assert (O.linear_attention(q, k, v) - plain).abs().max() <= 1e-12 * plain.abs().max()


def test_restatement_against_float64_autograd(case, monkeypatch):
    """oracle.scream_ref.linear_attention differentiated through elu + 1, per pair of the self and the cross form (the target-side
    form's pairs are the self form's), on the inputs of the GPU file with Q', K', O and kv in float64 and not rounded: every element
    within 2 n 2^-53 A."""
    lay, x, _ = case
    monkeypatch.setattr(O, "F", _F)
    worst = {}
    for form in ("self", "cross"):
        for qc, kc in lay.pairs(form):
            q = torch.from_numpy(x["q"][lay.rows(qc)]).requires_grad_()
            k = torch.from_numpy(x["k"][lay.rows(kc)]).requires_grad_()
            v = torch.from_numpy(x["V"][lay.rows(kc)].astype(np.float64)).requires_grad_()
            dO = x["dO"][lay.rows(qc)].astype(np.float64)
            want = {}
            o = O.linear_attention(q.view(1, -1, 8, 32), k.view(1, -1, 8, 32), v.view(1, -1, 8, 32), want).view(-1, 256)
            (o * torch.from_numpy(dO)).sum().backward()
            Qp, Kp = want["Q"].detach().numpy().reshape(-1, 256), want["K"].detach().numpy().reshape(-1, 256)
            L, S = lay.lens[qc], lay.lens[kc]
            (KV, A_KV), (ks, A_ks) = R.kv_reduce(Kp, v.detach().numpy())
            att, A_att = R.attn_apply(Qp, KV, ks, S)
            got = R.attn_bwd(Qp, Kp, v.detach().numpy(), att, dO, KV, ks)
            checks = [("KV", KV, want["KV"][0].detach().numpy(), A_KV, R.chain("kv", S=S)),
                      ("ks", ks, want["Ksum"][0].detach().numpy(), A_ks, R.chain("kv", S=S)),
                      ("O", att, o.detach().numpy(), A_att, R.chain("O"))]
            checks += [(n, got[n][0], t.grad.numpy(), got[n][1], R.chain(n, L=L, S=S)) for n, t in zip(OUT, (q, k, v))]
            for name, mine, auto, A, n in checks:
                bad = R.misses(mine, auto, A, 2 * n, u=R.U64, tiny=0.0)
                assert not bad.any(), (form, qc, kc, name, R.worst(mine, auto, A, u=R.U64))
                worst[name] = max(worst.get(name, 0.0), R.worst(mine, auto, A, u=R.U64)[0])
    print("\nrestatement vs float64 autograd, worst err / (2^-53 A): %s" % {k: "%.1f" % v for k, v in worst.items()})


# ------------------------------------------------------------------------------------- the reference alone meets the bar
def test_restatement_in_fp32_numpy_stays_inside_the_bar(case, capsys):
    """The condition that the reference alone meets the bar: the same formulas in fp32 numpy, on every case of the GPU file."""
    lay, x, ref = case
    worst = {}
    for form in R.FORMS:
        f = ref[form]
        img32, _, _ = R.ref_reduce(lay, form, x["K"], x["V"], np.float32)
        att32, _ = R.ref_apply(lay, form, x["Q"], f["img"], np.float32)
        bwd32 = R.ref_bwd(lay, form, x["Q"], x["K"], x["V"], f["O"], x["dO"], f["img"], np.float32)
        checks = [("kv", img32, *f["kv"]), ("O", att32, *f["att"], R.chain("O"))] + [(k, bwd32[k][0], *f["bwd"][k]) for k in OUT]
        for name, got, want, A, n in checks:
            assert got.dtype == np.float32
            ratio, at = R.worst(got, want, A)
            assert not R.misses(got, want, A, n).any(), (form, name, ratio, at)
            worst[form, name] = ratio
    with capsys.disabled():
        print("\nfp32 numpy vs float64, worst err / (2^-24 A) per form and output (bars: kv S + 8, O 96, dq 128, dk and dv L + 128):")
        for form in R.FORMS:
            print("  %-5s %s" % (form, "  ".join("%s %.2f" % (n, worst[form, n]) for n in ("kv", "O") + OUT)))


# ------------------------------------------------------------------------------------- what the bar must catch
def _sums(p, rows=slice(None), S=None, extra=None):
    Q, O_, dO = p["Q"][rows], p["O"][rows], p["dO"][rows]
    if extra is not None:  # one more row of finite garbage, as the padding of today's tests holds
        Q, O_, dO = (np.concatenate([a, np.full((1, 256), extra, np.float32)]) for a in (Q, O_, dO))
    return R.attn_bwd_sums(Q, O_, dO, p["ks"], p["S"] if S is None else S)


def _rows(p, dKV, dks, S=None, KV=None, ks=None, eps=R.EPS):
    return R.attn_bwd_rows(p["Q"], p["K"], p["V"], p["O"], p["dO"], p["KV"] if KV is None else KV, p["ks"] if ks is None else ks,
                           dKV, dks, p["S"] if S is None else S, eps)


def _wrong_S(p):
    return _rows(p, *_sums(p, S=p["L"]), S=p["L"])


def _no_eps(p):
    return R.attn_bwd(p["Q"], p["K"], p["V"], p["O"], p["dO"], p["KV"], p["ks"], eps=0.0)


def _last_token_out(p):
    return _rows(p, *_sums(p, rows=slice(0, p["L"] - 1)))


def _padded_row_in(p):
    return _rows(p, *_sums(p, extra=3.0))


def _dkv_transposed(p):
    (dKV, A), dks = _sums(p)
    return _rows(p, (dKV.transpose(0, 2, 1), A.transpose(0, 2, 1)), dks)


def _dks_sign(p):
    dKV, (dks, A) = _sums(p)
    return _rows(p, dKV, (-dks, A))


def _elu_derivative_one(p):
    r = _rows(p, *_sums(p))
    return dict(r, dq=r["dQp"], dk=r["dKp"])


def _elu_derivative_without_min(p):
    r = _rows(p, *_sums(p))
    return dict(r, dq=(r["dQp"][0] * p["Q"], None), dk=(r["dKp"][0] * p["K"], None))


def _tokens_from_256_out(p):
    return _rows(p, *_sums(p, rows=slice(0, 256)))


B = len(R.SRC_LEN)
# (wrong restatement, form, query cloud, the outputs it must throw outside the bar there)
WRONG = [
    ("the backward uses the query cloud's length for S", _wrong_S, "cross", 2, ("dq",)),              # L 7, S 15; S cancels in dk and dv
    ("1e-6 dropped from Z", _no_eps, "self", 3, OUT),                                                 # 9 rows; Q'.ks << 1e-6 in head 5
    ("the last token of an odd-length cloud left out of dKV / dks", _last_token_out, "self", 2, ("dk", "dv")),  # 7 rows
    ("one padded row included in dKV / dks", _padded_row_in, "self", 1, ("dk", "dv")),                # 2 rows
    ("dKV read transposed", _dkv_transposed, "self", 4, ("dk", "dv")),                                # 31 rows
    ("dks with the wrong sign", _dks_sign, "self", 5, ("dk",)),                                       # 32 rows
    ("elu's derivative taken as 1", _elu_derivative_one, "self", 6, ("dq", "dk")),                    # 33 rows
    ("elu's derivative taken as Q' without the min", _elu_derivative_without_min, "self", 7, ("dq", "dk")),  # 127 rows
    ("the kv of the neighbouring cloud used", None, "cross", 3, ("dq",)),                             # key cloud B + 4 for B + 3
    ("tokens from 256 on left out of a 257-row cloud", _tokens_from_256_out, "self", B, ("dk", "dv")),  # the first target cloud
]


@pytest.mark.parametrize("what,wrong,form,qc,outputs", WRONG, ids=[w[0] for w in WRONG])
def test_bar_catches_a_wrong_restatement(case, capsys, what, wrong, form, qc, outputs):
    lay = case[0]
    p = pair(case, form, qc)
    if wrong is None:  # offset off by one: the image of key cloud kc + 1
        KV, ks = R.kv_unimage(case[2][form]["img"][dict(lay.pairs(form))[qc] + 1])
        got = _rows(p, *R.attn_bwd_sums(p["Q"], p["O"], p["dO"], ks, p["S"]), KV=KV, ks=ks)
    else:
        got = wrong(p)
    shown = {}
    for k in outputs:
        want, A = p["want"][k]
        assert R.misses(got[k][0], want, A, R.chain(k, L=p["L"], S=p["S"])).any(), (what, form, qc, k)
        shown[k] = "%.3g" % R.worst(got[k][0], want, A)[0]
    with capsys.disabled():
        print("\n%s: caught on the %s form, query cloud %d (L %d, S %d); worst err / (2^-24 A) %s against bars of %d (dq) and %d (dk, dv)"
              % (what, form, qc, p["L"], p["S"], shown, R.chain("dq"), R.chain("dk", L=p["L"])))


# ------------------------------------------------------------------------------------- range, layout
def test_cases_stay_clear_of_subnormals_and_overflow(case):
    lay, x, ref = case
    for form in R.FORMS:
        f = ref[form]
        for name, (want, A) in [("kv", f["kv"][:2]), ("O", f["att"])] + [(k, f["bwd"][k][:2]) for k in OUT]:
            assert np.isfinite(want).all() and np.isfinite(A).all()
            assert (A[A != 0] >= 2.0 ** -100).all(), (form, name, A[A != 0].min())
            assert (np.abs(want) < 2.0 ** 100).all(), (form, name, np.abs(want).max())
            assert (np.abs(want) <= A * (1 + 1e-12)).all()  # a magnitude companion bounds its value
        own_q, own_k = (lay.real([c[i] for c in lay.pairs(form)]) for i in (0, 1))
        assert (f["bwd"]["dq"][1][own_q] > 0).all() and (f["bwd"]["dk"][1][own_k] > 0).all() and (f["bwd"]["dv"][1][own_k] > 0).all()
    head = lambda a, h: a.reshape(-1, 8, 32)[lay.real(range(2 * B)), h]
    den = np.einsum("ld,d->l", head(x["Q"], 5)[:1].astype(np.float64), head(x["K"], 5).astype(np.float64).sum(0))
    assert den[0] < 1e-12  # Q' . ks far below the 1e-6 of Z in head 5, even summed over every key row of the batch


def test_image_and_row_helpers():
    rng = np.random.default_rng(0)
    KV, ks = rng.standard_normal((8, 32, 32)), rng.standard_normal((8, 32))
    img = R.kv_image(KV, ks)
    assert img.shape == (8, R.KV_ELEMS)
    assert img[3, 5 * 32 + 7] == KV[3, 7, 5] and img[3, 1024 + 9] == ks[3, 9]  # KV[d][v] sits at [v][d]; ks follows
    KV2, ks2 = R.kv_unimage(img)
    assert np.array_equal(KV2, KV) and np.array_equal(ks2, ks)
    lens, row0, rs, rt, tile_cloud, _ = PackedBatch.layout([1, 129], [257, 8])
    lay = R.Layout(lens, row0, rs, rt)
    assert lay.rows(1) == slice(128, 257) and lay.pad(1) == slice(257, 384) and lay.where(130) == (1, 2)
    assert lay.pairs("cross") == [(0, 2), (1, 3)] and lay.row_ranges("tself") == ((384, 896), (384, 896))
    assert lay.real([0, 3]).sum() == 9 and rt == 896
