"""The contract of scream_kv_reduce, scream_attn_apply (csrc/attention.hip) and scream_attn_bwd (csrc/backward.hip) in float64,
in closed form: plain numpy, no autograd.  Every formula is a function of exactly the fp32 arrays the kernel is handed; the
backward is handed O and the kv image, so its restatement takes them too and does not recompute them.

One (query cloud of L rows, key cloud of S rows) and one head, Q' [L, 32], K' / V [S, 32], dO / O [L, 32]:

  reduce    KV[d][v] = sum_s K'[s,d] (V[s,v] / S)        ks[d] = sum_s K'[s,d]
  apply     Z_l = 1 / (Q'_l . ks + 1e-6)                 O_l = S Z_l Q'_l KV
  backward  dKV = sum_l S Z_l Q'_l^T dO_l                dks = -sum_l Z_l (dO_l . O_l) Q'_l
            dQ'_l = S Z_l dO_l KV^T - Z_l (dO_l . O_l) ks
            dK'_s = (V_s / S) dKV^T + dks                dV_s = K'_s dKV / S
            dq = dQ' min(Q', 1)                          dk = dK' min(K', 1)        (elu + 1 backward from its output)

Beside every output stands its MAGNITUDE COMPANION A: the same formula with every term replaced by its absolute value.  The
denominators of Z keep their sign (sums of positive terms), dO . O becomes sum |dO O|, the subtraction in dQ' and the addition in
dK' become additions of magnitudes.

THE BAR, element by element:   |got - want| <= n 2^-24 A + n 2^-149

Every kernel here is fp32 with one rounding per operation (no fast-math, correctly rounded division; the fp32-input MFMA is a
k-ordered fmaf chain that keeps subnormals), so a result that passes through at most n rounded operations, each of relative
error 2^-24 or -- where it underflows -- absolute error 2^-149, is within (1 + 2^-24)^n - 1 of A in relative terms whatever the
order of the sums.  n is the CHAIN COUNT below; each is a round upper bound of what the code does (counted beside it), with enough
room for the second-order terms ((1 + u)^k - 1 <= 1.0001 k u for k u < 1e-4, and every count below has more than 4 to spare).
Nothing here is sized from a measured error.

Chain counts, from the code (longest path of rounded operations to one element):

  KV, ks   S + 8.   kv_partial_kernel: V / S (1), one fma per token on the MFMA's chain, at most 256 per chunk, then
           kv_final_kernel adds the ceil(S / 256) chunk partials: at most 1 + S + ceil(S / 256).  ks: one add per token of its half
           wave (at most 128 per chunk), the add across the two halves (1), the chunk adds.  Both <= S + 4 for S <= 768.
  O        96.  attn_apply_kernel: the numerator is 32 fmas on the MFMA chain; Z is a product (1), 16 adds in its half wave, the add
           across halves (1), the 1e-6f that is itself 1e-6 rounded to fp32 (1), its addition (1), the division (1) = 21; then
           (acc * Z) * S (2): 55.
  dq       128.  attn_bwd_q_kernel: Z is a product (1), five shuffle adds (5), the rounded 1e-6f, its addition, the division (3) = 9;
           dO . O a product and five adds (6); dO KV^T a product and 32 adds (33), S * Z (1), times the dot (1): 44 with Z; the other
           term (Z * go) * ks is 9 + 6 + 2; the subtraction (1), min(Q', 1) (1): 46.
  dk, dv   L + 128, L the number of query rows summed.  attn_bwd_partial_kernel: Z (9), S * Z (1), times Q' (1), one fma per query
           row on the MFMA chain (at most 256 per chunk), attn_bwd_final_kernel's chunk adds (ceil(L / 256)): dKV <= L + 14 for
           L <= 768; dks: Z (9), dO . O (6), Z * go (1), times Q' and the subtraction (2), at most 128 tokens per half and chunk, the
           add across halves, the chunk adds: shorter.  attn_bwd_kv_kernel: a product and 32 adds over dKV (33), 1 / S and the
           multiplication by it (2), + dks (1), min(K', 1) (1): dk <= L + 51, dv <= L + 49.

Layout: a kv image holds, per (cloud, head) and cloud-major, KV stored as [v][d] (1024 floats) and then ks (32): 1056 floats.
Packed rows: cloud c owns rows [row0[c], row0[c] + len[c]) of a [rows, 256] array, head h in columns 32 h .. 32 h + 31.
"""
import numpy as np

HD, NH, D = 32, 8, 256
KV_ELEMS = (HD + 1) * HD
EPS = 1e-6
U32, TINY32, U64 = 2.0 ** -24, 2.0 ** -149, 2.0 ** -53

# ------------------------------------------------------------------------------------- the batch of the attention tests
# Both sides of the half-wave token split (1, 2), of the 8-token trip of the backward (7, 8, 9), of the 16-token trip of the reduce
# (15, 16, 17), of the 32-row sub-tile (31, 32, 33), of the 128-row tile (127, 128, 129) and of the 256-token chunk (255, 256, 257);
# 513 is three chunks beside clouds of one, under max_chunks = 3.
SRC_LEN = [1, 2, 7, 9, 31, 32, 33, 127, 129]
TGT_LEN = [257, 8, 15, 16, 17, 256, 128, 255, 513]
Q_SHIFT = (0, 0, 8, 16, 24, 36, 0, 8)   # head h of q sits this far down: Q' ~ exp(-shift)
K_SHIFT = Q_SHIFT[-3:] + Q_SHIFT[:-3]   # (36, 0, 8, 0, 0, 8, 16, 24): tiny K' only in heads 0 and 6, tiny Q' only in 3 and 4, both in 2, 5, 7
DO_SCALE = {6: 2.0 ** 16, 3: 2.0 ** -20}  # a loss scale on one head of dO, a vanishing gradient on another
FORMS = ("self", "cross", "tself")


def elu1(x):
    """elu(x) + 1 without the cancellation of exp(x) - 1 + 1."""
    return np.where(x > 0, x + 1, np.exp(np.minimum(x, 0)))


def make_inputs(rows, seed=20):
    """Pre-activations q, k ~ N(0, 0.7) shifted per head (float64), Q' and K' = elu + 1 in float64 rounded once, V and dO ~ N(0, 1)
    with dO's heads scaled by DO_SCALE: [rows, 256] each, every row filled (the caller owns the padding)."""
    rng = np.random.default_rng(seed)
    q = 0.7 * rng.standard_normal((rows, NH, HD)) - np.array(Q_SHIFT, np.float64)[None, :, None]
    k = 0.7 * rng.standard_normal((rows, NH, HD)) - np.array(K_SHIFT, np.float64)[None, :, None]
    V = rng.standard_normal((rows, NH, HD)).astype(np.float32)
    dO = rng.standard_normal((rows, NH, HD)).astype(np.float32)
    for h, s in DO_SCALE.items():
        dO[:, h] *= np.float32(s)
    f = lambda a: np.ascontiguousarray(a.reshape(rows, D))
    return dict(q=f(q), k=f(k), Q=f(elu1(q).astype(np.float32)), K=f(elu1(k).astype(np.float32)), V=f(V), dO=f(dO))


class Layout:
    """PackedBatch.layout's (lens, row0, rows_src, rows_total, ...) and what the three call forms make of it."""

    def __init__(self, lens, row0, rows_src, rows_total):
        self.lens, self.row0 = [int(x) for x in lens], [int(x) for x in row0]
        self.rs, self.rt, self.B = int(rows_src), int(rows_total), len(lens) // 2

    def rows(self, c):
        return slice(self.row0[c], self.row0[c] + self.lens[c])

    def pad(self, c):
        return slice(self.row0[c] + self.lens[c], self.row0[c] + (self.lens[c] + 127) // 128 * 128)

    def pairs(self, form):
        """(query cloud, key cloud) of the form: self over all 2B clouds; cross: queries [0, B), keys B + c; target-side self."""
        B = self.B
        return {"self": [(c, c) for c in range(2 * B)], "cross": [(c, B + c) for c in range(B)],
                "tself": [(c, c) for c in range(B, 2 * B)]}[form]

    def row_ranges(self, form):
        """((first, end) of the query rows, (first, end) of the key rows) that the form's calls own."""
        rs, rt = self.rs, self.rt
        return {"self": ((0, rt), (0, rt)), "cross": ((0, rs), (rs, rt)), "tself": ((rs, rt), (rs, rt))}[form]

    def real(self, clouds):
        m = np.zeros(self.rt, bool)
        for c in clouds:
            m[self.rows(c)] = True
        return m

    def where(self, row):
        """(cloud, row within the cloud) of a packed row."""
        c = max(i for i in range(2 * self.B) if self.row0[i] <= row)
        return c, row - self.row0[c]


# ------------------------------------------------------------------------------------- one pair, all heads
def _h(a, dtype):
    return np.asarray(a).reshape(-1, NH, HD).astype(dtype)


def kv_reduce(K, V, dtype=np.float64):
    """K', V [S, 256] -> (KV [8, d, v], A), (ks [8, d], A)."""
    K, V = _h(K, dtype), _h(V, dtype)
    Vs = V / dtype(K.shape[0])
    return ((np.einsum("shd,shv->hdv", K, Vs), np.einsum("shd,shv->hdv", np.abs(K), np.abs(Vs))),
            (K.sum(0), np.abs(K).sum(0)))


def _z(Q, ks, eps, dtype):
    return dtype(1) / (np.einsum("lhd,hd->lh", Q, ks) + dtype(eps))


def attn_apply(Q, KV, ks, S, eps=EPS, dtype=np.float64):
    """Q' [L, 256], KV [8, d, v], ks [8, d], S the key cloud's length -> (O [L, 256], A)."""
    Q, KV, ks = _h(Q, dtype), KV.astype(dtype), ks.astype(dtype)
    sz = dtype(S) * _z(Q, ks, eps, dtype)
    O = sz[..., None] * np.einsum("lhd,hdv->lhv", Q, KV)
    A = sz[..., None] * np.einsum("lhd,hdv->lhv", np.abs(Q), np.abs(KV))
    return O.reshape(-1, D), A.reshape(-1, D)


def attn_bwd_sums(Q, O, dO, ks, S, eps=EPS, dtype=np.float64):
    """Phase 1, over the query rows given: (dKV [8, d, v], A), (dks [8, d], A)."""
    Q, O, dO, ks = _h(Q, dtype), _h(O, dtype), _h(dO, dtype), ks.astype(dtype)
    Z = _z(Q, ks, eps, dtype)
    go, ago = np.einsum("lhv,lhv->lh", dO, O), np.einsum("lhv,lhv->lh", np.abs(dO), np.abs(O))
    sz = dtype(S) * Z
    return ((np.einsum("lh,lhd,lhv->hdv", sz, Q, dO), np.einsum("lh,lhd,lhv->hdv", sz, np.abs(Q), np.abs(dO))),
            (-np.einsum("lh,lhd->hd", Z * go, Q), np.einsum("lh,lhd->hd", Z * ago, np.abs(Q))))


def attn_bwd_rows(Q, K, V, O, dO, KV, ks, dKV, dks, S, eps=EPS, dtype=np.float64):
    """Phase 2.  dKV, dks: the (value, A) pairs of attn_bwd_sums.  Returns name -> (value, A) for dq, dk, dv [rows, 256], and
    for dQ', dK' (as 'dQp', 'dKp') before elu's derivative."""
    Q, K, V, O, dO = (_h(a, dtype) for a in (Q, K, V, O, dO))
    KV, ks = KV.astype(dtype), ks.astype(dtype)
    (dKV, A_dKV), (dks, A_dks) = ((a.astype(dtype), b.astype(dtype)) for a, b in (dKV, dks))
    S = dtype(S)
    Z = _z(Q, ks, eps, dtype)
    go, ago = np.einsum("lhv,lhv->lh", dO, O), np.einsum("lhv,lhv->lh", np.abs(dO), np.abs(O))
    dQp = (S * Z)[..., None] * np.einsum("lhv,hdv->lhd", dO, KV) - (Z * go)[..., None] * ks
    A_dQp = (S * Z)[..., None] * np.einsum("lhv,hdv->lhd", np.abs(dO), np.abs(KV)) + (Z * ago)[..., None] * np.abs(ks)
    Vs = V / S
    dKp = np.einsum("shv,hdv->shd", Vs, dKV) + dks
    A_dKp = np.einsum("shv,hdv->shd", np.abs(Vs), A_dKV) + A_dks
    dV = np.einsum("shd,hdv->shv", K, dKV) / S
    A_dV = np.einsum("shd,hdv->shv", np.abs(K), A_dKV) / S
    mq, mk = np.minimum(Q, dtype(1)), np.minimum(K, dtype(1))
    out = dict(dQp=(dQp, A_dQp), dKp=(dKp, A_dKp), dq=(dQp * mq, A_dQp * mq), dk=(dKp * mk, A_dKp * mk), dv=(dV, A_dV))
    return {k: (a.reshape(-1, D), b.reshape(-1, D)) for k, (a, b) in out.items()}


def attn_bwd(Q, K, V, O, dO, KV, ks, eps=EPS, dtype=np.float64):
    """scream_attn_bwd on one pair: name -> (value, A) for dq [L, 256], dk, dv [S, 256]."""
    S = np.asarray(K).shape[0]
    dKV, dks = attn_bwd_sums(Q, O, dO, ks, S, eps, dtype)
    r = attn_bwd_rows(Q, K, V, O, dO, KV, ks, dKV, dks, S, eps, dtype)
    return {k: r[k] for k in ("dq", "dk", "dv")}


def chain(name, L=0, S=0):
    """The chain count n of one output (module docstring)."""
    return {"kv": S + 8, "O": 96, "dq": 128, "dk": L + 128, "dv": L + 128}[name]


# ------------------------------------------------------------------------------------- the bar
def bar(A, n, u=U32, tiny=TINY32):
    return n * u * A + n * tiny


def misses(got, want, A, n, u=U32, tiny=TINY32):
    """Boolean array: the elements outside the bar (a NaN or an infinity is outside)."""
    return ~(np.abs(np.asarray(got, np.float64) - want) <= bar(A, n, u, tiny))


def worst(got, want, A, u=U32):
    """(largest err / (u A), its index).  An error where A == 0 counts as infinite, none there as zero."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, err / (u * A), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    if r.size == 0:
        return 0.0, ()
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(x) for x in i)


# ------------------------------------------------------------------------------------- images and packed rows
def kv_image(KV, ks):
    """KV [8, d, v], ks [8, d] -> [8, 1056]: KV as [v][d], then ks."""
    return np.concatenate([KV.transpose(0, 2, 1).reshape(NH, HD * HD), ks], axis=1)


def kv_unimage(img):
    """[8, 1056] -> KV [8, d, v], ks [8, d]."""
    img = np.asarray(img).reshape(NH, KV_ELEMS)
    return img[:, :HD * HD].reshape(NH, HD, HD).transpose(0, 2, 1), img[:, HD * HD:]


def ref_reduce(lay, form, K, V, dtype=np.float64):
    """scream_kv_reduce of a form on packed K', V [rows_total, 256]: (image [2B, 8, 1056], A, n [2B, 1, 1]); zero for a cloud
    that is no key cloud of the form."""
    img, A, n = (np.zeros((2 * lay.B, NH, KV_ELEMS), dtype), np.zeros((2 * lay.B, NH, KV_ELEMS)), np.zeros((2 * lay.B, 1, 1)))
    for _, kc in lay.pairs(form):
        (KV, A_KV), (ks, A_ks) = kv_reduce(K[lay.rows(kc)], V[lay.rows(kc)], dtype)
        img[kc], A[kc], n[kc] = kv_image(KV, ks), kv_image(A_KV, A_ks), chain("kv", S=lay.lens[kc])
    return img, A, n


def ref_apply(lay, form, Q, img, dtype=np.float64):
    """scream_attn_apply of a form on packed Q' and a kv image: (O [rows_total, 256], A); zero outside the form's real query rows."""
    O, A = np.zeros((lay.rt, D), dtype), np.zeros((lay.rt, D))
    for qc, kc in lay.pairs(form):
        KV, ks = kv_unimage(img[kc])
        O[lay.rows(qc)], A[lay.rows(qc)] = attn_apply(Q[lay.rows(qc)], KV, ks, lay.lens[kc], dtype=dtype)
    return O, A


def forward_rounded(lay, form, Q, K, V):
    """The float64 forward of the fp32 Q', K', V, rounded once at its end: (kv image, O) in fp32, as a test hands them to the
    backward or to the apply alone."""
    img, _, _ = ref_reduce(lay, form, K, V)
    O, _ = ref_apply(lay, form, Q, img)
    return img.astype(np.float32), O.astype(np.float32)


def ref_bwd(lay, form, Q, K, V, O, dO, img, dtype=np.float64):
    """scream_attn_bwd of a form on packed rows: name -> (value [rows_total, 256], A, n [rows_total, 1]) for dq, dk, dv; zero outside
    the form's real rows."""
    out = {k: (np.zeros((lay.rt, D), dtype), np.zeros((lay.rt, D)), np.zeros((lay.rt, 1))) for k in ("dq", "dk", "dv")}
    for qc, kc in lay.pairs(form):
        ql, kl = lay.rows(qc), lay.rows(kc)
        KV, ks = kv_unimage(img[kc])
        r = attn_bwd(Q[ql], K[kl], V[kl], O[ql], dO[ql], KV, ks, dtype=dtype)
        for k, sl in (("dq", ql), ("dk", kl), ("dv", kl)):
            out[k][0][sl], out[k][1][sl] = r[k]
            out[k][2][sl] = chain(k, L=lay.lens[qc], S=lay.lens[kc])
    return out
