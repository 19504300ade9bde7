"""Yardstick of the pose back end (1-NN search, Kabsch solve, RE/TE, the ICP search): exact and float64 references in plain
numpy, the case sets, and the bars the kernels are held to.  Nothing here imports scream_amd or touches a GPU; the references
are themselves held by tests/test_pose_ref_host.py before tests/test_gpu_pose_backend.py holds the kernels with them.

Exact lattice arithmetic.  Clouds whose coordinates are multiples of 1/4 with |x| <= 64, searched with s a power of two: every
quotient, product and sum of the kernel's fp32 sequence (|a|^2, a.b, -2 a.b + |a|^2, + |b|^2) is an integer multiple of 2^-4
below 2^16 (fewer than 2^20 units of 2^-4, where fp32 holds 2^24) and therefore exact in fp32, whatever the order.  The reference is integer arithmetic in int64: the exact
squared distance, arg-min to the LOWEST index, valid = d < thresh.  (`lattice_nn` checks the magnitude condition itself, so finer
lattices over a smaller range -- the ICP problem uses multiples of 1/8 -- are accepted when they are exact too.)

The Kabsch bar (kabsch_f64, kabsch_bar).  With R64 | t64 the float64 solve from the same fp32 inputs, sigma_1..3 the singular
values of its H, delta = det(V U^T) and S = sum_i w_i |a_i - cA| |b_i - cB|:
    |R - R64|_F <= C_R * 2^-24 * S / (sigma_2 + delta sigma_3) + 4 * 2^-24
    |t - t64|   <= |R - R64|_F * |cA| + C_T * 2^-24 * (|cA| + |cB|)
The first term of the rotation bar is the fp32 rounding of H (each term of H is rounded at 2^-24 of |a_i - cA| |b_i - cB|)
times the sensitivity of the polar factor, 1 / (sigma_2 + delta sigma_3) up to a constant; the second is the fp32 output.  A case
whose 2^-24 * S / (sigma_2 + delta sigma_3) exceeds 1e-3 has a rotation that the reference does not determine either: such
cases are listed as properness-only in the table (finite, R R^T = I and det = 1 to 1e-6, the centroid of A mapped onto the centroid of
B within the translation bar).  Which of the two a case is, is a column of the table; test_pose_ref_host.py checks that column
against the float64 reference.  Nothing is decided from a kernel's output and no case is skipped at run time.
"""
import zlib

import numpy as np

EPS32 = 2.0 ** -24
WELL_POSED_LIMIT = 1e-3

# C_R, C_T: four times the worst ratio of the reference's OWN fp32 path (oracle.scream_ref.rigid_transform_3d on the CPU, torch.svd
# = LAPACK) to the two expressions above, over every well-posed case of kabsch_case_table().  A kernel that carries its sums in fp64
# should sit below that path; one that loses more than four times what the reference loses has a defect.  Measured with
#     python tests/test_pose_ref_host.py
# (no GPU): worst rotation ratio 10.9 (case iso/2: |R32 - R64|_F = 1.3e-6, LAPACK's fp32 SVD), worst translation ratio 1.78 (case scale_-20/2);
# the two constants are those figures times four, rounded up to two digits.  tests/test_pose_ref_host.py re-measures the ratios and
# fails if they have moved by more than a factor of two, i.e. if the constants no longer follow from the measurement.
ORACLE_RATIO_R = 10.9
ORACLE_RATIO_T = 1.78
C_R = 44.0
C_T = 7.2


def case_rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def axis_angle(axis, deg):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


# ------------------------------------------------------------------------------------------------ exact lattice search
def lattice_cloud(rng, n, step=0.25, lim=64.0):
    """n points whose coordinates are multiples of `step` in [-lim, lim], fp32."""
    k = int(round(lim / step))
    return (rng.integers(-k, k + 1, size=(n, 3)) * step).astype(np.float32)


def _to_int(x, s, step):
    v = np.asarray(x, dtype=np.float64).reshape(-1, 3) / float(s) / step
    i = np.rint(v).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), v), "not on the lattice of step %g after / s" % step
    return i


def lattice_nn(query, target, s=1.0, thresh=np.inf, step=0.25, chunk=256, ties="lowest", strict=True, count_ties=False):
    """Exact thresholded 1-NN of lattice clouds in int64.  Returns (dmin fp32, idx int64, valid bool[, number of targets at the
    minimum]); an empty target cloud gives (+inf, -1, False).  ties="highest" and strict=False are the deliberately wrong variants
    the host tests prove the comparison can see."""
    q, t = _to_int(query, s, step), _to_int(target, s, step)
    n, m = len(q), len(t)
    big = max(int(np.abs(q).max()) if n else 0, int(np.abs(t).max()) if m else 0)
    assert 12 * big * big < 2 ** 24, "beyond the range where the fp32 sequence is exact"
    unit = step * step
    thr = np.float64(np.float32(thresh))
    dmin = np.full(n, np.inf, dtype=np.float32)
    idx = np.full(n, -1, dtype=np.int64)
    nties = np.zeros(n, dtype=np.int64)
    if m:
        for i0 in range(0, n, chunk):
            d = ((q[i0:i0 + chunk, None, :] - t[None, :, :]) ** 2).sum(axis=2)
            lo = d.min(axis=1)
            hit = d == lo[:, None]
            nties[i0:i0 + chunk] = hit.sum(axis=1)
            idx[i0:i0 + chunk] = hit.argmax(axis=1) if ties == "lowest" else m - 1 - hit[:, ::-1].argmax(axis=1)
            dmin[i0:i0 + chunk] = (lo * unit).astype(np.float32)  # exact: an integer below 2^24 times a power of two
    dd = dmin.astype(np.float64)
    valid = (dd < thr) if strict else (dd <= thr)
    return (dmin, idx, valid, nties) if count_ties else (dmin, idx, valid)


def lattice_square_distance(a, b, step=0.25):
    """Exact [B,N,M] squared distances of lattice batches, fp32."""
    out = []
    for x, y in zip(a, b):
        xi, yi = _to_int(x, 1.0, step), _to_int(y, 1.0, step)
        out.append((((xi[:, None, :] - yi[None, :, :]) ** 2).sum(axis=2) * (step * step)).astype(np.float32))
    return np.stack(out)


# The target-range split of scream_nn_search, restated (csrc/nn_search.hip: QB queries per block, RT targets per LDS tile, the
# split count in [1, 64] that minimises rounds of 256 blocks x (targets per split + 64)).  A block scans its split in tiles of RT
# targets, so ties ACROSS a tile edge exist only where a split is longer than RT: the tests that claim that edge ask this function
# for the geometry of their call and assert it.  test_pose_ref_host.py holds the copy against recorded plans and against the
# source lines it restates, so a retune of the kernel's heuristic fails there instead of silently removing the coverage.
NN_QB, NN_RT = 1024, 1024


def nn_split_plan(max_q_len, max_r_len, n_pairs):
    """(targets per split, number of splits) of one scream_nn_search call."""
    qblocks = (max_q_len + NN_QB - 1) // NN_QB
    max_splits = min((max_r_len + 255) // 256, 64)
    splits, best = 1, None
    for sp in range(1, max(max_splits, 1) + 1):
        blocks, per = qblocks * sp * n_pairs, (max_r_len + sp - 1) // sp
        cost = ((blocks + 255) // 256) * (per + 64)
        if best is None or cost < best:
            best, splits = cost, sp
    per = (max_r_len + splits - 1) // splits
    return per, (max_r_len + per - 1) // per


# (max_q_len, max_r_len, n_pairs) of the calls of tests/test_gpu_pose_backend.py that pin ties across an LDS tile edge: each has
# splits longer than one tile (the host test checks that), so a block carries best / bi from one tile into the next.
TILE_EDGE_CALLS = {"identical": (64, 2100, 256), "planted": (64, 2100, 256), "tie_lattice": (5000, 5832, 64), "negative": (1500, 12000, 64)}


TIE_SIDE = 18  # targets: the 18^3 = 5832 integer lattice points of a cube


def tie_lattice(seed=0):
    """Targets on the integer lattice in shuffled order (M = 5832); queries at body centres of its cells (8 equidistant nearest
    targets), face centres (4) and edge centres (2), N = 5000.  Returns (queries, targets, ties expected per query)."""
    rng = np.random.default_rng(seed)
    g = np.arange(TIE_SIDE) - TIE_SIDE // 2
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    t = t[rng.permutation(len(t))]
    parts, want = [], []
    for n, halves, ties in ((3000, 3, 8), (1000, 2, 4), (1000, 1, 2)):
        base = rng.integers(g[0], g[-1], size=(n, 3)).astype(np.float64)  # a cell's low corner: the +1 neighbours exist
        off = np.zeros((n, 3))
        for i in range(n):
            off[i, rng.permutation(3)[:halves]] = 0.5
        parts.append(base + off)
        want.append(np.full(n, ties))
    order = rng.permutation(5000)
    return np.concatenate(parts)[order].astype(np.float32), t.astype(np.float32), np.concatenate(want)[order]


def coincident_far_cloud(seed=0, n=6000):
    """The negative-distance case: queries at |x| ~ 100, NOT on a lattice; the targets are a copy of them and a second copy moved
    by one ulp per coordinate, shuffled together (M = 2 n).  The expanded form |a|^2 - 2 a.b + |b|^2 of a point against itself
    or its one-ulp neighbour is a rounding residue of either sign (multiples of 2^-9 here), so minima are negative for about
    four queries in ten and equal minima between the two copies are common."""
    rng = np.random.default_rng(seed)
    q = (rng.uniform(-1, 1, size=(n, 3)) + 100.0 * np.sign(rng.uniform(-1, 1, size=(n, 3)))).astype(np.float32)
    t = np.concatenate([q, np.nextafter(q, np.float32(0))])
    return q, t[rng.permutation(2 * n)].copy()


def icp_lattice_problem(seed=0):
    """Metric-frame ICP search problem (s = 1, c = 0, T0 = I, radius 0.5) on the lattice of step 1/8.  Targets: a 12^3 block of
    spacing 1/4 (shuffled), a few isolated points, among them one at the cloud's minimum corner and points at multiples of the
    radius.  Sources: body centres of the block's cells (8 ties at d^2 = 3/64), points at exactly the radius from an isolated
    target (d^2 == thresh: no correspondence), points just inside it, and points with no target within the radius."""
    rng = np.random.default_rng(seed)
    g = np.arange(12) * 0.25
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    lone = np.array([[-4.0, -4.0, -4.0], [6.0, 0.0, 0.0], [6.0, 2.0, 0.5], [0.0, 6.0, 1.5], [0.5, 6.0, 5.0], [5.0, 5.0, 6.0]])
    tgt = np.concatenate([block, lone])
    tgt = tgt[rng.permutation(len(tgt))]
    body = rng.integers(0, 11, size=(700, 3)) * 0.25 + 0.125
    axes = np.eye(3)
    at_radius = np.concatenate([lone + 0.5 * axes[i % 3] * (1 if i % 2 else -1) for i in range(6)])
    inside = np.concatenate([lone + 0.375 * axes[(i + 1) % 3] for i in range(3)])
    nowhere = lone + np.array([1.0, 1.0, 1.0])
    src = np.concatenate([body, at_radius, inside, nowhere])
    src = src[rng.permutation(len(src))]
    return src.astype(np.float32), tgt.astype(np.float32), 0.5


def icp_lattice_ref(src, tgt, radius):
    """(exact inlier count, exact RMSE as float64) of the search of the problem above at T = I."""
    d, _, valid = lattice_nn(src, tgt, 1.0, np.float32(radius) * np.float32(radius), step=0.125)
    cnt = int(valid.sum())
    return cnt, (float(np.sqrt(d[valid].astype(np.float64).sum() / cnt)) if cnt else 0.0)


# ------------------------------------------------------------------------------------------------------ Kabsch, float64
def kabsch_f64(A, B, w=None, thr=0.0, det_fix=True):
    """utils.py:138-178 in float64 from the same fp32 inputs: A, B [K,3], w [K] or None.  Returns a dict: T (4x4), R, t, sig (3),
    delta (+-1), S = sum w |a - cA| |b - cB|, ncA = |cA|, ncB = |cB|, cA, cB, cond = 2^-24 S / (sigma_2 + delta sigma_3)."""
    A = np.asarray(A, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    B = np.asarray(B, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    w = np.ones(len(A)) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64).copy()
    w[w < np.float64(np.float32(thr))] = 0.0
    wsum = w.sum() + 1e-6
    cA, cB = (A * w[:, None]).sum(axis=0) / wsum, (B * w[:, None]).sum(axis=0) / wsum
    Am, Bm = A - cA, B - cB
    H = Am.T @ (w[:, None] * Bm)
    U, sig, Vt = np.linalg.svd(H)
    V = Vt.T
    delta = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, delta if det_fix else 1.0]) @ U.T
    t = cB - R @ cA
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    S = float((w * np.linalg.norm(Am, axis=1) * np.linalg.norm(Bm, axis=1)).sum())
    gap = sig[1] + delta * sig[2]
    cond = EPS32 * S / gap if gap > 0 else np.inf
    return dict(T=T, R=R, t=t, sig=sig, delta=delta, S=S, ncA=float(np.linalg.norm(cA)), ncB=float(np.linalg.norm(cB)), cA=cA, cB=cB,
                cond=cond, H=H)


def gather_corr(src, ref, row0, n, ref_row0, idx, valid, s, c):
    """The correspondences of one packed pair as the reference forms them (evaluate_3d_match.py:96-101): rows of src with valid
    set, partners ref[idx] (idx None: the same row of ref, counted from ref_row0), both x / s + c rounded to fp32 per operation."""
    s32, c32 = np.float32(s), np.asarray(c, dtype=np.float32)
    rows = np.nonzero(np.asarray(valid[row0:row0 + n]) != 0)[0]
    partner = rows if idx is None else np.asarray(idx[row0:row0 + n])[rows]
    A = (np.asarray(src, dtype=np.float32)[row0 + rows] / s32).astype(np.float32) + c32
    B = (np.asarray(ref, dtype=np.float32)[ref_row0 + partner] / s32).astype(np.float32) + c32
    return A.astype(np.float32), B.astype(np.float32)


def kabsch_bar(ref, c_r=None, c_t=None):
    """(rotation bar, function rot_err -> translation bar) of one case from its kabsch_f64 result."""
    c_r, c_t = C_R if c_r is None else c_r, C_T if c_t is None else c_t
    bar_r = c_r * ref["cond"] + 4 * EPS32
    return bar_r, lambda rot_err: rot_err * ref["ncA"] + c_t * EPS32 * (ref["ncA"] + ref["ncB"])


def kabsch_ratios(T, ref):
    """How much of the two bars a result uses with C_R = C_T = 1: ((|dR| - 4 eps) / cond, (|dt| - |dR| |cA|) / (eps (|cA| + |cB|)))."""
    T = np.asarray(T, dtype=np.float64)
    er, et = np.linalg.norm(T[:3, :3] - ref["R"]), np.linalg.norm(T[:3, 3] - ref["t"])
    den_t = EPS32 * (ref["ncA"] + ref["ncB"])
    return (er - 4 * EPS32) / ref["cond"], ((et - er * ref["ncA"]) / den_t if den_t > 0 else (0.0 if et == 0 else np.inf))


def kabsch_check(T, ref, kind, c_r=None, c_t=None):
    """None if T meets what `kind` asks of it, else a string saying what it misses.  kind: "bar", "proper" or "identity"."""
    T = np.asarray(T, dtype=np.float64)
    if not np.isfinite(T).all():
        return "not finite"
    if not np.array_equal(T[3], [0, 0, 0, 1]):
        return "last row %s" % T[3]
    if kind == "identity":
        return None if np.array_equal(T, np.eye(4)) else "not the exact identity"
    R, t = T[:3, :3], T[:3, 3]
    bar_r, bar_t = kabsch_bar(ref, c_r, c_t)
    if kind == "bar":
        er, et = np.linalg.norm(R - ref["R"]), np.linalg.norm(t - ref["t"])
        if not er <= bar_r:
            return "|R - R64|_F = %.3e > %.3e" % (er, bar_r)
        if not et <= bar_t(er):
            return "|t - t64| = %.3e > %.3e" % (et, bar_t(er))
        return None
    assert kind == "proper", kind
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6:
        return "R R^T - I = %.3e" % np.abs(R @ R.T - np.eye(3)).max()
    if abs(np.linalg.det(R) - 1) > 1e-6:
        return "det R = %r" % np.linalg.det(R)
    miss = np.linalg.norm(R @ ref["cA"] + t - ref["cB"])
    if not miss <= bar_t(0.0):
        return "|R cA + t - cB| = %.3e > %.3e" % (miss, bar_t(0.0))
    return None


# ---- the case set -------------------------------------------------------------------------------------------------------------
def _moved(rng, A, noise=0.0, mirror=None, t_scale=1.0):
    """B = R (A mirrored) + t + noise from the fp32-rounded A, rounded to fp32."""
    A = A.astype(np.float32).astype(np.float64)
    X = A if mirror is None else A * np.asarray(mirror, dtype=np.float64)
    B = X @ random_rotation(rng).T + t_scale * rng.normal(size=3)
    if noise:
        B = B + noise * rng.normal(size=A.shape)
    return A.astype(np.float32), B.astype(np.float32)


def _iso(rng, K, noise=0.01):
    return _moved(rng, rng.normal(size=(K, 3)), noise)


def _build(family, param, rng):
    """(A, B, w, thr) of one case; fp32 arrays [K,3], w fp32 [K] or None."""
    w, thr = None, 0.0
    if family == "iso":
        A, B = _iso(rng, 500)
    elif family == "planar":  # exactly planar: z == 0 in A, so the third row of H is exactly zero
        A = rng.normal(size=(300, 3)) * [1, 1, 0]
        A, B = _moved(rng, A)
    elif family == "planar_noise":  # out-of-plane noise of relative size `param`
        A = rng.normal(size=(300, 3)) * [1, 1, param]
        A, B = _moved(rng, A)
    elif family == "collinear":  # sigma_2 / sigma_1 of the centred point matrix = param
        A = rng.normal(size=(300, 3)) * [1, param, param]
        A, B = _moved(rng, A @ random_rotation(rng).T)
    elif family in ("cube", "octahedron", "prism"):  # repeated singular values, under a known rotation
        if family == "octahedron":
            A = np.concatenate([np.eye(3), -np.eye(3)])
        else:
            A = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
            if family == "prism":  # sigma_1 = sigma_2 > sigma_3
                A = A * [1, 1, 0.5]
        A, B = _moved(rng, A)
    elif family == "mirror":  # delta = -1 with sigma_3 / sigma_1 of H = param
        r = np.sqrt(param)
        A, B = _moved(rng, rng.normal(size=(400, 3)) * [1, 1, r], noise=1e-3 * r, mirror=[1, 1, -1])
    elif family == "planar_mirror":  # exactly planar and mirrored IN the plane: sigma_3 = 0, the proper rotation is a half turn
        A, B = _moved(rng, rng.normal(size=(300, 3)) * [1, 1, 0], mirror=[1, -1, 1])
    elif family == "nearplanar_zmirror":  # delta = -1 with a small sigma_3
        A, B = _moved(rng, rng.normal(size=(300, 3)) * [1, 1, 1e-3], mirror=[1, 1, -1])
    elif family == "offset":  # cloud centre at |c| = param (metric-frame KITTI / OpenGF coordinates): t = cB - R cA cancels
        u = rng.normal(size=3)
        A = rng.normal(size=(500, 3)) + param * u / np.linalg.norm(u)
        A = A.astype(np.float32).astype(np.float64)
        R = axis_angle(rng.normal(size=3), 5.0)
        B = (A @ R.T + rng.normal(size=3) + 0.01 * rng.normal(size=A.shape)).astype(np.float32)
        A = A.astype(np.float32)
    elif family == "scale":  # coordinates scaled by 2^param (exact in fp32)
        A, B = _iso(rng, 500)
        A, B = (A * np.float32(2.0 ** param)).astype(np.float32), (B * np.float32(2.0 ** param)).astype(np.float32)
    elif family == "k":
        A, B = _iso(rng, int(param))
    elif family == "weights_span":  # weights over 1e-6 .. 1e3
        A, B = _iso(rng, 400)
        w = (10.0 ** rng.uniform(-6, 3, size=400)).astype(np.float32)
    elif family == "weights_keep":  # thresholds that leave exactly `param` points (and w == thr exactly is kept)
        A, B = _iso(rng, 64)
        w = rng.uniform(0.0, 0.4, size=64).astype(np.float32)
        keep = rng.permutation(64)[: int(param)]
        w[keep] = np.float32(0.5)
        w[keep[0]] = np.float32(0.75)
        thr = 0.5
    elif family == "weights_none":  # every weight below the threshold
        A, B = _iso(rng, 64)
        w, thr = rng.uniform(0.0, 0.4, size=64).astype(np.float32), 0.5
    else:
        raise KeyError(family)
    return A, B, w, thr


SEEDS = 3
# family, parameters, what the cases are held to.  "bar": the Kabsch bar against kabsch_f64; "proper": properness only (the
# reference does not determine the rotation either: cond > 1e-3); "identity": the exact identity (no correspondence survives).
_FAMILIES = [
    ("iso", [None], "bar"),
    ("planar", [None], "bar"),
    ("planar_noise", [1e-3, 1e-6, 1e-9, 1e-12], "bar"),
    ("collinear", [1e-2], "bar"),
    ("collinear", [1e-4], "proper"),
    ("cube", [None], "bar"),
    ("octahedron", [None], "bar"),
    ("prism", [None], "bar"),
    ("mirror", [0.3, 1e-2, 1e-4], "bar"),
    ("planar_mirror", [None], "bar"),
    ("nearplanar_zmirror", [None], "bar"),
    ("offset", [0, 10, 100, 1000], "bar"),
    ("scale", [-40, -20, -10, 10, 20], "bar"),
    ("k", [0], "identity"),
    ("k", [1, 2], "proper"),
    ("k", [3, 4, 255, 256, 257, 511, 513], "bar"),
    ("weights_span", [None], "bar"),
    ("weights_keep", [1, 2], "proper"),
    ("weights_keep", [3], "bar"),
    ("weights_none", [None], "identity"),
]
REFLECTED = ("mirror", "nearplanar_zmirror")  # families whose float64 delta is -1


def kabsch_case_table():
    """[(name, family, param, kind)]: every case of the dense solve, each a fixed seeded input."""
    rows = []
    for family, params, kind in _FAMILIES:
        for p in params:
            for seed in range(SEEDS):
                rows.append(("%s%s/%d" % (family, "" if p is None else "_%g" % p, seed), family, p, kind))
    rows.append(("k_65537/0", "k", 65537, "bar"))
    return rows


def kabsch_case(name):
    """(A, B, w, thr, kind) of the named case."""
    for nm, family, p, kind in kabsch_case_table():
        if nm == name:
            return _build(family, p, case_rng(name)) + (kind,)
    raise KeyError(name)


def small_problem_batch(bs=1000, K=37, seed=5):
    """bs small well-posed problems for ONE call (the per-block offsets): A, B [bs,K,3], w [bs,K], thr."""
    rng = np.random.default_rng(seed)
    A, B = np.empty((bs, K, 3), np.float32), np.empty((bs, K, 3), np.float32)
    for i in range(bs):
        A[i], B[i] = _iso(rng, K)
    return A, B, rng.uniform(0.2, 1.0, size=(bs, K)).astype(np.float32), 0.3


# ---- deliberately wrong solves (test_pose_ref_host.py: the bar must see each of them) ------------------------------------------
def kabsch_origin_f32(A, B):
    """H accumulated about the ORIGIN instead of the centroids, in fp32 (the centroid terms subtracted afterwards)."""
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    K = np.float32(len(A) + 1e-6)
    cA, cB = A.sum(axis=0, dtype=np.float32) / K, B.sum(axis=0, dtype=np.float32) / K
    H = np.zeros((3, 3), np.float32)
    for a, b in zip(A, B):
        H = (H + np.outer(a, b).astype(np.float32)).astype(np.float32)
    H = (H - np.float32(len(A)) * np.outer(cA, cB).astype(np.float32)).astype(np.float32)
    return _pose_from_h(H.astype(np.float64), cA.astype(np.float64), cB.astype(np.float64))


def _pose_from_h(H, cA, cB, sweeps=None):
    if sweeps is None:
        U, _, Vt = np.linalg.svd(H)
        V = Vt.T
    else:
        U, V = jacobi_svd3(H, sweeps)
    R = V @ np.diag([1.0, 1.0, np.sign(np.linalg.det(V) * np.linalg.det(U)) or 1.0]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cB - R @ cA
    return T


def jacobi_svd3(H, sweeps=16):
    """One-sided Jacobi as csrc/kabsch.hip runs it (scale-free stop rule), cut to `sweeps` passes.  Returns (U, V), sorted."""
    g, v = np.array(H, dtype=np.float64).T.copy(), np.eye(3)  # g[c] = column c of H V
    for _ in range(sweeps):
        off = 0.0
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al, be, ga = g[p] @ g[p], g[q] @ g[q], g[p] @ g[q]
            if ga != 0.0 and abs(ga) > 1e-16 * np.sqrt(al * be):
                off += abs(ga)
                zeta = (be - al) / (2 * ga)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.hypot(1.0, zeta))
                cs = 1 / np.sqrt(1 + t * t)
                sn = cs * t
                g[p], g[q] = cs * g[p] - sn * g[q], sn * g[p] + cs * g[q]
                v[p], v[q] = cs * v[p] - sn * v[q], sn * v[p] + cs * v[q]
        if off == 0.0:
            break
    s = np.linalg.norm(g, axis=1)
    order = np.argsort(-s, kind="stable")
    g, v, s = g[order], v[order], s[order]
    u = g / np.maximum(s, 1e-300)[:, None]
    if not s[2] > 1e-14 * s[0]:  # rank 2: complete the basis (the sign cancels against det(V U^T))
        u[2] = np.cross(u[0], u[1])
    return u.T, v.T


def kabsch_one_sweep(A, B):
    """The float64 solve with the Jacobi sweep cut to ONE pass."""
    r = kabsch_f64(A, B)
    return _pose_from_h(r["H"], r["cA"], r["cB"], sweeps=1)


# ------------------------------------------------------------------------------------------------------------- RE / TE
def re_te_f64(P, G):
    """utils.py:181-189 in float64 from fp32 poses [n,4,4]: (RE degrees, TE)."""
    P, G = np.asarray(P, np.float32).astype(np.float64).reshape(-1, 4, 4), np.asarray(G, np.float32).astype(np.float64).reshape(-1, 4, 4)
    x = ((P[:, :3, :3] * G[:, :3, :3]).sum(axis=(1, 2)) - 1.0) / 2.0
    return np.degrees(np.arccos(np.clip(x, -1.0, 1.0))), np.linalg.norm(P[:, :3, 3] - G[:, :3, 3], axis=1)


def re_interval(P, G):
    """[lo, hi] degrees that a correctly rounded fp32 evaluation must fall in.  x = (tr - 1) / 2 is formed from nine products, eight
    additions, a subtraction and a halving: dx = 4 * 2^-24 * (1 + sum |P_ij G_ij| / 2) bounds its rounding; acos is monotone, so the
    result lies between the acos of the two ends, widened by 4 * 2^-24 relative for acosf and the conversion to degrees."""
    P, G = np.asarray(P, np.float32).astype(np.float64).reshape(-1, 4, 4), np.asarray(G, np.float32).astype(np.float64).reshape(-1, 4, 4)
    pg = P[:, :3, :3] * G[:, :3, :3]
    x = (pg.sum(axis=(1, 2)) - 1.0) / 2.0
    dx = 4 * EPS32 * (1.0 + 0.5 * np.abs(pg).sum(axis=(1, 2)))
    re64 = np.degrees(np.arccos(np.clip(x, -1.0, 1.0)))
    lo = np.degrees(np.arccos(np.clip(x + dx, -1.0, 1.0)))
    hi = np.degrees(np.arccos(np.clip(x - dx, -1.0, 1.0)))
    return lo - 4 * EPS32 * re64, hi + 4 * EPS32 * re64


TE_RTOL, TE_ATOL = 4 * EPS32, 2.0 ** -149

RE_ANGLES = (0.0, 1e-3, 1e-2, 0.1, 1.0, 5.0, 15.0, 90.0, 179.0, 179.99, 180.0)


def pose_pairs(n, seed=0):
    """n pairs of fp32 poses (P, G): G a random pose, P = D G with D a rotation by RE_ANGLES[i % 11] about a random axis and a
    translation offset of 1e-6 .. 1e4, both rounded to fp32.  Returns (P, G, the angle of each pair)."""
    rng = np.random.default_rng(seed)
    P, G, ang = np.zeros((n, 4, 4)), np.zeros((n, 4, 4)), np.zeros(n)
    for i in range(n):
        ang[i] = RE_ANGLES[i % len(RE_ANGLES)]
        g = np.eye(4)
        g[:3, :3], g[:3, 3] = random_rotation(rng), rng.normal(size=3) * 10.0 ** rng.uniform(-6, 4)
        d = np.eye(4)
        u = rng.normal(size=3)
        d[:3, :3], d[:3, 3] = axis_angle(rng.normal(size=3), ang[i]), u / np.linalg.norm(u) * 10.0 ** rng.uniform(-6, 4)
        P[i], G[i] = d @ g, g
    return P.astype(np.float32), G.astype(np.float32), ang


# ---------------------------------------------------------------------------------------------------------- point loss
def point_loss_f64(pred, src, row0, lens, R, t):
    """Per pair, the float64 mean of the fp32 terms sum_xyz |pred - (R a + t)| (every fp32 operation rounded on its own, in the
    kernel's order); an empty pair gives 0."""
    pred, src = np.asarray(pred, np.float32), np.asarray(src, np.float32)
    out = np.zeros(len(lens))
    for p, (r0, n) in enumerate(zip(row0, lens)):
        if n == 0:
            continue
        a, q = src[r0:r0 + n], pred[r0:r0 + n]
        Rp, tp = np.asarray(R[p], np.float32).reshape(3, 3), np.asarray(t[p], np.float32).reshape(3)
        s = np.zeros(n, np.float32)
        for k in range(3):
            reg = ((Rp[k, 0] * a[:, 0] + Rp[k, 1] * a[:, 1]) + Rp[k, 2] * a[:, 2]) + tp[k]
            s = s + np.abs(q[:, k] - reg)
        assert s.dtype == np.float32
        out[p] = s.astype(np.float64).mean()
    return out


# ------------------------------------------------------------------------------------------- the fused gather + solve
def corr_problem(lens, kinds, seed=0, every=1, s=(0.37, 0.52, 0.81), c_norm=300.0):
    """A packed batch for scream_kabsch_corr in the normalised frame: src [rows,3], its partners twice -- `ref` in shuffled order
    with idx pointing at them, and `ref_rows` row-aligned with src (the idx == NULL mode) -- valid set on one row in `every`,
    per-pair s (not powers of two) and c at c_norm metres from the origin.  Clouds are padded to multiples of 128 rows.
    kinds: "iso"; "wallfloor" (a floor with a 3 mm strip of wall: near-planar); "mirror" (a reflected partner cloud, delta = -1)."""
    rng = np.random.default_rng(seed)
    row0, r0 = [], 0
    for n in lens:
        row0.append(r0)
        r0 += (n + 127) // 128 * 128
    src, ref, ref_rows = np.zeros((r0, 3), np.float32), np.zeros((r0, 3), np.float32), np.zeros((r0, 3), np.float32)
    idx, valid = np.zeros(r0, np.int32), np.zeros(r0, np.uint8)
    for p, (n, kind) in enumerate(zip(lens, kinds)):
        x = rng.normal(scale=0.3, size=(n, 3))
        mirror = None
        if kind == "wallfloor":
            wall = rng.uniform(size=n) < 0.1
            x[:, 2] = 0.0
            x[wall, 0], x[wall, 2] = 0.0, rng.uniform(0, 0.003, size=int(wall.sum()))
        elif kind == "mirror":
            mirror = [1, 1, -1]
        a, b = _moved(rng, x, noise=1e-3, mirror=mirror, t_scale=0.1)
        perm = rng.permutation(n)
        sl = slice(row0[p], row0[p] + n)
        src[sl], ref_rows[sl] = a, b
        ref[row0[p] + perm] = b
        idx[sl] = perm
        valid[row0[p]: row0[p] + n: every] = 1
    u = rng.normal(size=(len(lens), 3))
    c = (c_norm * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    return dict(src=src, ref=ref, ref_rows=ref_rows, idx=idx, valid=valid, row0=np.asarray(row0, np.int32),
                lens=np.asarray(lens, np.int32), s=np.asarray(s[: len(lens)], np.float32), c=c)


def corr_reference(pb, p, with_idx=True, valid=None):
    """kabsch_f64 of pair p of a corr_problem on the rows the reference gathers; also returns K."""
    v = pb["valid"] if valid is None else valid
    A, B = gather_corr(pb["src"], pb["ref"] if with_idx else pb["ref_rows"], int(pb["row0"][p]), int(pb["lens"][p]), int(pb["row0"][p]),
                       pb["idx"] if with_idx else None, v, pb["s"][p], pb["c"][p])
    return kabsch_f64(A, B), len(A)


# the corr problems of tests/test_gpu_pose_backend.py: (lens, kinds, one valid row in `every`); all well-posed (held to the bar)
CORR_PROBLEMS = {
    "dense": ((5000, 3000, 257), ("iso", "iso", "iso"), 1),
    "sparse": ((5000, 3000, 4000), ("iso", "iso", "iso"), 1000),
    "shapes": ((4000, 3000, 1000), ("wallfloor", "mirror", "iso"), 1),
}
