"""Restatement and yardstick of the raw-scan ICP (scream_icp_raw_range / scream_icp_raw_nn, csrc/icp_raw.hip) in plain numpy.
Nothing here imports scream_amd or touches a GPU; tests/test_rawicp_ref_host.py holds this file on the CPU before
tests/test_gpu_rawicp.py holds the kernels with it.

search           the brute-force float64 search: a = ((t0 x + t1 y) + t2 z) + t3, d2 = (dx^2 + dy^2) + dz^2 from direct
                 differences, the lowest target row on ties, a correspondence iff d2 < r2 strictly, r2 = the double product.
chunk_sums       the 17 sums in the kernel's order: per chunk of 256 consecutive source rows (a row without a correspondence
                 contributes 0.0) each wave of 64 rows by the butterfly v += v[lane ^ 1], ^ 2, ^ 4, ^ 8, ^ 16, ^ 32, the four waves
                 as (w0 + w1) + (w2 + w3); the chunk sums sequentially in ascending chunk order from 0.0.  (numpy's pairwise
                 ``sum`` is not that order.)
icp_raw_ref      the loop in the kernel's order, the Jacobi SVD of csrc/svd3.h restated operation by operation (pose_ref.jacobi_svd3
                 is the same algorithm with numpy's roundings): H = sum a b^T - cA (sum b)^T from the one-pass sums.
icp_raw_lapack   the same loop with two-pass means and covariance and np.linalg.svd: the independent float64 answer.

Margins.  A float64 `a` carries about 2^-50 |x| of freedom between correct implementations, so two candidates whose squared
distances differ by at least NEEDED64 = 2^-40 (|a|^2 + |b|^2)_max keep their order and a squared distance that far from r2 stays
on its side, with three decimal orders of headroom.  Every evaluation records its selection margin (nearest against second
nearest, over the rows with a correspondence), its radius margin (|d2 - r2| of the nearest, over all rows) and NEEDED64.  Under
the condition the GPU's correspondences are determined: fitness and iters are exact comparisons, T and RMSE differ by rounding.

Bars.  The form of pose_ref.kabsch_bar with EPS64 = 2^-53: the T that a loop returns solves, in exact arithmetic, the Kabsch
problem X -> B of its last update (X the matched source rows in their own frame, B their targets), so with the float64 figures of
that problem (pose_ref.kabsch_f64's S, sigma, delta, |cA|, |cB| without the + 1e-6)
    |R - R_lapack|_F <= C_R64 * 2^-53 * S / (sigma_2 + delta sigma_3) + 4 * 2^-53
    |t - t_lapack|   <= |R - R_lapack|_F * |cA| + C_T64 * 2^-53 * (|cA| + |cB|)
C_R64, C_T64 are four times the worst ratio of icp_raw_ref against icp_raw_lapack over the well-posed problems (one update and
whole loops), the convention of pose_ref.ORACLE_RATIO_R / C_R: a kernel further from LAPACK than four times what a faithful
restatement of itself is has a defect.  The one-pass covariance cancels against |c|^2 / spread^2, so the ratios are largest at
the far frames; they are measured on the CPU with
    python tests/test_rawicp_ref_host.py
and tests/test_rawicp_ref_host.py fails if they move by more than a factor of two.
inlier_rmse is held against one float64 spacing or RATIO = 2 times the restatements' distance, whichever is larger.
"""
import numpy as np

import icp_step_ref as ISR
import pose_ref as PR

EPS64 = 2.0 ** -53
RATIO = 2
VARIANTS = ("fp32_expanded", "le_radius", "ties_highest", "means_1e-6", "compose_right")

# measured by tests/test_rawicp_ref_host.py (python tests/test_rawicp_ref_host.py prints them): worst rotation ratio and worst
# translation ratio of icp_raw_ref against icp_raw_lapack over well_posed_problems(), one update and whole loops.
# Rotation: 3546 (lattice3841/30, whole loop: |R - R_lapack|_F = 6.1e-13; 1355 and 393 for the 257-row lattices at 30 and 300 m,
# 1.6 at the origin, 1.3 on the ring pair: the one-pass covariance sum a b^T - cA (sum b)^T loses |c|^2 / spread^2).
# Translation: 6.12 (ring/0, one update); negative at the far frames, where the rotation term of the bar dominates.
MEASURED_RATIO_R = 3546.0
MEASURED_RATIO_T = 6.12
C_R64 = 4.0 * MEASURED_RATIO_R
C_T64 = 4.0 * MEASURED_RATIO_T


# ------------------------------------------------------------------------------------------------------------ problems
def f64pose(T):
    return np.asarray(T, dtype=np.float64).reshape(4, 4).copy()


def lattice(frame, n, n_far=0, seed=0, slow=False):
    """(src, tgt, T0 float64, radius) of icp_step_ref's lattice / slow problem at a frame, the fp32 start pose widened."""
    mk = ISR.slow_problem if slow else ISR.lattice_problem
    src, tgt, T0, radius = mk(frame, ISR.frame_h(frame), n, *(() if slow else (n_far,)), seed)
    return src, tgt, f64pose(T0), float(radius)


def ring_scene(n, seed=0):
    """n fp32 points of a LiDAR-like scan spanning +-80 m: 64 beams between -24.8 and 2 degrees from a sensor 1.73 m above a
    ground plane, cut by walls 6 .. 80 m away (one distance per 5-degree sector)."""
    rng = np.random.default_rng([11, seed, n])
    elev = np.radians(rng.integers(0, 64, size=n) * (26.8 / 63.0) - 24.8)
    azim = rng.uniform(0.0, 2 * np.pi, size=n)
    wall = rng.uniform(6.0, 80.0, size=72)[(azim / (2 * np.pi) * 72).astype(int) % 72]
    with np.errstate(divide="ignore"):
        ground = np.where(elev < 0, 1.73 / np.maximum(np.sin(-elev), 1e-9), np.inf)
    rho = np.minimum(ground, wall / np.cos(elev))
    rho = rho * (1.0 + 0.002 * rng.normal(size=n))
    xyz = np.stack([rho * np.cos(elev) * np.cos(azim), rho * np.cos(elev) * np.sin(azim), rho * np.sin(elev)], axis=1)
    return xyz.astype(np.float32)


def ring_pair(n=4096, seed=1, frame=0.0, off_t=0.15, off_deg=0.3):
    """(src, tgt, T0, T_true, radius 0.2): tgt a ring scene (shifted to `frame` on every axis), src its rows in shuffled order with
    2 cm of noise, seen from a pose T_true^-1 of the size KITTI odometry leaves between the frames of a pair; T0 = T_true moved by
    off_t metres and off_deg degrees about the sensor."""
    rng = np.random.default_rng([13, seed, n, int(frame)])
    tgt = (ring_scene(n, seed).astype(np.float64) + frame).astype(np.float32)
    centre = np.full(3, float(frame))
    Tt = np.eye(4)
    Tt[:3, :3] = PR.axis_angle([0.1, 0.05, 1.0], 4.0)
    Tt[:3, 3] = centre - Tt[:3, :3] @ centre + np.array([1.3, 0.2, 0.02])
    pts = tgt[rng.permutation(n)].astype(np.float64) + 0.02 * rng.normal(size=(n, 3))
    src = ((pts - Tt[:3, 3]) @ Tt[:3, :3]).astype(np.float32)  # R^T (p - t)
    D = np.eye(4)
    D[:3, :3] = PR.axis_angle(rng.normal(size=3), off_deg)
    d = rng.normal(size=3)
    D[:3, 3] = centre - D[:3, :3] @ centre + off_t * d / np.linalg.norm(d)
    return src, tgt, D @ Tt, Tt, 0.2


def radius_lattice(shift):
    """(src, tgt, T = I, R = 0.5): targets on the even integers of [-4, 4]^3 plus one anchor row at -10 - shift per axis, which
    moves the grid origin by `shift` (sub-cell for shift < R); sources exactly 0.5 from a target along +-x, +-y, +-z (d2 == 0.25
    exactly: a correspondence at the radius nextafter(0.5, 1), none at 0.5 and below) and 0.25 from one (always a correspondence)."""
    g = np.arange(-4, 5, 2).astype(np.float64)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    block = block[rng.permutation(len(block))]
    tgt = np.concatenate([block[:60], np.full((1, 3), -10.0 - shift), block[60:]])
    offs = np.concatenate([0.5 * np.eye(3), -0.5 * np.eye(3), 0.25 * np.eye(3)])
    src = (block[:, None, :] + offs[None, :, :]).reshape(-1, 3)
    return src.astype(np.float32), tgt.astype(np.float32), np.eye(4), 0.5


SHIFTS = (0.0, 0.125, 0.25, 0.375)


def tie_pair(n=1024, seed=3):
    """A ring pair whose target holds every row twice, in shuffled order: every correspondence is a tie between two rows."""
    src, tgt, T0, Tt, radius = ring_pair(n, seed)
    rng = np.random.default_rng(seed)
    tgt2 = np.concatenate([tgt, tgt])[rng.permutation(2 * n)]
    return src, tgt2.copy(), Tt, radius


def well_posed_problems():
    """[(name, (src, tgt, T0, radius))]: the problems whose T is held to the bars."""
    out = [("lattice/%d" % f, lattice(f, 257, 3)) for f in ISR.FRAMES]
    out.append(("slow/0", lattice(0, 100, slow=True)))
    out.append(("lattice3841/30", lattice(30, 3841, 3)))
    s, t, T0, _, r = ring_pair()
    out.append(("ring/0", (s, t, T0, r)))
    return out


def loop_problems():
    """The whole-loop problems of the GPU test: the lattices at frames 0, 30, 300, the slow start, the ring pair."""
    wp = dict(well_posed_problems())
    return [(k, wp[k]) for k in ("lattice/0", "lattice/30", "lattice/300", "slow/0", "ring/0")]


# -------------------------------------------------------------------------------------------------------------- search
def transform(T, src):
    """a_k = ((t_k0 x + t_k1 y) + t_k2 z) + t_k3 in float64 from the fp32 rows."""
    x = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64)
    return np.stack([((T[k, 0] * x[:, 0] + T[k, 1] * x[:, 1]) + T[k, 2] * x[:, 2]) + T[k, 3] for k in range(3)], axis=1)


def search(a, tgt, radius, ties="lowest", strict=True, block=512):
    """Brute force over every target row.  Returns dict(idx int32 (-1: none), d2 (+inf: none), near (row of the nearest whatever the
    radius, -1 for an empty target), lo (its d2), second (the second nearest d2), mask)."""
    a = np.asarray(a, np.float64).reshape(-1, 3)
    t = np.asarray(tgt, np.float32).astype(np.float64).reshape(-1, 3)
    n, m = len(a), len(t)
    r2 = float(radius) * float(radius)
    near, lo, second = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    if m:
        for i0 in range(0, n, block):
            q = a[i0:i0 + block]
            dx, dy, dz = q[:, 0:1] - t[None, :, 0], q[:, 1:2] - t[None, :, 1], q[:, 2:3] - t[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            rows = np.arange(len(q))
            j = d.argmin(axis=1) if ties == "lowest" else m - 1 - d[:, ::-1].argmin(axis=1)
            near[i0:i0 + block], lo[i0:i0 + block] = j, d[rows, j]
            if m > 1:
                d[rows, j] = np.inf
                second[i0:i0 + block] = d.min(axis=1)
    mask = (lo < r2) if strict else (lo <= r2)
    return dict(idx=np.where(mask, near, -1).astype(np.int32), d2=np.where(mask, lo, np.inf), near=near, lo=lo, second=second, mask=mask)


def search_fp32_expanded(a, tgt, radius):
    """The deliberately wrong search: icp_grid.h's fp32 selection (-2 a.b + |a|^2) + |b|^2 on fp32 a, against the fp32 r2."""
    a32 = np.asarray(a, np.float64).astype(np.float32)
    t32 = np.asarray(tgt, np.float32)
    n, m = len(a32), len(t32)
    near, lo = np.zeros(n, np.int64), np.full(n, np.inf)
    for i0 in range(0, n, 64):
        q = a32[i0:i0 + 64]
        d = np.stack([ISR._expanded_d_f32(np.repeat(q[i:i + 1], m, axis=0), t32) for i in range(len(q))])
        j = d.argmin(axis=1)
        near[i0:i0 + 64], lo[i0:i0 + 64] = j, d[np.arange(len(q)), j]
    mask = lo < np.float32(radius) * np.float32(radius)
    return dict(idx=np.where(mask, near, -1).astype(np.int32), near=near, lo=lo.astype(np.float64), mask=mask)


# ---------------------------------------------------------------------------------------------------------------- sums
def chunk_sums(a, b, mask, d2):
    """(total [17], per-chunk [nchunks,17]) in the kernel's order.  a [n,3] float64, b [n,3] the matched target rows widened
    (any value where mask is False), d2 [n]."""
    n = len(a)
    nchunks = max(1, (n + 255) // 256)
    v = np.zeros((nchunks * 256, 17))
    if n:
        m = np.asarray(mask, bool)
        aa, bb = np.where(m[:, None], a, 0.0), np.where(m[:, None], b, 0.0)
        v[:n, 0] = m
        v[:n, 1] = np.where(m, d2, 0.0)
        v[:n, 2:5], v[:n, 5:8] = aa, bb
        v[:n, 8:17] = (aa[:, :, None] * bb[:, None, :]).reshape(n, 9)
    v = v.reshape(nchunks, 4, 64, 17)
    lane = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[:, :, lane ^ s, :]
    w = v[:, :, 0, :]
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    tot = np.zeros(17)
    for c in range(nchunks):
        tot = tot + part[c]
    return tot, part


# --------------------------------------------------------------------------------------------------------------- loops
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def _svd_kernel(H):
    """(U, V) of csrc/svd3.h, operation by operation on Python floats (IEEE float64, no contraction): pose_ref.jacobi_svd3 is the
    same algorithm through numpy's dot and hypot, whose roundings differ, and the loop below is held to the LAST bit of the RMSE."""
    sqrt = np.sqrt
    g = [[float(H[i][c]) for i in range(3)] for c in range(3)]
    v = [[1.0 if i == c else 0.0 for i in range(3)] for c in range(3)]
    for _ in range(16):
        off = 0.0
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = _dot3(g[p], g[p]), _dot3(g[q], g[q]), _dot3(g[p], g[q])
            lim = 1e-16 * float(sqrt(alpha * beta))
            if gamma != 0.0 and abs(gamma) > lim:
                off += abs(gamma)
                zeta = (beta - alpha) / (2.0 * gamma)
                t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + float(sqrt(1.0 + zeta * zeta)))
                cs = 1.0 / float(sqrt(1.0 + t * t))
                sn = cs * t
                for i in range(3):
                    gp, gq, vp, vq = g[p][i], g[q][i], v[p][i], v[q][i]
                    g[p][i], g[q][i] = cs * gp - sn * gq, sn * gp + cs * gq
                    v[p][i], v[q][i] = cs * vp - sn * vq, sn * vp + cs * vq
        if off == 0.0:
            break
    s = [float(sqrt(_dot3(g[c], g[c]))) for c in range(3)]
    for a in (0, 1, 0):
        b = a + 1
        if s[a] < s[b]:
            s[a], s[b], g[a], g[b], v[a], v[b] = s[b], s[a], g[b], g[a], v[b], v[a]
    u = [[0.0] * 3 for _ in range(3)]
    if not s[0] > 0.0:
        return np.eye(3), np.eye(3)
    u[0] = [g[0][i] / s[0] for i in range(3)]
    if s[1] > 1e-14 * s[0]:
        u[1] = [g[1][i] / s[1] for i in range(3)]
    else:
        a0 = [abs(x) for x in u[0]]
        k = 0 if (a0[0] <= a0[1] and a0[0] <= a0[2]) else (1 if a0[1] <= a0[2] else 2)
        e = [1.0 if i == k else 0.0 for i in range(3)]
        pr = _dot3(e, u[0])
        w = [e[i] - pr * u[0][i] for i in range(3)]
        nw = float(sqrt(_dot3(w, w)))
        u[1] = [w[i] / nw for i in range(3)]
    if s[2] > 1e-14 * s[0]:
        u[2] = [g[2][i] / s[2] for i in range(3)]
    else:
        u[2] = [u[0][1] * u[1][2] - u[0][2] * u[1][1], u[0][2] * u[1][0] - u[0][0] * u[1][2], u[0][0] * u[1][1] - u[0][1] * u[1][0]]
    return np.array(u).T, np.array(v).T


def update_ref(tot, means_eps=0.0):
    """dT from the 17 sums, in the kernel's order."""
    cnt = tot[0]
    cA, cB = tot[2:5] / (cnt + means_eps), tot[5:8] / (cnt + means_eps)
    H = tot[8:17].reshape(3, 3) - cA[:, None] * tot[5:8][None, :]
    U, V = _svd_kernel(H)
    delta = -1.0 if _det3(V) * _det3(U) < 0.0 else 1.0
    dT = np.eye(4)
    for i in range(3):
        for j in range(3):
            dT[i, j] = (V[i, 0] * U[j, 0] + V[i, 1] * U[j, 1]) + delta * V[i, 2] * U[j, 2]
        dT[i, 3] = cB[i] - ((dT[i, 0] * cA[0] + dT[i, 1] * cA[1]) + dT[i, 2] * cA[2])
    return dT


def compose(dT, T):
    """dT . T with every entry ((d_i0 T_0j + d_i1 T_1j) + d_i2 T_2j) + d_i3 T_3j."""
    out = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = ((dT[i, 0] * T[0, j] + dT[i, 1] * T[1, j]) + dT[i, 2] * T[2, j]) + dT[i, 3] * T[3, j]
    return out


def update_lapack(A, B):
    """open3d's TransformationEstimationPointToPoint: two-pass means and covariance, LAPACK SVD."""
    cA, cB = A.mean(axis=0), B.mean(axis=0)
    U, _, Vt = np.linalg.svd((A - cA).T @ (B - cB))
    R = Vt.T @ np.diag([1.0, 1.0, -1.0 if np.linalg.det(Vt.T @ U.T) < 0 else 1.0]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cB - R @ cA
    return T


def _loop(src, tgt, T0, radius, max_iter, rel_fitness, rel_rmse, kernel_order, variant=None):
    assert variant is None or variant in VARIANTS, variant
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt64 = np.asarray(tgt, np.float32).astype(np.float64).reshape(-1, 3)
    T, n, r2 = f64pose(T0), len(src), float(radius) * float(radius)

    def evaluate(T):
        a = transform(T, src)
        if variant == "fp32_expanded":
            s = search_fp32_expanded(a, tgt, radius)
            exact = search(a, tgt, radius)
            s["second"], s["d2"] = exact["second"], None
            dd = a - tgt64[np.maximum(s["near"], 0)] if len(tgt64) else a
            s["lo"] = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        else:
            s = search(a, tgt, radius, ties="highest" if variant == "ties_highest" else "lowest", strict=variant != "le_radius")
        mask, near, lo = s["mask"], s["near"], s["lo"]
        b = tgt64[np.maximum(near, 0)] if len(tgt64) else np.zeros_like(a)
        cnt = int(mask.sum())
        if kernel_order:
            tot, _ = chunk_sums(a, b, mask, lo)
            rmse = float(np.sqrt(tot[1] / tot[0])) if cnt else 0.0
        else:
            tot = None
            rmse = float(np.sqrt(lo[mask].sum() / cnt)) if cnt else 0.0
        big = (float((a * a).sum(axis=1).max()) if n else 0.0) + (float((tgt64 * tgt64).sum(axis=1).max()) if len(tgt64) else 0.0)
        return dict(T=T.copy(), idx=np.where(mask, near, -1), mask=mask, cnt=cnt, fitness=(cnt / n if n else 0.0), rmse=rmse, tot=tot,
                    a=a, b=b, sel_margin=(float((s["second"] - lo)[mask].min()) if cnt else np.inf),
                    rad_margin=(float(np.abs(lo - r2).min()) if n and len(tgt64) else np.inf), needed=2.0 ** -40 * big)

    ev = evaluate(T)
    trace, it = [ev], 0
    while it < max_iter:
        if ev["cnt"]:
            if kernel_order:
                dT = update_ref(ev["tot"], 1e-6 if variant == "means_1e-6" else 0.0)
                T = compose(T, dT) if variant == "compose_right" else compose(dT, T)
            else:
                T = update_lapack(ev["a"][ev["mask"]], ev["b"][ev["mask"]]) @ T
        it += 1
        ev2 = evaluate(T)
        trace.append(ev2)
        conv = abs(ev["fitness"] - ev2["fitness"]) < rel_fitness and abs(ev["rmse"] - ev2["rmse"]) < rel_rmse
        ev = ev2
        if conv:
            break
    return dict(T=ev["T"], fitness=ev["fitness"], rmse=ev["rmse"], iters=it, trace=trace)


def icp_raw_ref(src, tgt, T0, radius, max_iter, rel_fitness=1e-6, rel_rmse=1e-6, variant=None):
    """The loop in the kernel's order.  Returns dict(T, fitness, rmse, iters, trace); trace[k] is the evaluation after k updates."""
    return _loop(src, tgt, T0, radius, max_iter, rel_fitness, rel_rmse, True, variant)


def icp_raw_lapack(src, tgt, T0, radius, max_iter, rel_fitness=1e-6, rel_rmse=1e-6):
    """The independent float64 answer: two-pass means and covariance, np.linalg.svd, numpy's own sums and products."""
    return _loop(src, tgt, T0, radius, max_iter, rel_fitness, rel_rmse, False)


# ---------------------------------------------------------------------------------------------------------------- bars
def last_update_stats(run, src):
    """The float64 figures of the Kabsch problem X -> B that the run's T solves: the correspondences of the evaluation BEFORE the
    last update (of evaluation 0 for a run without updates), X in the source's own frame."""
    ev = run["trace"][-2] if len(run["trace"]) > 1 else run["trace"][0]
    X = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3)[ev["mask"]]
    B = ev["b"][ev["mask"]]
    cA, cB = X.mean(axis=0), B.mean(axis=0)
    Xm, Bm = X - cA, B - cB
    U, sig, Vt = np.linalg.svd(Xm.T @ Bm)
    delta = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    S = float((np.linalg.norm(Xm, axis=1) * np.linalg.norm(Bm, axis=1)).sum())
    return dict(cond=EPS64 * S / (sig[1] + delta * sig[2]), ncA=float(np.linalg.norm(cA)), ncB=float(np.linalg.norm(cB)))


def pose_ratios(T, T_lapack, st):
    """How much of the two bars T uses with C_R64 = C_T64 = 1."""
    T, L = np.asarray(T, np.float64), np.asarray(T_lapack, np.float64)
    er, et = np.linalg.norm(T[:3, :3] - L[:3, :3]), np.linalg.norm(T[:3, 3] - L[:3, 3])
    return (er - 4 * EPS64) / st["cond"], (et - er * st["ncA"]) / (EPS64 * (st["ncA"] + st["ncB"]))


def pose_check(T, T_lapack, st, c_r=None, c_t=None):
    """None if T is within the bars of T_lapack, else what it misses."""
    c_r, c_t = C_R64 if c_r is None else c_r, C_T64 if c_t is None else c_t
    T, L = np.asarray(T, np.float64), np.asarray(T_lapack, np.float64)
    if not np.isfinite(T).all():
        return "not finite"
    if not np.array_equal(T[3], [0, 0, 0, 1]):
        return "last row %s" % T[3]
    er, et = np.linalg.norm(T[:3, :3] - L[:3, :3]), np.linalg.norm(T[:3, 3] - L[:3, 3])
    bar_r = c_r * st["cond"] + 4 * EPS64
    bar_t = er * st["ncA"] + c_t * EPS64 * (st["ncA"] + st["ncB"])
    if not er <= bar_r:
        return "|R - R_lapack|_F = %.3e > %.3e" % (er, bar_r)
    if not et <= bar_t:
        return "|t - t_lapack| = %.3e > %.3e" % (et, bar_t)
    return None


def rmse_ok(got, ref, lapack):
    """|got - lapack| <= max(RATIO |ref - lapack|, one float64 spacing of lapack)."""
    return bool(abs(float(got) - lapack) <= max(RATIO * abs(ref - lapack), np.spacing(abs(lapack))))


def margins_hold(*runs):
    return all(ev["sel_margin"] >= ev["needed"] and ev["rad_margin"] >= ev["needed"] for run in runs for ev in run["trace"])


def same_trajectory(x, y):
    tx, ty = x["trace"], y["trace"]
    return x["iters"] == y["iters"] and len(tx) == len(ty) and all(
        np.array_equal(u["idx"], v["idx"]) and u["fitness"] == v["fitness"] for u, v in zip(tx, ty))
