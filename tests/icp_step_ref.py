"""Reference and yardstick of the ICP loop (scream_icp_p2p: icp_pose_step + icp_store_partial of csrc/icp_p2p.hip), in plain numpy.
Nothing here imports scream_amd or touches a GPU; tests/test_icp_step_ref_host.py holds this file on the CPU before
tests/test_gpu_icp_step.py holds the kernels with it.

icp_f64          open3d's RegistrationICP loop (as oracle/icp_ref.py restates it) in float64 from the fp32 clouds and the fp32 start
                 pose, with a brute-force nearest neighbour: direct differences, lowest index on ties, a correspondence iff
                 d^2 < radius^2 with radius^2 the fp32 product the kernel compares with.
icp_f32_storage  the same loop with the roundings that include/scream_hip.h and the kernel document, and no others: what storing
                 the loop's state in fp32 costs a correct implementation.  Its distance from icp_f64 is the yardstick.
rule_ok          the one comparison rule: |got - f64| <= max(RATIO * |yardstick - f64|, one fp32 spacing of the float64 value).

inlier_rmse is, in both functions, sqrt(mean |a - b|^2) with the DIFFERENCE a - b taken in float64 (open3d measures the
difference); the search's own fp32 value (-2 a.b + |a|^2) + |b|^2 serves selection only (variant "expanded_residual" shows why).

An evaluation that finds no correspondence gives the identity update and the loop goes on, as open3d's loop does
(oracle/icp_ref.py breaks instead).  `iters` follows that: a pair that never finds a correspondence stops at its second
evaluation (iters = 1) when both thresholds are positive, since |0 - 0| < threshold, and runs to max_iter when a threshold is 0.

The margin condition.  The kernel selects with the fp32 sequence above; each of its roundings is at most half an ulp of a quantity
below 2 (|a|^2 + |b|^2), so two candidates whose true squared distances differ by at least NEEDED = 2^-20 (|a|^2 + |b|^2)_max keep
their order, and a squared distance at least that far from radius^2 stays on its side.  Every evaluation records its selection
margin (nearest against second nearest, over the rows that have a correspondence), its radius margin (|d^2 - radius^2| of the
nearest, over all rows) and NEEDED; `margins_hold` asserts the condition over whole trajectories.  Under it the GPU's search
provably picks these correspondences: fitness is an exact comparison, T and RMSE differ by rounding only.
"""
import numpy as np

import pose_ref as PR

RATIO = 2  # the project's ratio (tests/train_ref.py)
SIDE = 12  # the target lattice is SIDE^3 = 1728 points
FRAMES = (0, 30, 300)
LENGTHS = (1, 255, 256, 257, 3840, 3841, 7681)  # one chunk; the 15-group boundary (15 x 256) and the first wrap; three chunks in group 0
COINCIDENT_FRAMES = (0, 3, 30, 300)
VARIANTS = ("expanded_residual", "drop_last_chunk", "compose_right", "divide_by_n")


def frame_h(frame):
    """Lattice spacing used at a frame: the smallest checked spacing whose margins clear NEEDED with headroom."""
    return 4.0 if frame >= 100 else 0.25


def n_far_for(n):
    return 3 if n >= 255 else 0


# ------------------------------------------------------------------------------------------------------------ problems
def lattice_problem(frame, h, n, n_far=0, seed=0):
    """(src fp32 [n,3], tgt fp32 [1728,3], T0 fp32 [4,4], radius).  Target: a shuffled 12^3 lattice of spacing h centred on
    (frame, frame, frame).  Source rows: lattice nodes drawn with repetition plus a uniform offset inside a ball of 0.05 h; the
    first n_far rows are displaced by 40 h along x and have no partner.  T0: a rotation about the lattice centre that moves no
    lattice point by more than 0.1 h, plus a shift of 0.05 h.  Radius 0.5 h; s = 1, c = 0."""
    rng = np.random.default_rng([seed, int(frame), n, n_far])
    g = (np.arange(SIDE) - (SIDE - 1) / 2.0) * h + frame
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    tgt = tgt[rng.permutation(len(tgt))].astype(np.float32)
    u = rng.normal(size=(n, 3))
    off = u / np.linalg.norm(u, axis=1, keepdims=True) * (0.05 * h * rng.uniform(size=(n, 1)) ** (1.0 / 3.0))
    src = tgt[rng.integers(0, len(tgt), size=n)].astype(np.float64) + off
    src[:n_far, 0] += 40.0 * h
    centre = np.full(3, float(frame))
    reach = (SIDE - 1) / 2.0 * np.sqrt(3.0) * h + 0.05 * h  # farthest a lattice row lies from the centre
    R = PR.axis_angle(rng.normal(size=3), np.degrees(0.1 * h / reach))
    d = rng.normal(size=3)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R, centre - R @ centre + 0.05 * h * d / np.linalg.norm(d)
    return src.astype(np.float32), tgt, T0.astype(np.float32), 0.5 * h


def coincident_problem(frame, h=None):
    """The target's own rows as the source, T0 = I: every true distance is 0, while the search's expanded fp32 value is a rounding
    residue of either sign once the frame is away from the origin.  The target is the lattice with every node moved inside a ball
    of 0.05 h: on the bare lattice (coordinates with a few bits) the expanded form is exact and shows nothing.
    (pose_ref.coincident_far_cloud is the same idea for the 1-NN search, but pairs every point with a one-ulp neighbour, which no
    margin condition survives.)"""
    h = frame_h(frame) if h is None else h
    _, tgt, _, radius = lattice_problem(frame, h, 1, 0, seed=1)
    rng = np.random.default_rng([7, int(frame)])
    u = rng.normal(size=tgt.shape)
    off = u / np.linalg.norm(u, axis=1, keepdims=True) * (0.05 * h * rng.uniform(size=(len(tgt), 1)) ** (1.0 / 3.0))
    tgt = (tgt.astype(np.float64) + off).astype(np.float32)
    return tgt.copy(), tgt, np.eye(4, dtype=np.float32), radius


def far_only_problem(frame, h, n, seed=0):
    """A source whose rows are all far: nothing is ever found."""
    return lattice_problem(frame, h, n, n, seed)


def slow_problem(frame, h, n, seed=0):
    """lattice_problem with the start shifted by 0.45 h along the diagonal, so that part of the rows lies beyond the radius at
    first and gains its partner after the first update: the fitness moves and the default stop rule needs more updates."""
    src, tgt, T0, radius = lattice_problem(frame, h, n, 0, seed)
    T0 = T0.copy()
    T0[:3, 3] += np.float32(0.45 * h / np.sqrt(3.0))
    return src, tgt, T0, radius


def few_corr_problem(frame, h, n, k, seed=0):
    """A source of n rows of which exactly k (the last k) have a partner."""
    return lattice_problem(frame, h, n, n - k, seed)


def stop_rule_problems():
    """[(name, problem)] run under the default thresholds 1e-6: one ordinary problem per frame (two updates) and the slow start at
    the origin (three).  test_icp_step_ref_host.py asserts that every |d fitness| and |d rmse| of icp_f64 on them stays a factor
    10 away from the thresholds, so the update count is not a matter of rounding."""
    out = [("ordinary/%d" % f, lattice_problem(f, frame_h(f), 257, 3)) for f in FRAMES]
    return out + [("slow/0", slow_problem(0, 0.25, 100, 0))]


BATCH_H = 4.0  # one call has one radius: the pairs that share a batch share the spacing that the frame at 300 needs


def degenerate_problems():
    """[(name, problem, correspondences)]: nothing found (an empty source, a source whose rows are all far) and undetermined
    poses (a source of one point, sources with exactly one and exactly two correspondences)."""
    far = far_only_problem(30, BATCH_H, 40)
    return [("empty", (np.zeros((0, 3), np.float32),) + far[1:], 0), ("all_far", far, 0),
            ("one_point", lattice_problem(30, BATCH_H, 1, 0, seed=2), 1), ("one_corr", few_corr_problem(30, BATCH_H, 40, 1), 1),
            ("two_corr", few_corr_problem(0, BATCH_H, 300, 2), 2)]


def degenerate_neighbours():
    """The two ordinary pairs a degenerate pair sits between."""
    return lattice_problem(300, BATCH_H, 257, 3, seed=3), lattice_problem(30, BATCH_H, 300, 3, seed=3)


def batch_problems():
    """Five pairs of different lengths and frames that stop after 2, 3, 1, 1 and 2 updates under the default thresholds."""
    return [("ordinary/300", lattice_problem(300, BATCH_H, 3841, 3)), ("slow/0", slow_problem(0, BATCH_H, 100, 0)),
            ("all_far/30", far_only_problem(30, BATCH_H, 40)), ("coincident/3", coincident_problem(3, BATCH_H)),
            ("ordinary/30", lattice_problem(30, BATCH_H, 257, 3))]


BATCH_ITERS = (2, 3, 1, 1, 2)


def extra_problems():
    """[(name, problem, max_iter, threshold)] of every GPU problem outside the grid and the coincident clouds."""
    out = [("stop/" + nm, pb, 30, 1e-6) for nm, pb in stop_rule_problems()] + [("batch/" + nm, pb, 30, 1e-6) for nm, pb in batch_problems()]
    out += [("neighbour/%d" % i, pb, 5, 1e-6) for i, pb in enumerate(degenerate_neighbours())]
    return out + [("degenerate/" + nm, pb, 1, 0.0) for nm, pb, _ in degenerate_problems()]


def stop_rule_is_decided(run, rel=1e-6):
    """Every |d fitness| and |d rmse| between consecutive evaluations is at least 10 rel or at most rel / 10."""
    tr = run["trace"]
    return all(abs(float(x[k]) - float(y[k])) >= 10 * rel or abs(float(x[k]) - float(y[k])) <= rel / 10
               for x, y in zip(tr, tr[1:]) for k in ("fitness", "rmse"))


# -------------------------------------------------------------------------------------------------------------- search
def _search(q, tgt, r2, block=256):
    """Brute-force 1-NN in float64 by direct differences.  Returns (idx, nearest d^2, second-nearest d^2, mask d^2 < r2)."""
    n = len(q)
    idx, lo, second = np.zeros(n, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    tx, ty, tz = (np.ascontiguousarray(tgt[:, k])[None, :] for k in range(3))
    for i0 in range(0, n, block):
        qb = q[i0:i0 + block]
        d = np.square(qb[:, 0:1] - tx)  # (dx^2 + dy^2) + dz^2, one axis at a time to keep the temporaries two-dimensional
        d += np.square(qb[:, 1:2] - ty)
        d += np.square(qb[:, 2:3] - tz)
        rows = np.arange(len(d))
        j = d.argmin(axis=1)  # lowest index on ties
        idx[i0:i0 + block], lo[i0:i0 + block] = j, d[rows, j]
        if tgt.shape[0] > 1:
            d[rows, j] = np.inf
            second[i0:i0 + block] = d.min(axis=1)
    return idx, lo, second, lo < r2


def _evaluation(T, q, tgt, r2, n):
    """The record of one evaluation: T, idx, mask, cnt, fitness, rmse (float64, direct difference), the margins and NEEDED."""
    if n:
        idx, lo, second, mask = _search(q, tgt, r2)
    else:
        idx, lo, second, mask = np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0, bool)
    cnt = int(mask.sum())
    big = (float((q * q).sum(axis=1).max()) if n else 0.0) + float((tgt * tgt).sum(axis=1).max())
    return dict(T=T.copy(), idx=idx, mask=mask, cnt=cnt, fitness=(cnt / n if n else 0.0),
                rmse=(float(np.sqrt(lo[mask].sum() / cnt)) if cnt else 0.0), d2=lo,
                sel_margin=(float((second - lo)[mask].min()) if cnt else np.inf),
                rad_margin=(float(np.abs(lo - r2).min()) if n else np.inf), needed=2.0 ** -20 * big)


def _radius2(radius):
    return float(np.float32(radius) * np.float32(radius))  # the fp32 product the kernel compares d with


def _result(trace, iters, keep_trace):
    last = trace[-1]
    return dict(T=last["T"], fitness=last["fitness"], rmse=last["rmse"], iters=iters, trace=trace if keep_trace else [last])


# ------------------------------------------------------------------------------------------------------- the float64 loop
def _rigid_update_f64(A, B):
    """open3d's TransformationEstimationPointToPoint without scaling: exact means, centred covariance, R = V diag(1, 1, det) U^T.
    (pose_ref.kabsch_f64 rounds its inputs to fp32 and carries the + 1e-6 of utils.py, so it serves the one-update test, whose
    inputs ARE fp32, not this loop, whose transformed points are float64.)"""
    cA, cB = A.mean(axis=0), B.mean(axis=0)
    U, _, Vt = np.linalg.svd((A - cA).T @ (B - cB))
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cB - R @ cA
    return T


def icp_f64(src, tgt, T0, radius, max_iter, rel_fitness=1e-6, rel_rmse=1e-6, trace=True):
    """src, tgt: the fp32 metric clouds (s = 1, c = 0), T0 the fp32 start pose.  Returns dict(T, fitness, rmse, iters, trace);
    trace[k] is the evaluation after k updates."""
    src, tgt = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(tgt, np.float32).astype(np.float64)
    T, r2, n = np.asarray(T0, np.float32).astype(np.float64), _radius2(radius), len(src)

    def evaluate(T):
        q = src @ T[:3, :3].T + T[:3, 3]
        return _evaluation(T, q, tgt, r2, n), q

    ev, q = evaluate(T)
    out, it = [ev], 0
    while it < max_iter:
        if ev["cnt"]:
            T = _rigid_update_f64(q[ev["mask"]], tgt[ev["idx"][ev["mask"]]]) @ T
        it += 1
        ev2, q = evaluate(T)
        out.append(ev2)
        conv = abs(ev["fitness"] - ev2["fitness"]) < rel_fitness and abs(ev["rmse"] - ev2["rmse"]) < rel_rmse
        ev = ev2
        if conv:
            break
    return _result(out, it, trace)


# ------------------------------------------------------------------------------------------------- the fp32-storage loop
def _expanded_d_f32(a, b):
    """The search's own fp32 value (csrc/icp_grid.h, take): dot by fma, then fma(-2, dot, |a|^2) + |b|^2, norms as (x^2 + y^2) + z^2."""
    a, b = a.astype(np.float32), b.astype(np.float32)
    sa = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    sb = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dot = (a[:, 0] * b[:, 0]).astype(np.float64)
    dot = (a64[:, 1] * b64[:, 1] + dot).astype(np.float32).astype(np.float64)  # a product of two fp32 is exact in float64
    dot = (a64[:, 2] * b64[:, 2] + dot).astype(np.float32).astype(np.float64)
    return (-2.0 * dot + sa.astype(np.float64)).astype(np.float32) + sb


def _rank_one_basis(H):
    """(U, V) of a rank-one H (ONE correspondence: H = (a - cA)(b - cB)^T) as csrc/kabsch.hip completes them.  The rotation about
    the one singular direction is then not determined, and where the matched point lands after the fp32 rounding of R depends on
    which rotation is taken (the entries of R are rounded at 2^-24 and multiplied by coordinates of hundreds of metres).  So here,
    and only here, the yardstick follows the kernel's choice instead of LAPACK's: V from the one-sided Jacobi sweep
    (jacobi_svd3, restated in pose_ref.jacobi_svd3), u1 = the unit vector of the coordinate axis on which |u0| is smallest, made
    orthogonal to u0 (kabsch.hip, jacobi_svd3: "rank 1: any unit vector orthogonal to u0"), u2 = u0 x u1 ("rank <= 2: complete
    the basis")."""
    _, V = PR.jacobi_svd3(H)
    g = (H @ V).T  # g[c] = column c of H V, sorted by descending norm like V
    s = np.linalg.norm(g, axis=1)
    assert s[0] > 0.0 and not s[1] > 1e-14 * s[0]
    u0 = g[0] / s[0]
    k = 0 if (abs(u0[0]) <= abs(u0[1]) and abs(u0[0]) <= abs(u0[2])) else (1 if abs(u0[1]) <= abs(u0[2]) else 2)
    e = np.zeros(3)
    e[k] = 1.0
    w = e - (e @ u0) * u0
    u1 = w / np.sqrt(w @ w)
    return np.stack([u0, u1, np.cross(u0, u1)], axis=1), V


def _pose_update_f32(cnt, s_a, s_b, s_ab, denom_count):
    """icp_pose_step from the float64 sums: fp32 centroids sum / (float(cnt) + 1e-6f), H expanded in float64 and rounded to fp32,
    float64 SVD, fp32 R, t = fp32(cB - R cA) with the fp32 R.  Returns the fp32 dT."""
    denom = np.float32(denom_count) + np.float32(1e-6)
    cA, cB = s_a.astype(np.float32) / denom, s_b.astype(np.float32) / denom
    cA64, cB64 = cA.astype(np.float64), cB.astype(np.float64)
    H = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            H[r, c] = ((s_ab[r, c] - cA64[r] * s_b[c]) - s_a[r] * cB64[c]) + (cnt * cA64[r]) * cB64[c]
    H = H.astype(np.float32).astype(np.float64)  # the reference holds H in fp32
    U, sig, Vt = np.linalg.svd(H)
    V = Vt.T
    if sig[0] > 0.0 and not sig[1] > 1e-14 * sig[0]:
        U, V = _rank_one_basis(H)
    R = (V @ np.diag([1.0, 1.0, np.linalg.det(V) * np.linalg.det(U)]) @ U.T).astype(np.float32)
    dT = np.eye(4, dtype=np.float32)
    dT[:3, :3] = R
    dT[:3, 3] = (cB64 - R.astype(np.float64) @ cA64).astype(np.float32)
    return dT


def _matmul4_f32(A, B):
    """The fp32 4x4 product accumulated in k order from 0.f, every operation rounded."""
    out = np.zeros((4, 4), np.float32)
    for k in range(4):
        out = out + A[:, k:k + 1] * B[k:k + 1, :]
    return out


def icp_f32_storage(src, tgt, T0, radius, max_iter, rel_fitness=1e-6, rel_rmse=1e-6, trace=True, s=1.0, c=(0.0, 0.0, 0.0),
                    variant=None):
    """The loop with fp32 storage.  The roundings, in the kernel's order:
      metric points x / s + c in fp32; a = T x in fp32 as ((t0 x + t1 y) + t2 z) + t3; float64 sums of count, |a - b|^2, a, b
      and a b^T; fp32 centroids sum / (float(cnt) + 1e-6f); H from the expanded form, rounded to fp32; float64 3x3 SVD and
      R = V diag(1, 1, det) U^T; fp32 dT; the fp32 product dT . T in k order; fp32 fitness and RMSE, compared in fp32.
    `variant` names one of the deliberately WRONG loops of VARIANTS (test_icp_step_ref_host.py: the rule must see each)."""
    assert variant is None or variant in VARIANTS, variant
    s32, c32 = np.float32(s), np.asarray(c, np.float32)
    src = ((np.asarray(src, np.float32).reshape(-1, 3) / s32).astype(np.float32) + c32).astype(np.float32)
    tgt = ((np.asarray(tgt, np.float32) / s32).astype(np.float32) + c32).astype(np.float32)
    tgt64 = tgt.astype(np.float64)
    T, r2, n = np.asarray(T0, np.float32).copy(), _radius2(radius), len(src)
    rel_fitness, rel_rmse = np.float32(rel_fitness), np.float32(rel_rmse)

    def evaluate(T):
        x, y, z = src[:, 0], src[:, 1], src[:, 2]
        a = np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1)
        assert a.dtype == np.float32
        ev = _evaluation(T.astype(np.float64), a.astype(np.float64), tgt64, r2, n)
        keep = ev["mask"].copy()
        if variant == "drop_last_chunk" and n:
            keep[(n - 1) // 256 * 256:] = False
        A, B = a[keep].astype(np.float64), tgt64[ev["idx"][keep]]
        cnt = int(keep.sum())
        diff = A - B
        sq = ((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]).sum()
        if variant == "expanded_residual":
            sq = _expanded_d_f32(a[keep], tgt[ev["idx"][keep]]).astype(np.float64).sum()
        with np.errstate(invalid="ignore"):
            ev.update(cnt_used=cnt, sum_sq=float(sq), fitness=np.float32(cnt / n) if n else np.float32(0.0),
                      rmse=np.float32(np.sqrt(sq / cnt)) if cnt else np.float32(0.0))
        ev["sums"], ev["a"] = (A.sum(axis=0), B.sum(axis=0), A.T @ B), a
        return ev

    ev = evaluate(T)
    out, it = [ev], 0
    while it < max_iter:
        s_a, s_b, s_ab = ev["sums"]
        dT = _pose_update_f32(float(ev["cnt_used"]), s_a, s_b, s_ab, n if variant == "divide_by_n" else ev["cnt_used"])
        T = _matmul4_f32(T, dT) if variant == "compose_right" else _matmul4_f32(dT, T)
        it += 1
        ev2 = evaluate(T)
        out.append(ev2)
        conv = bool(np.abs(ev["fitness"] - ev2["fitness"]) < rel_fitness and np.abs(ev["rmse"] - ev2["rmse"]) < rel_rmse)
        ev = ev2
        if conv:
            break
    res = _result(out, it, trace)
    res["T"] = T.copy()  # fp32
    return res


# ----------------------------------------------------------------------------------------------------------- the rule
def spacing32(x):
    """One fp32 spacing of the float64 value(s) x."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def rule_bar(f64, yard):
    f64 = np.asarray(f64, np.float64)
    return np.maximum(RATIO * np.abs(np.asarray(yard, np.float64) - f64), spacing32(f64))


def rule_ok(got, f64, yard):
    """|got - f64| <= max(RATIO |yard - f64|, one fp32 spacing of f64), entry-wise; a NaN misses."""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    return bool(np.all(np.abs(got - f64) <= rule_bar(f64, yard)))


def rule_report(what, got, f64, yard):
    """The rule's figures in one line: worst |got - f64|, the yardstick's worst error, the worst share of the bar used."""
    got, f64, yard = (np.asarray(v, np.float64) for v in (got, f64, yard))
    err, bar = np.abs(got - f64), rule_bar(f64, yard)
    return "%s: |got - f64| %.3e  |yard - f64| %.3e  worst err / bar %.3f" % (what, np.max(err), np.max(np.abs(yard - f64)), np.max(err / bar))


def margins_hold(*runs):
    """The margin condition over every evaluation of the given trajectories (results of icp_f64 / icp_f32_storage with trace)."""
    return all(ev["sel_margin"] >= ev["needed"] and ev["rad_margin"] >= ev["needed"] for run in runs for ev in run["trace"])


def same_correspondences(run_a, run_b):
    ta, tb = run_a["trace"], run_b["trace"]
    return len(ta) == len(tb) and all(np.array_equal(x["mask"], y["mask"]) and np.array_equal(x["idx"][x["mask"]], y["idx"][y["mask"]])
                                      for x, y in zip(ta, tb))
