"""The pose back end on the MI355X -- the thresholded 1-NN search, the Kabsch solve (dense and fused with the gather), RE/TE, the
search inside the ICP loop and the point loss -- against the exact and float64 references of tests/pose_ref.py, at the ties, edges
and conditionings that random clouds never produce.  The references are held on the CPU by tests/test_pose_ref_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_ref as PR
from oracle import scream_ref as O
from scream_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    from scream_amd import _lib
    _lib.load()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def i32(a):
    return torch.tensor(np.asarray(a).tolist(), dtype=torch.int32, device=DEV)


def pack(clouds):
    """Clouds [n_i,3] -> (packed fp32 [rows,3] with zero padding to multiples of 128 and at least 128 rows each, row0)."""
    row0, r = [], 0
    for x in clouds:
        row0.append(r)
        r += max(128, (len(x) + 127) // 128 * 128)
    out = np.zeros((r, 3), np.float32)
    for x, r0 in zip(clouds, row0):
        out[r0:r0 + len(x)] = x
    return out, row0 + [r]


def search(queries, targets, s, thresh):
    """One packed scream_nn_search.  Returns per pair (idx, dmin, valid) and the rows that belong to no query cloud."""
    q, q0 = pack(queries)
    r, r0 = pack(targets)
    idx, dmin, valid = ops.nn_search(dev(q), dev(r), i32(q0[:-1]), i32([len(x) for x in queries]), i32(r0[:-1]), i32([len(x) for x in targets]),
                                     dev(np.asarray(s, np.float32)), max(len(x) for x in queries), max(len(x) for x in targets), thresh)
    idx, dmin, valid = idx.cpu().numpy(), dmin.cpu().numpy(), valid.cpu().numpy()
    pad = np.ones(len(q), bool)
    out = []
    for x, a in zip(queries, q0):
        sl = slice(a, a + len(x))
        pad[sl] = False
        out.append((idx[sl], dmin[sl], valid[sl]))
    return out, (idx[pad], dmin[pad], valid[pad])


def assert_search(got, want, what):
    idx, dmin, valid = got
    d_w, i_w, v_w = want
    np.testing.assert_array_equal(idx, i_w, err_msg="idx, %s" % (what,))
    np.testing.assert_array_equal(dmin, d_w, err_msg="dmin, %s" % (what,))
    np.testing.assert_array_equal(valid.astype(bool), v_w, err_msg="valid, %s" % (what,))


def assert_padding(pad):
    idx, dmin, valid = pad
    assert (idx == -1).all() and np.isposinf(dmin).all() and not valid.any()


# ---------------------------------------------------------------------------------------------------- the 1-NN search
IDENTICAL_M = (1, 31, 32, 33, 1023, 1024, 1025, 4097, 8191)


def test_nn_all_targets_identical_index_zero_wins():
    """Every target is the same point: every distance ties, across chunk edges (32) and target-range splits, and index 0 must win.
    As single pairs, and as one packed call whose shared split length cuts the smaller clouds at odd places.  (Every split of
    these calls is shorter than one LDS tile: the tile edge is pinned by the *_across_lds_tiles tests below.)"""
    rng = np.random.default_rng(0)
    qs = [PR.lattice_cloud(rng, 300) for _ in IDENTICAL_M]
    pts = [PR.lattice_cloud(rng, 1) for _ in IDENTICAL_M]
    ts = [np.repeat(p, m, axis=0) for p, m in zip(pts, IDENTICAL_M)]
    wants = [PR.lattice_nn(q, t, 1.0, 5000.0) for q, t in zip(qs, ts)]
    for q, t, m, want in zip(qs, ts, IDENTICAL_M, wants):
        assert (want[1] == 0).all() and 0 < want[2].sum() < 300
        got, pad = search([q], [t], [1.0], 5000.0)
        assert_search(got[0], want, "M = %d alone" % m)
        assert_padding(pad)
    got, pad = search(qs, ts, [1.0] * len(qs), 5000.0)
    for g, m, want in zip(got, IDENTICAL_M, wants):
        assert_search(g, want, "M = %d in the packed call" % m)
    assert_padding(pad)


def test_nn_tie_lattice_and_threshold_equality():
    """Queries with 8, 4 and 2 equidistant nearest targets on a shuffled integer lattice: the lowest index among them, the exact
    distance, and `valid` strict at d == thresh (the body centres sit at exactly 0.75) but set at the next threshold above."""
    q, t, ties = PR.tie_lattice()
    body = ties == 8
    for thresh, body_valid in ((np.float32(0.75), False), (np.nextafter(np.float32(0.75), np.float32(1)), True)):
        want = PR.lattice_nn(q, t, 1.0, thresh)
        assert want[2][body].all() == body_valid and want[2][body].any() == body_valid and want[2][~body].all()
        got, pad = search([q], [t], [1.0], float(thresh))
        assert_search(got[0], want, "thresh %r" % thresh)
        assert_padding(pad)
    # a power-of-two scale keeps the arithmetic exact: the same answers through the division
    got, _ = search([q * np.float32(0.25)], [t * np.float32(0.25)], [0.25], 0.75)
    assert_search(got[0], PR.lattice_nn(q, t, 1.0, 0.75), "s = 1/4")


def test_nn_planted_duplicates_lower_position_wins():
    """The nearest target of every query of a pair sits at TWO positions of the target array, drawn from the chunk, split and array
    edges; one packed call holds every pair of positions (planting at (i, j) and at (j, i) is the same array).  The lower wins.
    (Splits of 373 targets here; test_nn_planted_duplicates_across_lds_tiles has the two positions in different tiles of a block.)"""
    M = 4100
    pos = (0, 31, 32, 33, 1023, 1024, 1025, M // 2 - 1, M // 2 + 1, M - 1)
    rng = np.random.default_rng(1)
    base = PR.lattice_cloud(rng, M)
    P = np.array([[3.0, -2.0, 5.0]], np.float32)
    base = np.where((np.abs(base - P).max(axis=1) < 4)[:, None], base + np.float32(16), base).astype(np.float32)  # nothing else near P
    q = (P + rng.integers(-2, 3, size=(64, 3)) * 0.25).astype(np.float32)
    pairs = [(i, j) for a, i in enumerate(pos) for j in pos[a + 1:]]
    ts = []
    for i, j in pairs:
        t = base.copy()
        t[i] = t[j] = P
        ts.append(t)
    got, pad = search([q] * len(pairs), ts, [1.0] * len(pairs), 1.0)
    for g, t, (i, j) in zip(got, ts, pairs):
        want = PR.lattice_nn(q, t, 1.0, 1.0)
        assert (want[1] == i).all()
        assert_search(g, want, "positions %d, %d" % (i, j))
    assert_padding(pad)


def test_nn_negative_computed_distances_bit_for_bit():
    """Coincident points 100 m from the origin: the expanded form gives residues of either sign, so the keys of negative floats go
    through the merge of the target-range splits (M = 12 000), and equal negative minima must still resolve to the lowest index."""
    q, t = PR.coincident_far_cloud()
    d, idx, _ = O.nn_search_exact(q, t, 1.0)
    assert (d < 0).mean() >= 0.25
    got, pad = search([q], [t], [1.0], 0.0)  # thresh 0: valid is the sign of the minimum
    assert_search(got[0], (d, idx, d < 0), "coincident clouds at |x| ~ 100")
    assert_padding(pad)
    got, _ = search([q, q[:700]], [t, t[:5000]], [1.0, 1.0], 0.0)  # and in a packed call with another split length
    assert_search(got[0], (d, idx, d < 0), "packed")
    d2, idx2, _ = O.nn_search_exact(q[:700], t[:5000], 1.0)
    assert_search(got[1], (d2, idx2, d2 < 0), "packed, second pair")


# ---- the same ties where ONE block scans several LDS tiles ----------------------------------------------------------------------
# A block scans its target range in tiles of 1024 and carries best / bi from tile to tile; the calls above are split so finely (the
# heuristic fills the 256 CUs) that no block ever sees a second tile.  The calls below are shaped like the evaluation's, many pairs at
# once, so that a split is longer than a tile; pose_ref.nn_split_plan restates the heuristic and each test asserts its geometry.
def _assert_multi_tile(name, queries, targets):
    call = (max(len(x) for x in queries), max(len(x) for x in targets), len(queries))
    assert call == PR.TILE_EDGE_CALLS[name], call
    per, splits = PR.nn_split_plan(*call)
    assert per > PR.NN_RT, (call, per, splits)
    return per, splits


def test_nn_all_targets_identical_across_lds_tiles():
    """256 pairs in one call, one split of 2100 targets per block (tiles 0-1023, 1024-2047, 2048-2099): every target identical, so
    the tie between tile 0 and the later tiles must go to index 0, for target counts on either side of the tile edges."""
    rng = np.random.default_rng(20)
    Ms = (2100, 1, 1023, 1024, 1025, 2047, 2048, 2049)
    qs = [PR.lattice_cloud(rng, 64) for _ in range(256)]
    ts = [np.repeat(PR.lattice_cloud(rng, 1), Ms[i % len(Ms)], axis=0) for i in range(256)]
    assert _assert_multi_tile("identical", qs, ts) == (2100, 1)
    got, pad = search(qs, ts, [1.0] * 256, 5000.0)
    for i, (g, q, t) in enumerate(zip(got, qs, ts)):
        want = PR.lattice_nn(q, t, 1.0, 5000.0)
        assert (want[1] == 0).all()
        assert_search(g, want, "pair %d, M = %d" % (i, len(t)))
    assert_padding(pad)


def test_nn_planted_duplicates_across_lds_tiles():
    """The nearest target of a pair's queries sits at two positions of a 2100-target array that ONE block scans in three tiles:
    positions on the chunk edges, on both tile edges (1023 | 1024, 2047 | 2048) and at the ends, every pair of them.  The lower wins,
    also when the two copies sit in different tiles."""
    M = 2100
    pos = (0, 31, 32, 33, 1023, 1024, 1025, M // 2 - 1, M // 2 + 1, 2047, 2048, M - 1)
    rng = np.random.default_rng(21)
    base = PR.lattice_cloud(rng, M)
    P = np.array([[3.0, -2.0, 5.0]], np.float32)
    base = np.where((np.abs(base - P).max(axis=1) < 4)[:, None], base + np.float32(16), base).astype(np.float32)  # nothing else near P
    q = (P + rng.integers(-2, 3, size=(64, 3)) * 0.25).astype(np.float32)
    pairs = [(i, j) for a, i in enumerate(pos) for j in pos[a + 1:]]
    pairs = [pairs[k % len(pairs)] for k in range(256)]  # 66 pairs of positions, repeated to the 256 pairs of the geometry
    ts = []
    for i, j in pairs:
        t = base.copy()
        t[i] = t[j] = P
        ts.append(t)
    assert _assert_multi_tile("planted", [q] * 256, ts) == (2100, 1)
    got, pad = search([q] * 256, ts, [1.0] * 256, 1.0)
    for g, t, (i, j) in zip(got[:66], ts, pairs):
        want = PR.lattice_nn(q, t, 1.0, 1.0)
        assert (want[1] == i).all()
        assert_search(g, want, "positions %d, %d" % (i, j))
    for k in range(66, 256):
        for a, b in zip(got[k], got[k - 66]):
            np.testing.assert_array_equal(a, b)
    assert_padding(pad)


def test_nn_tie_lattice_across_lds_tiles():
    """The tie lattice as 64 pairs of one call: 4 splits of 1458 targets, each scanned as a tile of 1024 and one of 434, so the 8 / 4 /
    2 equidistant targets of a query fall on both sides of tile edges AND of split edges.  d == thresh stays invalid."""
    q, t, ties = PR.tie_lattice()
    assert _assert_multi_tile("tie_lattice", [q] * 64, [t] * 64) == (1458, 4)
    want = PR.lattice_nn(q, t, 1.0, 0.75)
    got, pad = search([q] * 64, [t] * 64, [1.0] * 64, 0.75)
    for k, g in enumerate(got):
        assert_search(g, want, "pair %d" % k)
    assert_padding(pad)


def test_nn_negative_computed_distances_across_lds_tiles():
    """Coincident clouds at 100 m as 64 pairs of one call: 2 splits of 6000 targets, six tiles each; negative minima are carried from
    tile to tile inside a block and merged between the two splits."""
    q, t = PR.coincident_far_cloud()
    q = q[:1500].copy()
    assert _assert_multi_tile("negative", [q] * 64, [t] * 64) == (6000, 2)
    d, idx, _ = O.nn_search_exact(q, t, 1.0)
    assert (d < 0).mean() >= 0.25
    got, pad = search([q] * 64, [t] * 64, [1.0] * 64, 0.0)
    for k, g in enumerate(got):
        assert_search(g, (d, idx, d < 0), "pair %d" % k)
    assert_padding(pad)


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1023, 1024, 1025, 1279, 4097])
def test_nn_query_block_edges_with_empty_clouds_in_the_batch(N):
    """Query counts on the 256-thread and 1024-query block edges, against a small and a multi-tile target cloud, in a packed batch
    that holds an empty query cloud and an empty target cloud between them."""
    rng = np.random.default_rng(N)
    qa, qc, qd = PR.lattice_cloud(rng, N), PR.lattice_cloud(rng, N), PR.lattice_cloud(rng, N)
    ta, tb, td = PR.lattice_cloud(rng, 37), PR.lattice_cloud(rng, 100), PR.lattice_cloud(rng, 2500)
    empty = np.zeros((0, 3), np.float32)
    thresh = 300.0
    got, pad = search([qa, empty, qc, qd], [ta, tb, empty, td], [1.0, 1.0, 1.0, 1.0], thresh)
    assert_search(got[0], PR.lattice_nn(qa, ta, 1.0, thresh), "N = %d against M = 37" % N)
    assert len(got[1][0]) == 0
    assert_search(got[2], PR.lattice_nn(qc, empty, 1.0, thresh), "the empty target cloud")
    assert (got[2][0] == -1).all() and np.isposinf(got[2][1]).all() and not got[2][2].any()
    assert_search(got[3], PR.lattice_nn(qd, td, 1.0, thresh), "N = %d against M = 2500" % N)
    assert_padding(pad)


@pytest.mark.parametrize("B,N,M", [(2, 300, 301), (1, 65534, 40), (1, 65535, 33), (1, 70000, 40)])
def test_square_distance_equals_the_integer_distances(B, N, M):
    from scream_amd.geometry import square_distance
    rng = np.random.default_rng(N)
    a = np.stack([PR.lattice_cloud(rng, N) for _ in range(B)])
    b = np.stack([PR.lattice_cloud(rng, M) for _ in range(B)])
    np.testing.assert_array_equal(square_distance(dev(a), dev(b)).cpu().numpy(), PR.lattice_square_distance(a, b))


# --------------------------------------------------------------------------------------------------- the dense solve
def solve(A, B, w=None, thr=0.0):
    from scream_amd.geometry import rigid_transform_3d
    wt = None if w is None else dev(np.asarray(w, np.float32).copy())[None]
    return rigid_transform_3d(dev(A)[None], dev(B)[None], wt, thr).cpu().numpy()[0]


@pytest.mark.parametrize("name", [row[0] for row in PR.kabsch_case_table()])
def test_kabsch_case_against_float64(name):
    """One case of pose_ref.kabsch_case_table(): conditioning (planar, near-planar down to 1e-12, near-collinear, repeated singular
    values), reflections, offsets to 1000 m, scales 2^-40 .. 2^20, K on the 256-thread stride edges, weights.  Well-posed cases are
    held to the Kabsch bar against kabsch_f64, the others to properness, as the table says.
    (The scale_-40 cases are the ones the absolute term of the old Jacobi stop rule failed: no rotation was applied at all.)"""
    A, B, w, thr, kind = PR.kabsch_case(name)
    ref = PR.kabsch_f64(A, B, w, thr)
    T = solve(A, B, w, thr)
    if kind == "bar":
        print("%s: cond %.2e, share of the bar with C_R = C_T = 1: R %.3f, t %.3f" % ((name, ref["cond"]) + PR.kabsch_ratios(T, ref)))
    miss = PR.kabsch_check(T, ref, kind)
    assert miss is None, (name, kind, miss)


def test_kabsch_thousand_small_problems_in_one_call_equal_each_alone():
    from scream_amd.geometry import rigid_transform_3d
    A, B, w, thr = PR.small_problem_batch()
    dA, dB, dw = dev(A), dev(B), dev(w)
    T = rigid_transform_3d(dA, dB, dw.clone(), thr)
    alone = torch.cat([rigid_transform_3d(dA[i:i + 1].contiguous(), dB[i:i + 1].contiguous(), dw[i:i + 1].clone(), thr) for i in range(len(A))])
    assert torch.equal(T, alone)
    T = T.cpu().numpy()
    misses = []
    for i in range(len(A)):
        ref = PR.kabsch_f64(A[i], B[i], w[i], thr)
        assert ref["cond"] < PR.WELL_POSED_LIMIT
        miss = PR.kabsch_check(T[i], ref, "bar")
        if miss:
            misses.append((i, miss))
    assert not misses, misses[:5]


def test_kabsch_weight_conventions():
    from scream_amd.geometry import rigid_transform_3d
    rng = np.random.default_rng(3)
    A, B = PR._iso(rng, 300)
    dA, dB = dev(A)[None], dev(B)[None]
    none = rigid_transform_3d(dA, dB)
    assert torch.equal(none, rigid_transform_3d(dA, dB, torch.ones(1, 300, device=DEV), 0))  # w = None is w = ones, bit for bit
    half = torch.full((1, 300), 0.5, device=DEV)
    assert torch.equal(rigid_transform_3d(dA, dB, half.clone(), 0.5), rigid_transform_3d(dA, dB, half.clone(), 0))  # w == thr is kept
    assert PR.kabsch_check(rigid_transform_3d(dA, dB, half.clone(), 0.5).cpu().numpy()[0], PR.kabsch_f64(A, B, np.full(300, 0.5, np.float32), 0.5), "bar") is None
    np.testing.assert_array_equal(rigid_transform_3d(dA, dB, half.clone(), np.nextafter(np.float32(0.5), np.float32(1))).cpu().numpy()[0],
                                  np.eye(4, dtype=np.float32))  # every weight below thr: the exact identity
    w = rng.uniform(0, 1, size=(1, 300)).astype(np.float32)
    dw = dev(w)
    T = rigid_transform_3d(dA, dB, dw, 0.4).cpu().numpy()[0]
    got = dw.cpu().numpy()
    assert (got[w < 0.4] == 0).all() and np.array_equal(got[w >= 0.4], w[w >= 0.4])  # the caller's tensor, as utils.py:151 leaves it
    assert PR.kabsch_check(T, PR.kabsch_f64(A, B, w[0], 0.4), "bar") is None


# ------------------------------------------------------------------------------------------ the fused gather + solve
def corr_call(pb, with_idx=True, valid=None, order=None, n_corr=True):
    order = list(range(len(pb["lens"]))) if order is None else order
    row0, lens = i32(pb["row0"][order]), i32(pb["lens"][order])
    args = (dev(pb["src"]), dev(pb["ref"] if with_idx else pb["ref_rows"]), row0, lens, row0, dev(pb["idx"]) if with_idx else None,
            dev(pb["valid"] if valid is None else valid), dev(pb["s"][order]), dev(pb["c"][order]))
    if n_corr:
        T, n = ops.kabsch_corr(*args)
        return T.cpu().numpy(), n.cpu().numpy()
    from scream_amd import _lib
    T = torch.empty(len(order), 4, 4, device=DEV)
    ptr = [None if a is None else a.data_ptr() for a in args]
    _lib.check(_lib.load().scream_kabsch_corr(*ptr, len(order), T.data_ptr(), None, torch.cuda.current_stream().cuda_stream), "scream_kabsch_corr")
    return T.cpu().numpy(), None


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("name", sorted(PR.CORR_PROBLEMS))
def test_kabsch_corr_against_float64_on_the_gathered_rows(name, with_idx):
    """Every row valid, one row in 1000, and a near-planar and a reflected pair; with idx and in the idx == NULL mode; s not a
    power of two and c 300 m from the origin (x / s + c is rounded to fp32 first, as the reference does)."""
    lens, kinds, every = PR.CORR_PROBLEMS[name]
    pb = PR.corr_problem(lens, kinds, every=every)
    T, n = corr_call(pb, with_idx)
    for p in range(len(lens)):
        ref, K = PR.corr_reference(pb, p, with_idx)
        assert n[p] == K
        miss = PR.kabsch_check(T[p], ref, "bar")
        print("%s pair %d K %d share of the bar: R %.3f t %.3f" % ((name, p, K) + PR.kabsch_ratios(T[p], ref)))
        assert miss is None, (name, p, miss)
    # n_corr == NULL is accepted and changes nothing
    T2, _ = corr_call(pb, with_idx, n_corr=False)
    np.testing.assert_array_equal(T2, T)
    # pairs listed in descending row order: the same poses, permuted
    T3, n3 = corr_call(pb, with_idx, order=[2, 1, 0])
    np.testing.assert_array_equal(T3, T[::-1])
    np.testing.assert_array_equal(n3, n[::-1])


@pytest.mark.parametrize("with_idx", [True, False])
def test_kabsch_corr_pair_without_a_valid_row_between_two_that_have_some(with_idx):
    lens, kinds, every = PR.CORR_PROBLEMS["dense"]
    pb = PR.corr_problem(lens, kinds, every=every)
    T, n = corr_call(pb, with_idx)
    valid = pb["valid"].copy()
    valid[pb["row0"][1]: pb["row0"][2]] = 0
    T0, n0 = corr_call(pb, with_idx, valid=valid)
    np.testing.assert_array_equal(T0[1], np.eye(4, dtype=np.float32))
    assert n0.tolist() == [n[0], 0, n[2]]
    np.testing.assert_array_equal(T0[[0, 2]], T[[0, 2]])  # the neighbours, bit for bit


# ----------------------------------------------------------------------------------------------------------- RE / TE
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_transformation_error_inside_the_float64_interval(n):
    """Relative rotations of 0 .. 180 degrees composed with random poses: RE inside the interval that fp32 rounding of the trace
    allows around float64 (about 1e-3 degrees wide at 5 and 15 degrees, where recall is decided), TE to 4 * 2^-24."""
    P, G, ang = PR.pose_pairs(max(n, 11) if n > 1 else 1, seed=n)
    P, G, ang = P[-n:], G[-n:], ang[-n:]
    re, te = ops.transformation_error_batched(dev(P), dev(G))
    re, te = re.cpu().numpy().astype(np.float64), te.cpu().numpy().astype(np.float64)
    lo, hi = PR.re_interval(P, G)
    re64, te64 = PR.re_te_f64(P, G)
    bad = ~((lo <= re) & (re <= hi))
    assert not bad.any(), list(zip(ang[bad], re[bad], re64[bad], lo[bad], hi[bad]))[:5]
    np.testing.assert_allclose(te, te64, rtol=PR.TE_RTOL, atol=PR.TE_ATOL)
    assert re.shape == (n,)


def test_transformation_error_clamps_give_exactly_0_and_180_degrees():
    rng = np.random.default_rng(9)
    G = np.tile(np.eye(4, dtype=np.float32), (70, 1, 1))
    for i in range(70):
        G[i, :3, :3] = PR.random_rotation(rng)
    up, down = G.copy(), G.copy()
    up[:, :3, :3] *= np.float32(1.01)     # tr = 3.03: x = 1.015 is clamped to 1
    down[:, :3, :3] *= np.float32(-1.01)  # x = -2.015 is clamped to -1
    re_up, _ = ops.transformation_error_batched(dev(up), dev(G))
    re_down, _ = ops.transformation_error_batched(dev(down), dev(G))
    assert (re_up.cpu().numpy() == 0.0).all()
    # acos(-1) = fp32 pi, and pi * 180 / pi with each fp32 operation rounded is exactly 180
    assert np.float32(np.float32(np.float32(np.pi) * np.float32(180.0)) / np.float32(np.pi)) == np.float32(180.0)
    assert (re_down.cpu().numpy() == 180.0).all(), re_down[:3]


# ------------------------------------------------------------------------------------------- the search inside ICP
def _icp(src, tgt, radius, max_iter, search="grid"):
    n, m = len(src), len(tgt)
    return ops.icp_p2p(dev(src), dev(tgt), i32([0]), i32([n]), i32([0]), i32([m]), dev(np.ones(1, np.float32)), dev(np.zeros((1, 3), np.float32)),
                       dev(np.eye(4, dtype=np.float32)[None]), n, m, radius, max_iter, search=search)


def test_icp_grid_search_on_a_lattice_ties_and_points_at_the_radius():
    """A metric-frame lattice problem (s = 1, c = 0, T0 = I, radius 0.5): sources with 8 equidistant targets, sources at exactly the
    radius from their only neighbour (d^2 == thresh: not a correspondence).  Without an update the fitness is the exact count and
    the RMSE the exact value; with updates the whole run is bit for bit that of the brute-force search (a tie resolved differently
    changes b, hence H, hence T)."""
    src, tgt, radius = PR.icp_lattice_problem()
    cnt, rmse = PR.icp_lattice_ref(src, tgt, radius)
    for brute in (False, True):
        T, fr, iters = _icp(src, tgt, radius, 0, search="brute" if brute else "grid")
        fr = fr.cpu().numpy()[0]
        assert fr[0] == np.float32(cnt / len(src)), (brute, fr, cnt)
        assert abs(float(fr[1]) - rmse) <= np.spacing(np.float32(rmse)), (brute, fr, rmse)
        np.testing.assert_array_equal(T.cpu().numpy()[0], np.eye(4, dtype=np.float32))
        assert int(iters[0]) == 0
    for max_iter in (1, 5):
        got = _icp(src, tgt, radius, max_iter)
        want = _icp(src, tgt, radius, max_iter, search="brute")
        for a, b in zip(got, want):
            assert torch.equal(a, b), (max_iter, a, b)
        assert 1 <= int(got[2][0]) <= max_iter


# --------------------------------------------------------------------------------------------------- the point loss
def test_point_loss_pair_lengths_and_a_cloud_at_300_m():
    """Pairs of length 0 (loss 0), 1, 256, 257 and a cloud 300 m from the origin in one packed batch, against the float64 mean of
    the fp32 terms."""
    rng = np.random.default_rng(4)
    lens = [0, 1, 256, 257, 500]
    clouds = [rng.normal(size=(n, 3)).astype(np.float32) for n in lens]
    clouds[4] = (clouds[4] + np.float32(173.2)).astype(np.float32)
    R = np.stack([PR.random_rotation(rng) for _ in lens]).astype(np.float32)
    t = rng.normal(size=(len(lens), 3)).astype(np.float32)
    src, row0 = pack(clouds)
    pred = np.zeros_like(src)
    for p, (r0, n) in enumerate(zip(row0, lens)):
        pred[r0:r0 + n] = (clouds[p].astype(np.float64) @ R[p].astype(np.float64).T + t[p] + 0.01 * rng.normal(size=(n, 3))).astype(np.float32)
    got = ops.point_loss(dev(pred), dev(src), i32(row0[:-1]), i32(lens), dev(R), dev(t)).cpu().numpy().astype(np.float64)
    want = PR.point_loss_f64(pred, src, row0[:-1], lens, R, t)
    assert got[0] == 0.0 and (want[1:] > 0).all()
    np.testing.assert_allclose(got, want, rtol=4 * PR.EPS32, atol=0)
