"""tests/icp_step_ref.py held on the CPU: the float64 loop against oracle/icp_ref.py (scipy's cKDTree), the margin condition on every
problem tests/test_gpu_icp_step.py uses, and proof that the comparison rule bites -- four deliberately wrong variants of the
yardstick each miss it on a designed problem.  No GPU, no import of the code under test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_step_ref as IR
from oracle import icp_ref as ORACLE

UPDATES = 5


def _grid():
    return [(frame, n) for frame in IR.FRAMES for n in IR.LENGTHS]


_RUNS = {}


def runs(frame, n):
    """(problem, icp_f64, icp_f32_storage) of one grid problem over UPDATES updates with the thresholds at 0; computed once."""
    if (frame, n) not in _RUNS:
        prob = IR.lattice_problem(frame, IR.frame_h(frame), n, IR.n_far_for(n))
        _RUNS[frame, n] = (prob, IR.icp_f64(*prob, UPDATES, 0.0, 0.0), IR.icp_f32_storage(*prob, UPDATES, 0.0, 0.0))
    return _RUNS[frame, n]


def misses(wrong, f64, yard):
    """Names of the quantities of the last evaluation of `wrong` that miss the rule against the same evaluation of the references."""
    k = len(wrong["trace"]) - 1
    return [q for q in ("T", "fitness", "rmse") if not IR.rule_ok(wrong["trace"][k][q], f64["trace"][k][q], yard["trace"][k][q])]


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("frame,n", [(f, n) for f in IR.FRAMES for n in (1, 257, 3841)])
def test_icp_f64_agrees_with_the_kdtree_oracle_step_by_step(frame, n):
    from scipy.spatial import cKDTree
    (src, tgt, T0, radius), f64, _ = runs(frame, n)
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    tree = cKDTree(t64)
    for k, ev in enumerate(f64["trace"]):
        assert ev["cnt"] > 0
        T, fit, rmse, it = ORACLE.icp_p2p(s64, t64, T0.astype(np.float64), radius, max_iter=k, rel_fitness=0.0, rel_rmse=0.0)
        assert it == k
        np.testing.assert_allclose(ev["T"], T, rtol=0, atol=1e-12)
        d, j = tree.query(s64 @ ev["T"][:3, :3].T + ev["T"][:3, 3], k=1, distance_upper_bound=radius)
        np.testing.assert_array_equal(np.isfinite(d), ev["mask"])
        np.testing.assert_array_equal(j[ev["mask"]], ev["idx"][ev["mask"]])
        assert fit == ev["fitness"] and abs(rmse - ev["rmse"]) <= 1e-12


@pytest.mark.parametrize("frame", IR.FRAMES)
def test_icp_f64_update_count_equals_the_oracles_under_the_default_stop_rule(frame):
    src, tgt, T0, radius = IR.lattice_problem(frame, IR.frame_h(frame), 257, 3)
    got = IR.icp_f64(src, tgt, T0, radius, 30)
    T, fit, rmse, it = ORACLE.icp_p2p(src.astype(np.float64), tgt.astype(np.float64), T0.astype(np.float64), radius, max_iter=30)
    assert got["iters"] == it and 0 < it < 30
    np.testing.assert_allclose(got["T"], T, rtol=0, atol=1e-12)


def test_icp_f64_goes_on_with_the_identity_where_nothing_is_found():
    """open3d's loop, not the oracle's break: an empty correspondence set is an identity update; the pair stops at its second
    evaluation under positive thresholds and runs to the cap when they are 0."""
    prob = IR.far_only_problem(30, 0.25, 40)
    for run in (IR.icp_f64, IR.icp_f32_storage):
        a, b, z = run(*prob, 7), run(*prob, 7, 0.0, 0.0), run(*prob, 0)
        assert (a["iters"], b["iters"], z["iters"]) == (1, 7, 0)
        for r in (a, b, z):
            assert r["fitness"] == 0 and r["rmse"] == 0 and np.array_equal(np.asarray(r["T"], np.float64), prob[2].astype(np.float64))
    empty = (np.zeros((0, 3), np.float32),) + prob[1:]
    assert IR.icp_f64(*empty, 7)["iters"] == 1 and IR.icp_f32_storage(*empty, 7)["iters"] == 1


# ------------------------------------------------------------------------------------------------ the margin condition
@pytest.mark.parametrize("frame,n", _grid())
def test_margin_condition_on_the_grid(frame, n):
    _, f64, yard = runs(frame, n)
    assert IR.margins_hold(f64, yard), [(ev["sel_margin"], ev["rad_margin"], ev["needed"]) for ev in f64["trace"] + yard["trace"]]
    assert IR.same_correspondences(f64, yard)
    assert f64["trace"][0]["cnt"] == n - IR.n_far_for(n)


@pytest.mark.parametrize("frame", IR.COINCIDENT_FRAMES)
def test_margin_condition_on_the_coincident_clouds(frame):
    prob = IR.coincident_problem(frame)
    f64, yard = IR.icp_f64(*prob, 1000), IR.icp_f32_storage(*prob, 1000)
    assert IR.margins_hold(f64, yard) and IR.same_correspondences(f64, yard)
    assert f64["trace"][0]["rmse"] == 0.0 and yard["trace"][0]["rmse"] == 0.0 and f64["fitness"] == 1.0
    assert f64["iters"] == yard["iters"] == 1


def test_margin_condition_on_the_remaining_gpu_problems():
    for name, prob, max_iter, rel in IR.extra_problems():
        f64, yard = IR.icp_f64(*prob, max_iter, rel, rel), IR.icp_f32_storage(*prob, max_iter, rel, rel)
        assert IR.margins_hold(f64, yard) and IR.same_correspondences(f64, yard), name
        assert f64["iters"] == yard["iters"], name
        if rel > 0:
            assert IR.stop_rule_is_decided(f64, rel) and (f64["iters"] < max_iter or name.startswith("neighbour")), name
    assert tuple(IR.icp_f64(*pb, 30)["iters"] for _, pb in IR.batch_problems()) == IR.BATCH_ITERS
    assert [r["trace"][0]["cnt"] for r in (IR.icp_f64(*pb, 0) for _, pb, _ in IR.degenerate_problems())] == [k for _, _, k in IR.degenerate_problems()]


# --------------------------------------------------------------------------------------------------- the bar bites
def _wrong(frame, n, variant, updates=UPDATES):
    prob, f64, yard = runs(frame, n)
    return misses(IR.icp_f32_storage(*prob, updates, 0.0, 0.0, variant=variant), f64, yard)


def test_the_yardstick_itself_meets_the_rule_trivially_and_a_nan_misses():
    _, f64, yard = runs(30, 257)
    assert misses(yard, f64, yard) == []
    assert not IR.rule_ok(np.nan, f64["rmse"], yard["rmse"])


@pytest.mark.parametrize("frame", (30, 300))
def test_rule_sees_the_rmse_taken_from_the_searchs_expanded_value(frame):
    for n in (257, 3841):
        assert "rmse" in _wrong(frame, n, "expanded_residual"), (frame, n)


@pytest.mark.parametrize("n", (257, 3841))
def test_rule_sees_a_dropped_last_chunk(n):
    """At 257 the last chunk holds one row; at 3 841 it is the chunk that wraps into group 0."""
    for frame in IR.FRAMES:
        got = _wrong(frame, n, "drop_last_chunk")
        assert "fitness" in got, (frame, n, got)


def test_rule_sees_the_update_composed_on_the_wrong_side():
    """After ONE update: the loop is self-correcting, so later updates pull a wrongly composed pose back to the fit."""
    for frame in IR.FRAMES:
        assert "T" in _wrong(frame, 257, "compose_right", updates=1), frame


def test_rule_sees_centroids_divided_by_the_source_length():
    assert IR.n_far_for(257) > 0
    for frame in (30, 300):
        assert "T" in _wrong(frame, 257, "divide_by_n", updates=1), frame


def test_expanded_value_sums_negative_on_coincident_clouds():
    """Why the kernel may not use that sum: on coincident clouds away from the origin it is a rounding residue of either sign
    instead of 0, and where it is negative the RMSE is the square root of a negative number -- NaN, which no stop rule accepts."""
    sums = {}
    for frame in (3, 30):
        prob = IR.coincident_problem(frame)
        ev = IR.icp_f32_storage(*prob, 0, variant="expanded_residual")["trace"][0]
        sums[frame] = ev["sum_sq"]
        assert ev["sum_sq"] != 0.0 and (np.isnan(ev["rmse"]) if ev["sum_sq"] < 0 else ev["rmse"] > 0), (frame, ev["sum_sq"], ev["rmse"])
        good = IR.icp_f32_storage(*prob, 0)["trace"][0]
        assert good["sum_sq"] == 0.0 and good["rmse"] == 0.0
    assert min(sums.values()) < 0, sums
