"""Holds tests/rawicp_ref.py on the CPU: the brute-force search against scipy's k-d tree, the kernel-order loop against the LAPACK
loop, the recorded ratios, the margin condition, the stop rule, and that the rule sees each deliberately wrong variant.
``python tests/test_rawicp_ref_host.py`` prints the measured ratios that rawicp_ref.py records."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_step_ref as ISR  # noqa: E402
import rawicp_ref as RR  # noqa: E402

MAX_ITER = 60


@functools.lru_cache(maxsize=None)
def runs():
    """{name: (problem, one-update ref, one-update lapack, loop ref, loop lapack)} of the well-posed problems, computed once."""
    out = {}
    for name, pb in RR.well_posed_problems():
        out[name] = (pb, RR.icp_raw_ref(*pb, 1, 0.0, 0.0), RR.icp_raw_lapack(*pb, 1, 0.0, 0.0), RR.icp_raw_ref(*pb, MAX_ITER),
                     RR.icp_raw_lapack(*pb, MAX_ITER))
    return out


def all_search_problems():
    out = [(n, pb) for n, pb in RR.well_posed_problems()]
    out += [("radius/%g" % s, RR.radius_lattice(s)) for s in RR.SHIFTS]
    out.append(("ties", RR.tie_pair()))
    return out


def test_search_agrees_with_ckdtree():
    from scipy.spatial import cKDTree
    for name, (src, tgt, T, radius) in all_search_problems():
        a = RR.transform(T, src)
        s = RR.search(a, tgt, radius)
        t64 = tgt.astype(np.float64)
        d, j = cKDTree(t64).query(a, k=1)
        # the tree's distance is a square root; compare where the nearest is unambiguous and away from the radius
        clear = (s["second"] - s["lo"] > 1e-9) & (np.abs(s["lo"] - radius * radius) > 1e-9)
        assert clear.sum() > 0.5 * len(a) or name.startswith(("radius", "ties")), name
        assert np.array_equal(j[clear], s["near"][clear]), name
        assert np.allclose(d[clear] ** 2, s["lo"][clear], rtol=1e-12, atol=1e-18), name
        assert np.array_equal((d[clear] < radius), s["mask"][clear]), name


def test_radius_lattice_is_exact():
    for shift in RR.SHIFTS:
        src, tgt, T, radius = RR.radius_lattice(shift)
        a = RR.transform(T, src)
        at, below, above = RR.search(a, tgt, radius), RR.search(a, tgt, np.nextafter(radius, 0)), RR.search(a, tgt, np.nextafter(radius, 1))
        n_edge, n_in = 125 * 6, 125 * 3
        assert at["mask"].sum() == n_in and below["mask"].sum() == n_in and above["mask"].sum() == n_in + n_edge
        assert np.all(at["lo"][~at["mask"]] == 0.25)


def test_ties_go_to_the_lowest_row():
    src, tgt, T, radius = RR.tie_pair()
    s = RR.search(RR.transform(T, src), tgt, radius)
    hit = s["idx"][s["mask"]]
    assert s["mask"].sum() > 900
    for j in hit[:200]:
        twins = np.nonzero((tgt == tgt[j]).all(axis=1))[0]
        assert len(twins) == 2 and j == twins.min()


def test_two_loops_make_identical_trajectories():
    for name, (pb, r1, l1, rl, ll) in runs().items():
        assert RR.same_trajectory(r1, l1), name
        assert RR.same_trajectory(rl, ll), name
        assert rl["iters"] < MAX_ITER, (name, rl["iters"])


def measured_ratios(report=False):
    worst_r, worst_t = 0.0, 0.0
    for name, (pb, r1, l1, rl, ll) in runs().items():
        for kind, ref, lap in (("one", r1, l1), ("loop", rl, ll)):
            st = RR.last_update_stats(lap, pb[0])
            rr, rt = RR.pose_ratios(ref["T"], lap["T"], st)
            if report:
                print("%-16s %-4s iters %2d  ratio R %10.3f  ratio t %10.3f  cond %.2e |cA| %.1f" % (name, kind, ref["iters"], rr, rt, st["cond"], st["ncA"]))
            worst_r, worst_t = max(worst_r, rr), max(worst_t, rt)
    return worst_r, worst_t


def test_ratios_are_the_recorded_ones():
    worst_r, worst_t = measured_ratios()
    assert RR.MEASURED_RATIO_R / 2 <= worst_r <= RR.MEASURED_RATIO_R * 2, worst_r
    assert RR.MEASURED_RATIO_T / 2 <= worst_t <= RR.MEASURED_RATIO_T * 2, worst_t
    assert RR.C_R64 == 4 * RR.MEASURED_RATIO_R and RR.C_T64 == 4 * RR.MEASURED_RATIO_T


def test_restatement_meets_its_own_bars():
    for name, (pb, r1, l1, rl, ll) in runs().items():
        for ref, lap in ((r1, l1), (rl, ll)):
            assert RR.pose_check(ref["T"], lap["T"], RR.last_update_stats(lap, pb[0])) is None, name


def test_margins_hold_on_every_trajectory():
    for name, (pb, r1, l1, rl, ll) in runs().items():
        assert RR.margins_hold(r1, l1, rl, ll), name


def test_stop_rule_is_decided():
    for name, (pb, r1, l1, rl, ll) in runs().items():
        assert ISR.stop_rule_is_decided(rl) and ISR.stop_rule_is_decided(ll), name


def _seen(variant_run, ref, lap, pb):
    """The rule sees a wrong loop: another trajectory, a T outside the bars, or an RMSE outside its bar."""
    if variant_run["iters"] != lap["iters"] or variant_run["fitness"] != lap["fitness"]:
        return True
    if RR.pose_check(variant_run["T"], lap["T"], RR.last_update_stats(lap, pb[0])) is not None:
        return True
    return not RR.rmse_ok(variant_run["rmse"], ref["rmse"], lap["rmse"])


def test_fp32_expanded_selection_fails_at_80_m(capsys):
    src, tgt, T0, Tt, radius = RR.ring_pair()
    a = RR.transform(T0, src)
    exact, wrong = RR.search(a, tgt, radius), RR.search_fp32_expanded(a, tgt, radius)
    differ = int((exact["idx"] != wrong["idx"]).sum())
    with capsys.disabled():
        print("\nfp32 expanded selection on the ring pair (+-80 m, radius 0.2, %d rows): %d correspondences differ from the float64 "
              "brute force" % (len(a), differ))
    assert differ > 0
    name = "ring/0"
    pb, r1, l1, rl, ll = runs()[name]
    assert _seen(RR.icp_raw_ref(*pb, MAX_ITER, variant="fp32_expanded"), rl, ll, pb)


def test_le_radius_is_seen():
    src, tgt, T, radius = RR.radius_lattice(0.0)
    a = RR.transform(T, src)
    assert RR.search(a, tgt, radius, strict=False)["mask"].sum() != RR.search(a, tgt, radius)["mask"].sum()


def test_ties_highest_is_seen():
    src, tgt, T, radius = RR.tie_pair()
    a = RR.transform(T, src)
    assert not np.array_equal(RR.search(a, tgt, radius, ties="highest")["idx"], RR.search(a, tgt, radius)["idx"])


@pytest.mark.parametrize("variant", ["means_1e-6", "compose_right"])
def test_wrong_update_is_seen(variant):
    seen = 0
    for name, (pb, r1, l1, rl, ll) in runs().items():
        seen += _seen(RR.icp_raw_ref(*pb, 1, 0.0, 0.0, variant=variant), r1, l1, pb)
    assert seen > 0, variant


if __name__ == "__main__":
    r, t = measured_ratios(report=True)
    print("worst rotation ratio %.4g, worst translation ratio %.4g" % (r, t))
    for name, (pb, r1, l1, rl, ll) in runs().items():
        print(name, "iters", rl["iters"], "fitness", rl["fitness"], "rmse", rl["rmse"], "margins", RR.margins_hold(r1, l1, rl, ll),
              "decided", ISR.stop_rule_is_decided(rl), "min sel", min(e["sel_margin"] for e in rl["trace"]),
              "min rad", min(e["rad_margin"] for e in rl["trace"]), "needed", max(e["needed"] for e in rl["trace"]))
