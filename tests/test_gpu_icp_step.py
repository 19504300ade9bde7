"""The ICP loop on the MI355X (scream_icp_p2p: icp_pose_step + icp_store_partial of csrc/icp_p2p.hip) against the float64 loop of
tests/icp_step_ref.py: the chunk-partial sums at their group boundaries, the expanded covariance, the centroid denominators, the
composition dT . T, both parities of the buffers, the freeze of stopped pairs, the stop rules, empty and partnerless sources, and
frames 30 m and 300 m from the origin.

One rule for every float compared (T entry-wise, RMSE and fitness as scalars):
    |gpu - f64| <= max(2 |yardstick - f64|, one fp32 spacing of the float64 value)
with the yardstick icp_f32_storage, the loop with exactly the documented fp32 roundings.  Every test first asserts, on the CPU, the
margin condition under which the GPU's search provably picks the references' correspondences (icp_step_ref.py); fitness is then
exact.  The references are held by tests/test_icp_step_ref_host.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_step_ref as IR
import pose_ref as PR
from scream_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJECTORY_LENGTHS = (257, 3841)
TRAJECTORY_UPDATES = 6


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
    return out, row0


def icp_args(problems, max_iter, rel):
    """The positional arguments of ops.icp_p2p / ops.IcpRun for the problems as one packed call."""
    radius = problems[0][3]
    assert all(p[3] == radius for p in problems), "one call has one radius"
    src, s0 = pack([p[0] for p in problems])
    tgt, t0 = pack([p[1] for p in problems])
    ns, ms, k = [len(p[0]) for p in problems], [len(p[1]) for p in problems], len(problems)
    return (dev(src), dev(tgt), i32(s0), i32(ns), i32(t0), i32(ms), dev(np.ones(k, np.float32)), dev(np.zeros((k, 3), np.float32)),
            dev(np.stack([p[2] for p in problems]).astype(np.float32)), max(ns), max(ms), radius, max_iter, rel, rel)


def gpu_icp(problems, max_iter, rel=1e-6, pieces=None, search="grid"):
    """The problems as ONE call of ops.icp_p2p (pieces: through ops.IcpRun, that many launches at a time).  Returns numpy
    (T [n,4,4] fp32, fitness [n] fp32, rmse [n] fp32, iters [n])."""
    args, k = icp_args(problems, max_iter, rel), len(problems)
    if pieces is None:
        T, fr, iters = ops.icp_p2p(*args, search=search)
    else:
        run = ops.IcpRun(*args, search=search)
        while run.launches_left > 0:
            run.advance(pieces)
        T, fr, iters = run.T, run.fr, run.iters
    torch.cuda.synchronize()
    fr = fr.cpu().numpy()
    return T.cpu().numpy().reshape(k, 4, 4), fr[:, 0].copy(), fr[:, 1].copy(), iters.cpu().numpy()


@functools.lru_cache(maxsize=None)
def grid_refs(frame, n, updates):
    """(problem, icp_f64, icp_f32_storage) of a grid problem over `updates` updates with the thresholds at 0; computed once."""
    prob = IR.lattice_problem(frame, IR.frame_h(frame), n, IR.n_far_for(n))
    return prob, IR.icp_f64(*prob, updates, 0.0, 0.0), IR.icp_f32_storage(*prob, updates, 0.0, 0.0)


def assert_valid(f64, yard):
    assert IR.margins_hold(f64, yard), "the margin condition fails: the comparison would not be valid"
    assert IR.same_correspondences(f64, yard)


def assert_rule(what, got, f64, yard):
    print(IR.rule_report(what, got, f64, yard))
    assert IR.rule_ok(got, f64, yard), IR.rule_report(what, got, f64, yard)


def assert_evaluation(what, fit, rmse, ev64, ev32, n):
    """Fitness exact, RMSE within the rule, against evaluation records of the two references."""
    assert fit == np.float32(ev64["cnt"] / n if n else 0.0), (what, fit, ev64["cnt"], n)
    assert_rule(what + " rmse", rmse, ev64["rmse"], ev32["rmse"])


def apply(T, x):
    T = np.asarray(T, np.float64)
    return np.asarray(x, np.float64) @ T[:3, :3].T + T[:3, 3]


def assert_undetermined_pose(what, T, prob, f64, yard):
    """One or two correspondences do not determine the pose: T is finite and a proper rotation to 8 fp32 spacings, and every
    matched source row lands where the float64 loop puts it, within the rule."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1]), (what, T)
    tol = 8 * float(np.spacing(np.float32(1.0)))
    assert np.abs(R.T @ R - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1.0) <= tol, (what, R)
    rows = prob[0][f64["trace"][0]["mask"]]
    assert_rule(what + " matched rows", apply(T, rows), apply(f64["T"], rows), apply(yard["T"], rows))


# ------------------------------------------------------------------------------------------------ evaluation, one update
GRID = [(f, n) for f in IR.FRAMES for n in IR.LENGTHS]


@pytest.mark.parametrize("frame,n", GRID)
def test_icp_evaluation_only(frame, n):
    """max_iter = 0: the chunk partials and their sum in 15 strided groups alone.  Lengths: one chunk, 15 and 16 chunks (the first
    wrap into group 0 at 3 841), three chunks in group 0 (7 681); three rows without a partner."""
    prob, f64, yard = grid_refs(frame, n, 1)
    assert_valid(f64, yard)
    T, fit, rmse, iters = gpu_icp([prob], 0)
    assert_evaluation("eval %d/%d" % (frame, n), fit[0], rmse[0], f64["trace"][0], yard["trace"][0], n)
    np.testing.assert_array_equal(T[0], prob[2])
    assert iters[0] == 0


@pytest.mark.parametrize("frame,n", GRID)
def test_icp_one_update(frame, n):
    """max_iter = 1, thresholds 0: T against the float64 Kabsch of the known correspondences composed onto T0."""
    prob, f64, yard = grid_refs(frame, n, 1)
    assert_valid(f64, yard)
    src, tgt, T0, radius = prob
    T, fit, rmse, iters = gpu_icp([prob], 1, rel=0.0)
    assert iters[0] == 1
    ev = yard["trace"][0]
    what = "update %d/%d" % (frame, n)
    if ev["cnt"] >= 3:
        T64 = PR.kabsch_f64(ev["a"][ev["mask"]], tgt[ev["idx"][ev["mask"]]])["T"] @ T0.astype(np.float64)
        assert_rule(what + " T", T[0], T64, yard["T"])
    else:
        assert_undetermined_pose(what, T[0], prob, f64, yard)
    assert_evaluation(what, fit[0], rmse[0], f64["trace"][1], yard["trace"][1], n)


@pytest.mark.parametrize("frame,n", [(f, n) for f in IR.FRAMES for n in TRAJECTORY_LENGTHS])
def test_icp_trajectories_of_two_to_six_updates(frame, n):
    """Thresholds 0, so exactly k updates: both parities of the T, state and partial buffers, and the composition k times."""
    prob, f64, yard = grid_refs(frame, n, TRAJECTORY_UPDATES)
    assert_valid(f64, yard)
    for k in range(2, TRAJECTORY_UPDATES + 1):
        T, fit, rmse, iters = gpu_icp([prob], k, rel=0.0)
        assert iters[0] == k
        what = "trajectory %d/%d k=%d" % (frame, n, k)
        assert_rule(what + " T", T[0], f64["trace"][k]["T"], yard["trace"][k]["T"])
        assert_evaluation(what, fit[0], rmse[0], f64["trace"][k], yard["trace"][k], n)


# ------------------------------------------------------------------------------------------------------- the stop rules
@pytest.mark.parametrize("name", [nm for nm, _ in IR.stop_rule_problems()])
def test_icp_default_stop_rule_stops_where_float64_stops(name):
    prob = dict(IR.stop_rule_problems())[name]
    f64, yard = IR.icp_f64(*prob, 30), IR.icp_f32_storage(*prob, 30)
    assert_valid(f64, yard)
    assert IR.stop_rule_is_decided(f64) and f64["iters"] == yard["iters"] < 30
    T, fit, rmse, iters = gpu_icp([prob], 30)
    assert iters[0] == f64["iters"], (iters, f64["iters"])
    assert_rule("stop %s T" % name, T[0], f64["T"], yard["T"])
    assert_evaluation("stop " + name, fit[0], rmse[0], f64["trace"][-1], yard["trace"][-1], len(prob[0]))


def test_icp_cap_and_schedule_in_pieces_of_one():
    """Thresholds 0 and max_iter = 3 give exactly 3 updates; the default schedule launched one piece at a time through IcpRun
    gives the bits of the one call."""
    probs = [pb for nm, pb in IR.stop_rule_problems() if nm in ("ordinary/0", "slow/0")]
    for pb in probs:
        assert_valid(IR.icp_f64(*pb, 30), IR.icp_f32_storage(*pb, 30))
    assert list(gpu_icp(probs, 3, rel=0.0)[3]) == [3, 3]
    whole, pieces = gpu_icp(probs, 30), gpu_icp(probs, 30, pieces=1)
    for a, b in zip(whole, pieces):
        np.testing.assert_array_equal(a, b)
    assert list(whole[3]) == [IR.icp_f64(*pb, 30)["iters"] for pb in probs]


# --------------------------------------------------------------------------------------------------- coincident clouds
@pytest.mark.parametrize("frame", IR.COINCIDENT_FRAMES)
def test_icp_coincident_clouds(frame):
    """The target's own rows as the source: the residual is 0, whatever the frame.  (The search's expanded fp32 value is a rounding
    residue of either sign there; summed as the squared residual it gave a nonzero or NaN RMSE and a run to the cap.)"""
    prob = IR.coincident_problem(frame)
    f64, yard = IR.icp_f64(*prob, 1000), IR.icp_f32_storage(*prob, 1000)
    assert_valid(f64, yard)
    T, fit, rmse, iters = gpu_icp([prob], 0)
    assert fit[0] == 1.0 and rmse[0] == 0.0, (fit, rmse)
    np.testing.assert_array_equal(T[0], np.eye(4, dtype=np.float32))
    T, fit, rmse, iters = gpu_icp([prob], 1000)
    assert np.isfinite(rmse[0]) and fit[0] == 1.0, (fit, rmse)
    assert_rule("coincident %d rmse" % frame, rmse[0], f64["rmse"], yard["rmse"])
    assert iters[0] == f64["iters"] and f64["iters"] <= 2, (iters, f64["iters"])


# ------------------------------------------------------------------------------------------------------ degenerate sets
@functools.lru_cache(maxsize=None)
def neighbours_alone(max_iter, rel):
    return [gpu_icp([pb], max_iter, rel) for pb in IR.degenerate_neighbours()]


def assert_neighbours_untouched(got, max_iter, rel):
    for slot, alone in zip((0, 2), neighbours_alone(max_iter, rel)):
        for a, b in zip(got, alone):
            np.testing.assert_array_equal(a[slot], b[0])


@pytest.mark.parametrize("name", [nm for nm, _, _ in IR.degenerate_problems()])
def test_icp_degenerate_pair_between_two_ordinary_pairs(name):
    prob, k = {nm: (pb, k) for nm, pb, k in IR.degenerate_problems()}[name]
    first, last = IR.degenerate_neighbours()
    n = len(prob[0])
    f64, yard = IR.icp_f64(*prob, 1, 0.0, 0.0), IR.icp_f32_storage(*prob, 1, 0.0, 0.0)
    assert_valid(f64, yard)
    assert f64["trace"][0]["cnt"] == k
    for max_iter, rel in ((1, 0.0), (2, 0.0), (5, 1e-6)):
        got = gpu_icp([first, prob, last], max_iter, rel)
        assert_neighbours_untouched(got, max_iter, rel)
        T, fit, rmse, iters = (v[1] for v in got)
        assert np.isfinite(T).all() and np.isfinite(fit) and np.isfinite(rmse)
        assert fit == np.float32(k / n if n else 0.0)
        if k == 0:
            # nothing found: identity updates until the stop rule or the cap ends the run (open3d's loop; include/scream_hip.h)
            np.testing.assert_array_equal(T, prob[2])
            assert rmse == 0.0 and iters == (1 if rel > 0 else max_iter), (rmse, iters)
        elif max_iter == 1:
            assert iters == 1
            assert_undetermined_pose("degenerate " + name, T, prob, f64, yard)


# ------------------------------------------------------------------------------------- batch independence and freeze
def test_icp_pairs_of_one_batch_equal_their_own_calls():
    """Five pairs of different lengths and frames that stop after 2, 3, 1, 1 and 2 updates in one call: every output is bitwise that
    of the pair's own call (a stopped pair freezes while the others go on), on the grid path and on the brute-force path, which
    agree bit for bit."""
    probs = [pb for _, pb in IR.batch_problems()]
    for pb, want in zip(probs, IR.BATCH_ITERS):
        f64, yard = IR.icp_f64(*pb, 30), IR.icp_f32_storage(*pb, 30)
        assert_valid(f64, yard)
        assert f64["iters"] == yard["iters"] == want and IR.stop_rule_is_decided(f64)
    together = gpu_icp(probs, 30)
    assert tuple(together[3]) == IR.BATCH_ITERS
    for p, pb in enumerate(probs):
        for a, b in zip(together, gpu_icp([pb], 30)):
            np.testing.assert_array_equal(a[p], b[0])
    brute = gpu_icp(probs, 30, search="brute")
    for a, b in zip(together, brute):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------- the workspace and its size
WS_MARGIN = 264  # bytes of the big tensor on either side of the workspace; not a multiple of 256, so the slice starts unaligned


def _range_call(search, args, ws, ws_bytes, outputs=None):
    """One whole run through the C function itself with the caller's workspace pointer and size.  Returns (T, fr, iters)."""
    from scream_amd import _lib
    lib = _lib.load()
    fn = {"grid": lib.scream_icp_p2p_range, "brute": lib.scream_icp_p2p_brute_range}[search]
    src, tgt, s0, ns, t0, ms, s, c, T0, max_n, max_m, radius, max_iter, rel_f, rel_r = args
    k = s.shape[0]
    if outputs is None:
        outputs = (T0.clone(), torch.empty(k, 2, device=DEV), torch.empty(k, dtype=torch.int32, device=DEV))
    T, fr, iters = outputs
    ptr = lambda t: t.data_ptr()
    _lib.check(fn(ptr(src), ptr(tgt), ptr(s0), ptr(ns), ptr(t0), ptr(ms), ptr(s), ptr(c), k, max_n, max_m, src.shape[0], tgt.shape[0],
                  float(radius), int(max_iter), float(rel_f), float(rel_r), ptr(T), ptr(fr), ptr(iters), 0, int(max_iter) + 2, None,
                  ws, ws_bytes, torch.cuda.current_stream().cuda_stream), "scream_icp_p2p_%srange" % ("brute_" if search == "brute" else ""))
    return T, fr, iters


@pytest.mark.parametrize("search", ["grid", "brute"])
def test_icp_run_stays_inside_exactly_the_workspace_it_asks_for(search):
    """A run given exactly scream_icp_workspace_bytes bytes, unaligned, in the middle of a larger tensor: the bytes around it keep
    their pattern, what the workspace held before (zeros, 0xFF) changes no output bit, the outputs are those of ops.icp_p2p, and
    one byte less is refused before anything is enqueued.  Three pairs with source lengths on both sides of a 256-row chunk
    (257, 40, 300) in one call, and a call whose only source is empty; max_iter = 5."""
    from scream_amd import _lib
    first, last = IR.degenerate_neighbours()
    degenerate = {nm: pb for nm, pb, _ in IR.degenerate_problems()}
    for problems in ([first, degenerate["one_corr"], last], [degenerate["empty"]]):
        args = icp_args(problems, 5, 1e-6)
        need = _lib.load().scream_icp_workspace_bytes(args[0].shape[0], args[1].shape[0], len(problems))
        assert need > 0
        want = ops.icp_p2p(*args, search=search)
        runs = []
        for fill in (0x00, 0xFF):
            big = torch.full((WS_MARGIN + need + WS_MARGIN,), fill, dtype=torch.uint8, device=DEV)
            runs.append(_range_call(search, args, big.data_ptr() + WS_MARGIN, need))
            torch.cuda.synchronize()
            assert bool((big[:WS_MARGIN] == fill).all()) and bool((big[WS_MARGIN + need:] == fill).all()), (search, fill)
        for got in runs:
            for a, b in zip(got, want):
                assert torch.equal(a, b), (search, a, b)
        # one byte short: SCREAM_EINVAL, and nothing was enqueued -- the outputs keep what they held
        outputs = (args[8].clone(), torch.full((len(problems), 2), -7.0, device=DEV), torch.full((len(problems),), -7, dtype=torch.int32, device=DEV))
        before = [o.clone() for o in outputs]
        big = torch.zeros(WS_MARGIN + need + WS_MARGIN, dtype=torch.uint8, device=DEV)
        with pytest.raises(_lib.ScreamHipError, match="SCREAM_EINVAL"):
            _range_call(search, args, big.data_ptr() + WS_MARGIN, need - 1, outputs)
        torch.cuda.synchronize()
        for a, b in zip(outputs, before):
            assert torch.equal(a, b)
        assert not bool(big.any())
