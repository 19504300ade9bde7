"""The raw-scan ICP on the MI355X (csrc/icp_raw.hip, scream_amd/rawicp.py) against tests/rawicp_ref.py.
The search is held bit for bit (idx and d2 array_equal to the float64 brute force); fitness, iters and the correspondences of
whole loops are exact comparisons (tests/test_rawicp_ref_host.py proves the margins that determine them); inlier_rmse of an
evaluation is bit for bit the kernel-order restatement; T is held to the bars of rawicp_ref (C_R64 / C_T64 against the LAPACK
loop).  Run with `pytest -m gpu`."""
import functools

import numpy as np
import pytest
import torch

import icp_step_ref as ISR
import rawicp_ref as RR
from scream_amd import ScreamHipError, _lib
from scream_amd.rawicp import RawIcpRun, icp_raw_batch, raw_nn_batch

pytestmark = pytest.mark.gpu
MAX_ITER = 60


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def gpu_nn(srcs, tgts, Ts, radius, **kw):
    out = raw_nn_batch(srcs, tgts, np.stack(Ts), radius, **kw)
    return ([i.cpu().numpy() for i in out[0]], [d.cpu().numpy() for d in out[1]]) + tuple(out[2:])


def gpu_icp(pbs, max_iter, rel=1e-6, **kw):
    """[(src, tgt, T0, radius)] sharing one radius -> numpy (T, fitness_rmse, iters[, status])."""
    out = icp_raw_batch([p[0] for p in pbs], [p[1] for p in pbs], np.stack([p[2] for p in pbs]), pbs[0][3], max_iter, rel, rel, **kw)
    return tuple(o.cpu().numpy() for o in out)


def check_search(src, tgt, T, radius, what):
    want = RR.search(RR.transform(T, src), tgt, radius)
    idx, d2 = gpu_nn([src], [tgt], [T], radius)
    assert np.array_equal(idx[0], want["idx"]), what
    assert np.array_equal(d2[0], want["d2"]), what
    return want


@functools.lru_cache(maxsize=None)
def refs():
    """{name: (problem, one-update lapack, loop ref, loop lapack)} of the well-posed problems, computed once for the module."""
    return {name: (pb, RR.icp_raw_lapack(*pb, 1, 0.0, 0.0), RR.icp_raw_ref(*pb, MAX_ITER), RR.icp_raw_lapack(*pb, MAX_ITER))
            for name, pb in RR.well_posed_problems()}


# ------------------------------------------------------------------------------------------------------------ 1. search
@pytest.mark.parametrize("frame", [0.0, 1000.0])
@pytest.mark.parametrize("radius", [0.2, 0.45])
def test_search_ring_pair_bit_for_bit(frame, radius):
    src, tgt, T0, Tt, _ = RR.ring_pair(frame=frame)
    for name, T in (("start", T0), ("true", Tt)):
        want = check_search(src, tgt, T, radius, "%s frame %g radius %g" % (name, frame, radius))
    assert want["mask"].sum() > 0.9 * len(src)  # under the true pose the search finds what it should


@pytest.mark.parametrize("shift", RR.SHIFTS)
def test_search_exactly_at_the_radius(shift):
    src, tgt, T, radius = RR.radius_lattice(shift)
    for r, n_hit in ((radius, 375), (np.nextafter(radius, 0), 375), (np.nextafter(radius, 1), 375 + 750)):
        want = check_search(src, tgt, T, float(r), "shift %g radius %r" % (shift, r))
        assert want["mask"].sum() == n_hit


def test_search_ties_go_to_the_lowest_row():
    src, tgt, T, radius = RR.tie_pair()
    want = check_search(src, tgt, T, radius, "ties")
    assert want["mask"].sum() > 900


def test_search_lengths_batch_and_one_point_target():
    src, tgt, T0, Tt, radius = RR.ring_pair()
    lens = (1, 255, 256, 257, 0)
    srcs = [src[100 * k:100 * k + n] for k, n in enumerate(lens)] + [src]
    tgts = [tgt, tgt[:3000], tgt, tgt[500:], tgt, tgt[:1]]
    Ts = [Tt, T0, Tt, T0, Tt, Tt]
    bi, bd = gpu_nn(srcs, tgts, Ts, radius)
    for k in range(len(srcs)):
        want = RR.search(RR.transform(Ts[k], srcs[k]), tgts[k], radius)
        assert bi[k].shape == (len(srcs[k]),)
        assert np.array_equal(bi[k], want["idx"]) and np.array_equal(bd[k], want["d2"]), k
        ai, ad = gpu_nn([srcs[k]], [tgts[k]], [Ts[k]], radius)  # the same pair alone
        assert np.array_equal(ai[0], bi[k]) and np.array_equal(ad[0], bd[k]), k
    # the one-point target at its own place: exactly one row can match
    one = np.concatenate([tgt[:1] + np.float32(0.05), src[:50]])
    want = check_search(one, tgt[:1], np.eye(4), radius, "one-point target")
    assert want["idx"][0] == 0 and want["mask"].sum() >= 1


# ----------------------------------------------------------------------------------------------------- 2. evaluation only
def test_evaluation_only_is_the_restatement_bit_for_bit():
    pbs = [pb for _, pb in RR.well_posed_problems()]
    for pb in pbs:
        T, fr, iters = gpu_icp([pb], 0)
        ev = RR.icp_raw_ref(*pb, 0)["trace"][0]
        assert iters[0] == 0 and np.array_equal(T[0], pb[2])
        assert fr[0, 0] == ev["cnt"] / len(pb[0])
        assert fr[0, 1] == ev["rmse"], (fr[0, 1], ev["rmse"])


@pytest.mark.parametrize("frame", [0, 30, 300, 1000])
def test_coincident_clouds_have_zero_rmse(frame):
    src, tgt, T0, radius = ISR.coincident_problem(frame)
    T, fr, iters = gpu_icp([(src, tgt, RR.f64pose(T0), float(radius))], 0)
    assert fr[0, 0] == 1.0 and fr[0, 1] == 0.0


# ----------------------------------------------------------------------------------------------------------- 3. one update
def test_one_update_is_within_the_bars():
    for name, (pb, l1, rl, ll) in refs().items():
        T, fr, iters = gpu_icp([pb], 1, 0.0)
        assert iters[0] == 1, name
        miss = RR.pose_check(T[0], l1["T"], RR.last_update_stats(l1, pb[0]))
        assert miss is None, "%s: %s" % (name, miss)
        assert fr[0, 0] == l1["fitness"], name


# ---------------------------------------------------------------------------------------------------------- 4. whole loops
@pytest.mark.parametrize("name", [n for n, _ in RR.loop_problems()])
def test_whole_loop(name):
    pb, l1, rl, ll = refs()[name]
    T, fr, iters = gpu_icp([pb], 50000)
    print("%s: iters %d (ref %d) fitness %r rmse %r (ref %r lapack %r) max|T - T_ref| %.3e max|T - T_lapack| %.3e"
          % (name, iters[0], rl["iters"], fr[0, 0], fr[0, 1], rl["rmse"], ll["rmse"], np.abs(T[0] - rl["T"]).max(), np.abs(T[0] - ll["T"]).max()))
    assert iters[0] == rl["iters"] == ll["iters"]
    assert fr[0, 0] == rl["fitness"] == ll["fitness"]
    idx, _ = gpu_nn([pb[0]], [pb[1]], [T[0]], pb[3])
    assert np.array_equal(idx[0], rl["trace"][-1]["idx"]) and np.array_equal(idx[0], ll["trace"][-1]["idx"])
    miss = RR.pose_check(T[0], ll["T"], RR.last_update_stats(ll, pb[0]))
    assert miss is None, "%s: %s" % (name, miss)
    assert RR.rmse_ok(fr[0, 1], rl["rmse"], ll["rmse"]), (fr[0, 1], rl["rmse"], ll["rmse"])


# ---------------------------------------------------------------------------------------------------------- 5. degenerates
@pytest.mark.parametrize("case", range(5))
def test_degenerates(case):
    name, (src, tgt, T0, radius), n_corr = ISR.degenerate_problems()[case]
    pb = (src, tgt, RR.f64pose(T0), float(radius))
    if n_corr == 0:
        for max_iter, rel, want_iters in ((0, 1e-6, 0), (5, 1e-6, 1), (5, 0.0, 5)):
            T, fr, iters = gpu_icp([pb], max_iter, rel)
            assert np.array_equal(T[0].view(np.uint64), pb[2].view(np.uint64)), name
            assert iters[0] == want_iters and fr[0, 0] == 0.0 and fr[0, 1] == 0.0, (name, iters[0])
        return
    T, fr, iters = gpu_icp([pb], 1, 0.0)
    ev = RR.icp_raw_ref(*pb, 0)["trace"][0]
    assert ev["cnt"] == n_corr and fr[0, 0] * len(src) == pytest.approx(n_corr, abs=1e-9)
    R = T[0, :3, :3] @ np.linalg.inv(pb[2][:3, :3])  # the update's rotation (the fp32 start pose is orthogonal to 1e-7 only)
    assert np.isfinite(T[0]).all() and np.array_equal(T[0, 3], [0, 0, 0, 1])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    X = src.astype(np.float64)[ev["mask"]]
    cB = ev["b"][ev["mask"]].mean(axis=0)
    assert np.linalg.norm(T[0, :3, :3] @ X.mean(axis=0) + T[0, :3, 3] - cB) < 1e-9 * (1 + np.linalg.norm(cB))


# ------------------------------------------------------------------------------------------------------------- 6. schedule
def test_schedule_is_independent_of_the_piece():
    pb = dict(RR.well_posed_problems())["lattice/30"]
    got = []
    for piece in (7, 32, 128):
        T, fr, iters = gpu_icp([pb], 70, 0.0, piece=piece)
        assert iters[0] == 70
        got.append((T.copy(), fr.copy()))
    for T, fr in got[1:]:
        assert np.array_equal(T.view(np.uint64), got[0][0].view(np.uint64)) and np.array_equal(fr.view(np.uint64), got[0][1].view(np.uint64))


def test_long_schedule_stops_launching():
    pb = dict(RR.well_posed_problems())["ring/0"]
    run = RawIcpRun([pb[0]], [pb[1]], pb[2][None], pb[3], 50000, 1e-6, 1e-6).run(piece=32)
    iters = int(run.iters.cpu()[0])
    assert 0 < iters < 64
    assert run.iterations == -(-(iters + 1) // 32) * 32
    assert run.iterations_left == 50001 - run.iterations


# --------------------------------------------------------------------------------------------------------------- 7. status
def test_refused_pairs_leave_their_neighbours_alone():
    wp = dict(RR.well_posed_problems())
    a, b = wp["slow/0"], wp["lattice/0"]
    radius = a[3]
    assert radius == b[3]
    wide = np.array([[0, 0, 0], [2.0 ** 21 * radius * 1.5, 0, 0]], np.float32)  # more than 2^21 cells of the radius on x
    nan = a[1].copy()
    nan[7, 1] = np.nan
    T_bad = RR.f64pose(np.eye(4))
    T_bad[0, 3] = 0.125
    pbs = [a, (a[0], wide, T_bad, radius), (b[0], nan, T_bad, radius), b]
    with pytest.raises(ScreamHipError, match="pair 1, 2"):
        gpu_icp(pbs, 30)
    T, fr, iters, status = gpu_icp(pbs, 30, strict=False)
    assert list(status) == [0, -1, -1, 0] and iters[1] == -1 and iters[2] == -1
    assert np.array_equal(T[1], T_bad) and np.array_equal(T[2], T_bad)
    for k, pb in ((0, a), (3, b)):
        T1, fr1, it1 = gpu_icp([pb], 30)
        assert np.array_equal(T[k].view(np.uint64), T1[0].view(np.uint64)) and np.array_equal(fr[k], fr1[0]) and iters[k] == it1[0]
    idx, d2, st = gpu_nn([p[0] for p in pbs], [p[1] for p in pbs], [p[2] for p in pbs], radius, strict=False)
    assert list(st) == [0, -1, -1, 0] and (idx[1] == -1).all() and np.isinf(d2[2]).all()


def test_bad_radius_refuses_every_pair():
    pb = dict(RR.well_posed_problems())["lattice/0"]
    for r in (0.0, -1.0, float("inf"), float("nan")):
        T, fr, iters, status = gpu_icp([(pb[0], pb[1], pb[2], r)], 5, strict=False)
        assert status[0] == -1 and iters[0] == -1 and np.array_equal(T[0], pb[2])


# -------------------------------------------------------------------------------------------------------- 8. repeatability
def test_two_calls_are_bitwise_equal():
    wp = dict(RR.well_posed_problems())
    pbs = [wp["lattice/0"], wp["slow/0"]]
    x, y = gpu_icp(pbs, 50000), gpu_icp(pbs, 50000)
    for u, v in zip(x, y):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------- 9. composition
def _write_kitti_root(root, drives=(0, 1, 2), frames=36, points=1500):
    """Three synthetic drives: a straight run at 1 m per frame; every frame's scan is the drive's world points seen from the
    frame's TRUE pose (2 cm of noise, shuffled), while the pose file is 5 cm off per frame, so the ICP has something to refine."""
    import os
    from scream_amd.kitti_raw import _VELO2CAM_R, _VELO2CAM_T
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = np.array(_VELO2CAM_R).reshape(3, 3), _VELO2CAM_T
    os.makedirs(os.path.join(root, "dataset", "poses"))
    for d in drives:
        rng = np.random.default_rng(40 + d)
        world = np.concatenate([rng.uniform([-30, -2, -15], [30, 3, 50], size=(points, 3)), np.ones((points, 1))], axis=1)
        vdir = os.path.join(root, "dataset", "sequences", "%02d" % d, "velodyne")
        os.makedirs(vdir)
        rows = []
        for t in range(frames):
            P = np.eye(4)
            P[:3, :3] = RR.PR.axis_angle([0, 1, 0], 0.2 * t)
            P[:3, 3] = [0.02 * t, 0.0, 1.0 * t]
            velo = (np.linalg.inv(V) @ np.linalg.inv(P) @ world.T).T[:, :3] + 0.02 * rng.normal(size=(points, 3))
            scan = np.concatenate([velo[rng.permutation(points)], np.zeros((points, 1))], axis=1).astype(np.float32)
            scan.tofile(os.path.join(vdir, "%06d.bin" % t))
            P[:3, 3] += 0.05 * rng.normal(size=3)
            rows.append(P[:3].reshape(-1))
        np.savetxt(os.path.join(root, "dataset", "poses", "%02d.txt" % d), np.array(rows), fmt="%.18e")


def test_refine_poses_and_save_pair_compose(tmp_path):
    import os
    import process_kitti
    from scream_amd.evaluate_kitti import KittiPairFiles
    from scream_amd.kitti_raw import KITTI_PREDATOR

    class ThreeDrives(KITTI_PREDATOR):
        DATA_FILES = {"train": [0, 1, 2], "val": [0, 1, 2], "test": [0, 1, 2]}

    root, out = str(tmp_path / "root"), str(tmp_path / "out")
    os.makedirs(root)
    _write_kitti_root(root)
    ds = ThreeDrives(root, "val")
    assert len(ds) == 9 and ds.refine_poses(batch_pairs=4) == 9
    assert process_kitti.save_pair("val", out=out, dataset=ds) == 9
    files = KittiPairFiles(os.path.join(out, "KITTI_val"))
    assert len(files) == 9 and len(files[8]) == 6
    for i in (0, 4, 8):
        drive, t0, t1 = ds.files[i]
        src, tgt, M = ds._scan(drive, t0), ds._scan(drive, t1), ds.initial_pose(i)
        lap = RR.icp_raw_lapack(src, tgt, M, 0.2, MAX_ITER)
        assert RR.margins_hold(lap) and lap["iters"] < MAX_ITER and lap["fitness"] > 0.9
        T, fr, iters = gpu_icp([(src, tgt, M, 0.2)], 50000)
        assert iters[0] == lap["iters"] and fr[0, 0] == lap["fitness"]
        miss = RR.pose_check(T[0], lap["T"], RR.last_update_stats(lap, src))
        assert miss is None, miss
        M2 = np.load(ds.icp_file(i))
        assert np.array_equal(M2, M @ (T[0] @ np.linalg.inv(M)))  # what the batched call cached is what the pair gives alone
        saved = np.load(os.path.join(out, "KITTI_val", "T%d.npy" % i))
        assert np.array_equal(saved[:3], M2[:3].astype(np.float32).astype(np.float64)) and np.array_equal(saved[3], [0, 0, 0, 1])
        assert np.abs(saved - M @ (lap["T"] @ np.linalg.inv(M))).max() < 1e-5  # fp32 storage of a pose with |t| ~ 10 m
        s = np.load(os.path.join(out, "KITTI_val", "src%d.npy" % i))
        assert s.dtype == np.float64 and 0 < len(s) <= len(src) and np.array_equal(s, s.astype(np.float32).astype(np.float64))
