"""scream_amd/kitti_raw.py (KITTI_PREDATOR) and process_kitti.py on the CPU against tests/golden/kitti_predator.npz, which
tools/make_kitti_golden.py recorded from the reference's datasets/kitti.py on synthetic odometry (drives 0-7, with stops longer
than 100 frames, so both branches of the selection loop run).  The GPU calls are replaced by CPU stand-ins: this file holds the
host layer (selection, M, cache files, what save_pair writes), tests/test_gpu_rawicp.py the composition with the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import process_kitti  # noqa: E402
from scream_amd import kitti_raw  # noqa: E402
from scream_amd.evaluate_kitti import KittiPairFiles  # noqa: E402

ICP_SHIFT = np.array([0.03125, -0.0625, 0.015625])  # the stand-in's "refinement": exact in float64 and fp32


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("kitti_predator")


def write_root(root, fx, drives, points=40):
    """The layout KITTI_PREDATOR reads: the fixture's poses and a small seeded scan per frame."""
    os.makedirs(os.path.join(root, "dataset", "poses"))
    for d in drives:
        rows = fx["poses_%d" % d]
        np.savetxt(os.path.join(root, "dataset", "poses", "%02d.txt" % d), rows, fmt="%.18e")
        vdir = os.path.join(root, "dataset", "sequences", "%02d" % d, "velodyne")
        os.makedirs(vdir)
        rng = np.random.default_rng(d)
        for t in range(len(rows)):
            rng.uniform(-20, 20, size=(points, 4)).astype(np.float32).tofile(os.path.join(vdir, "%06d.bin" % t))


@pytest.fixture(scope="module")
def root(tmp_path_factory, fixture):
    r = str(tmp_path_factory.mktemp("kitti"))
    write_root(r, fixture, range(8))
    return r


@pytest.fixture
def cpu_stubs(monkeypatch):
    """icp_raw_batch: T = shift . T_init, recorded; voxel_down_sample_batch: the cloud's rows rounded to the voxel, unique."""
    calls = []

    def icp(srcs, tgts, T_inits, max_corr_dist=0.2, max_iter=50000, *a, **k):
        T0 = np.asarray(T_inits, dtype=np.float64)
        calls.append(dict(n=len(srcs), radius=max_corr_dist, max_iter=max_iter, dtypes={s.dtype for s in srcs}, T0=T0.copy()))
        D = np.eye(4)
        D[:3, 3] = ICP_SHIFT
        T = np.stack([D @ t for t in T0])
        return torch.from_numpy(T), torch.zeros(len(srcs), 2, dtype=torch.float64), torch.ones(len(srcs), dtype=torch.int32)

    def down(clouds, voxel_size, return_counts=False):
        out = []
        for c in clouds:
            a = c.cpu().numpy()
            assert a.dtype == np.float32
            out.append(torch.from_numpy(np.unique((np.floor(a / voxel_size) * voxel_size).astype(np.float32), axis=0)))
        return out

    monkeypatch.setattr(kitti_raw.rawicp, "icp_raw_batch", icp)
    monkeypatch.setattr(kitti_raw.voxel, "voxel_down_sample_batch", down)
    monkeypatch.setattr(process_kitti.voxel, "voxel_down_sample_batch", down)
    return calls


def dataset(root, mode):
    return kitti_raw.KITTI_PREDATOR(root, mode, device="cpu")


@pytest.mark.parametrize("mode", ["train", "val"])
def test_files_are_the_reference_lists(root, fixture, mode):
    ds = dataset(root, mode)
    want = [tuple(int(v) for v in row) for row in fixture["files_" + mode]]
    assert ds.files == want and len(ds) == len(want) > 30
    # both branches ran: somewhere the walk stepped over frames (a pair starts later than the previous one ended + 1)
    gaps = [b[1] - a[2] for a, b in zip(ds.files, ds.files[1:]) if a[0] == b[0]]
    assert max(gaps) > 50 and min(gaps) == 1


def test_initial_pose_is_the_reference_M(root, fixture):
    """Equal to the last float64 bit: the same numpy expression on the same arrays."""
    sets = {m: dataset(root, m) for m in ("train", "val")}
    for M, mode, item in zip(fixture["M"], fixture["M_mode"], fixture["M_item"]):
        got = sets[str(mode)].initial_pose(int(item))
        assert got.dtype == np.float64 and np.array_equal(got, M), (mode, item, np.abs(got - M).max())
    assert float(fixture["icp_radius"]) == sets["train"].icp_radius == 0.2
    assert int(fixture["icp_max_iteration"]) == sets["train"].icp_max_iter == 50000


def test_velo2cam_property_holds_the_transpose(root):
    v = dataset(root, "val").velo2cam
    assert np.array_equal(v[3, :3], [-4.069766e-03, -7.631618e-02, -2.717806e-01]) and np.array_equal(v[:, 3], [0, 0, 0, 1])


def test_cache_file_name_and_round_trip(tmp_path, fixture, cpu_stubs):
    r = str(tmp_path)
    write_root(r, fixture, (6, 7))
    ds = dataset(r, "val")
    assert ds.refine_poses(indices=range(11), batch_pairs=4) == 11
    assert [c["n"] for c in cpu_stubs] == [4, 4, 3] and all(c["radius"] == 0.2 and c["max_iter"] == 50000 for c in cpu_stubs)
    assert all(c["dtypes"] == {np.dtype(np.float32)} for c in cpu_stubs)
    drive, t0, t1 = ds.files[5]
    name = os.path.join(r, "icp", "%d_%d_%d.npy" % (drive, t0, t1))
    assert os.path.exists(name) and ds.icp_file(5) == r + "/icp/%d_%d_%d.npy" % (drive, t0, t1)
    M = ds.initial_pose(5)
    assert np.array_equal(cpu_stubs[1]["T0"][1], M)  # the raw source is refined from T_init = M
    D = np.eye(4)
    D[:3, 3] = ICP_SHIFT
    want = M @ ((D @ M) @ np.linalg.inv(M))  # M2 = M @ reg, reg = T @ inv(M)
    assert np.array_equal(np.load(name), want)
    # a second data set reads the files back and computes nothing
    n_calls = len(cpu_stubs)
    ds2 = dataset(r, "val")
    assert ds2.refine_poses(indices=range(11)) == 0 and len(cpu_stubs) == n_calls
    item = ds2[5]
    assert np.array_equal(item[4], want[:3, :3].astype(np.float32)) and np.array_equal(item[5], want[:3, 3:].astype(np.float32))
    assert item[4].dtype == np.float32 and item[5].shape == (3, 1) and item[0].dtype == np.float64 and item[2].shape == (len(item[0]), 1)
    # an item without a file is refined on demand, alone
    ds2[12]
    assert len(cpu_stubs) == n_calls + 1 and cpu_stubs[-1]["n"] == 1


def test_augmentation_branch_draws_like_the_reference(tmp_path, fixture, cpu_stubs):
    r = str(tmp_path)
    write_root(r, fixture, (6, 7))
    plain = kitti_raw.KITTI_PREDATOR(r, "val", device="cpu")[0]
    aug = kitti_raw.KITTI_PREDATOR(r, "val", data_augmentation=True, device="cpu")
    np.random.seed(3)
    import random
    random.seed(3)
    a = aug[0]
    assert a[0].shape == plain[0].shape and a[1].shape == plain[1].shape and np.array_equal(a[4], plain[4])
    scale = np.linalg.norm(a[0] - a[0].mean(axis=0), axis=1).max() / np.linalg.norm(plain[0] - plain[0].mean(axis=0), axis=1).max()
    assert 0.79 < scale < 1.21 and not np.allclose(a[0], plain[0])


def test_save_pair_writes_fp32_poses_and_skips_item_one_of_test(tmp_path, fixture, cpu_stubs):
    r, out = str(tmp_path / "root"), str(tmp_path / "out")
    os.makedirs(r)
    write_root(r, fixture, (6, 7))
    ds = dataset(r, "val")
    ds.files = ds.files[:5]
    assert process_kitti.save_pair("val", out=out, dataset=ds, pairs_per_call=2) == 5
    files = KittiPairFiles(os.path.join(out, "KITTI_val"))
    assert len(files) == 5
    for k in range(5):
        T = np.load(os.path.join(out, "KITTI_val", "T%d.npy" % k))
        M2 = ds.refined_pose(k)
        assert T.dtype == np.float64 and np.array_equal(T, T.astype(np.float32).astype(np.float64))  # fp32 values
        assert np.array_equal(T[:3], M2[:3].astype(np.float32).astype(np.float64)) and np.array_equal(T[3], [0, 0, 0, 1])
        src = np.load(os.path.join(out, "KITTI_val", "src%d.npy" % k))
        assert src.dtype == np.float64 and np.array_equal(src, src.astype(np.float32).astype(np.float64))
        assert len(files[k]) == 6
    # mode "test": item 1 is skipped and the files stay numbered without a gap
    ds.split = "test"
    assert process_kitti.save_pair("test", out=out, dataset=ds, pairs_per_call=16) == 4
    for k, item in enumerate((0, 2, 3, 4)):
        T = np.load(os.path.join(out, "KITTI_test", "T%d.npy" % k))
        assert np.array_equal(T[:3], ds.refined_pose(item)[:3].astype(np.float32).astype(np.float64))
    assert not os.path.exists(os.path.join(out, "KITTI_test", "T4.npy"))
    assert process_kitti.check_saved_pairs("test", out) == 4
