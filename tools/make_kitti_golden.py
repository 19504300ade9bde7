"""Record tests/golden/kitti_predator.npz: what the reference's datasets/kitti.py (KITTI_PREDATOR) selects and passes on for a
small synthetic odometry set, so that tests/test_kitti_raw_host.py can hold scream_amd/kitti_raw.py without the reference.

    python tools/make_kitti_golden.py --reference /path/to/SCREAM --out tests/golden/kitti_predator.npz

The reference module is loaded from its file with stand-ins for what is not installed: ``open3d`` (registration_icp records its
arguments and returns the identity, voxel_down_sample returns its input), the reference's ``utils.to_o3d_pcd`` and its ``lie``
package (imported, never called here).  One numpy difference is bridged: the selection loop asks ``next_time in inames`` with an
EMPTY array wherever no frame lies further than 10 m (every stop, and the end of every drive); numpy answered False there when the
reference was written and raises since 2.2, so the module sees a ``where`` whose empty result compares unequal to everything.
Only the recorded arrays are written: the synthetic poses (drives 0-7), the ``files`` lists of train and val, M for six pairs
(with reg = I the cache file holds M2 = M exactly), the fp32 rot / trans of those items and the recorded ICP arguments.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

DRIVES = range(8)
M_ITEMS = (("train", 0), ("train", 1), ("train", 7), ("val", 0), ("val", 2), ("val", 3))


def synthetic_poses(drive):
    """[n,12] odometry rows of one drive: straight runs at 0.6-1.4 m per frame, slow stretches, one stop longer than 100 frames
    and a gentle yaw, seeded by the drive number."""
    rng = np.random.default_rng(100 + drive)
    n = 260 + 20 * drive
    speed = np.full(n, 1.0)
    k = 0
    while k < n:
        run = int(rng.integers(30, 80))
        speed[k:k + run] = rng.uniform(0.6, 1.4)
        k += run
        if rng.uniform() < 0.5:
            slow = int(rng.integers(10, 40))
            speed[k:k + slow] = rng.uniform(0.02, 0.2)
            k += slow
    stop0 = int(rng.integers(60, 100))
    speed[stop0:stop0 + 115] = 0.0
    yaw = np.cumsum(rng.normal(scale=0.004, size=n))
    rows, p = [], np.zeros(3)
    for i in range(n):
        c, s = np.cos(yaw[i]), np.sin(yaw[i])
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        p = p + R @ np.array([0.0, 0.0, speed[i]])
        rows.append(np.hstack([R, p[:, None]]).reshape(-1))
    return np.array(rows)


def write_root(root, poses):
    """The directory layout the data set reads, with an eight-point scan per frame."""
    os.makedirs(os.path.join(root, "dataset", "poses"))
    for d, rows in poses.items():
        np.savetxt(os.path.join(root, "dataset", "poses", "%02d.txt" % d), rows, fmt="%.18e")
        vdir = os.path.join(root, "dataset", "sequences", "%02d" % d, "velodyne")
        os.makedirs(vdir)
        rng = np.random.default_rng(d)
        for t in range(len(rows)):
            rng.uniform(-20, 20, size=(8, 4)).astype(np.float32).tofile(os.path.join(vdir, "%06d.bin" % t))


class _Cloud:
    def __init__(self, pts):
        self.points = np.asarray(pts)

    def transform(self, T):
        return self


class _EmptyUnequal(np.ndarray):
    def __eq__(self, other):
        return False if self.size == 0 else np.ndarray.__eq__(self, other)

    __hash__ = None


class _Numpy:
    """numpy, except that where()'s index arrays compare as the numpy of the reference's day did when empty."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def where(*a, **k):
        return tuple(np.asarray(x).view(_EmptyUnequal) for x in np.where(*a, **k))


def load_reference(path, record):
    o3d = types.ModuleType("open3d")
    reg = types.SimpleNamespace()

    def registration_icp(src, tgt, radius, init, estimation, criteria):
        record.append(dict(radius=float(radius), init=np.asarray(init).copy(), max_iteration=int(criteria.max_iteration),
                           estimation=type(estimation).__name__))
        return types.SimpleNamespace(transformation=np.eye(4))

    class TransformationEstimationPointToPoint:
        pass

    reg.registration_icp = registration_icp
    reg.TransformationEstimationPointToPoint = TransformationEstimationPointToPoint
    reg.ICPConvergenceCriteria = lambda max_iteration=30: types.SimpleNamespace(max_iteration=max_iteration)
    o3d.registration = reg
    o3d.voxel_down_sample = lambda pcd, voxel: pcd
    utils = types.ModuleType("utils")
    utils.to_o3d_pcd = lambda xyz, *a: _Cloud(xyz)
    lie, lie_np, se3, lie_utils = (types.ModuleType(n) for n in ("lie", "lie.numpy", "lie.numpy.se3", "lie.numpy.utils"))
    se3.SE3 = object
    for n in ("se3_init", "se3_inv", "se3_cat", "se3_transform"):
        setattr(lie_utils, n, None)
    saved = {k: sys.modules.get(k) for k in ("open3d", "utils", "lie", "lie.numpy", "lie.numpy.se3", "lie.numpy.utils")}
    sys.modules.update({"open3d": o3d, "utils": utils, "lie": lie, "lie.numpy": lie_np, "lie.numpy.se3": se3, "lie.numpy.utils": lie_utils})
    try:
        spec = importlib.util.spec_from_file_location("reference_kitti", os.path.join(path, "datasets", "kitti.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.np = _Numpy()
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "kitti_predator.npz"))
    a = ap.parse_args()
    poses = {d: synthetic_poses(d) for d in DRIVES}
    record = []
    mod = load_reference(a.reference, record)
    out = {"poses_%d" % d: rows for d, rows in poses.items()}
    with tempfile.TemporaryDirectory() as root:
        write_root(root, poses)
        sets = {m: mod.KITTI_PREDATOR(root, mode=m, data_augmentation=False) for m in ("train", "val")}
        for m, ds in sets.items():
            out["files_" + m] = np.array(ds.files, dtype=np.int64).reshape(-1, 3)
        Ms, rots, transs = [], [], []
        for m, i in M_ITEMS:
            item = sets[m][i]
            Ms.append(np.load(sets[m].icp_path + "/%d_%d_%d.npy" % tuple(sets[m].files[i])))
            rots.append(item[4])
            transs.append(item[5])
    assert len(record) == len(M_ITEMS) and all(np.array_equal(r["init"], np.eye(4)) for r in record)
    out.update(M=np.array(Ms), rot=np.array(rots), trans=np.array(transs), M_mode=np.array([m for m, _ in M_ITEMS]),
               M_item=np.array([i for _, i in M_ITEMS]), icp_radius=np.array(record[0]["radius"]),
               icp_max_iteration=np.array(record[0]["max_iteration"]), icp_estimation=np.array(record[0]["estimation"]))
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d train pairs, %d val pairs, %d bytes" % (a.out, len(out["files_train"]), len(out["files_val"]), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
