"""From raw KITTI odometry to the pairs the models see: ``KITTI_PREDATOR`` restates datasets/kitti.py:14-230 without open3d.

    ds = KITTI_PREDATOR("/data/KITTI-Registration", "train")
    ds.refine_poses()                       # fills <root>/icp/<drive>_<t0>_<t1>.npy, eight pairs per GPU call
    src, tgt, src_feats, tgt_feats, rot, trans = ds[0]

Layout, as the reference reads it: ``<root>/dataset/poses/%02d.txt`` (odometry, 12 numbers per frame) and
``<root>/dataset/sequences/%02d/velodyne/%06d.bin`` (fp32 x, y, z, reflectance).  The pair selection, the hard-coded ``velo2cam``
(the property holds the TRANSPOSED matrix, as the reference's does), the start pose
``M = (velo2cam @ pos0.T @ inv(pos1.T) @ inv(velo2cam)).T`` and the cache files holding ``M2 = M @ reg`` are the reference's.

The refinement is scream_amd.rawicp.icp_raw_batch on the unvoxelised scans (float64, radius 0.2 m, 50000 iterations at most,
1e-6 / 1e-6).  The reference transforms the source by M on the host and starts open3d's ICP from the identity; here the raw
source goes to the GPU with ``T_init = M`` and ``reg = T @ inv(M)`` is formed in float64 on the host: the two differ by the
float64 roundings of the transformed points.  Parity with open3d itself (registration_icp, voxel_down_sample) is unpinned
throughout: it is not installed here.  The clouds are voxelised at 0.3 m by voxel_down_sample_batch (float64 sums of the fp32
points, the mean rounded once to fp32, rows in ascending (i, j, k)); __getitem__ returns them as float64 arrays like the
reference's ``np.array(pcd.points)``.
"""
from __future__ import annotations

import glob
import os
import random

import numpy as np
import torch

from . import rawicp, voxel

__all__ = ["KITTI_PREDATOR"]

_VELO2CAM_R = (7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03,
               1.480755e-02)
_VELO2CAM_T = (-4.069766e-03, -7.631618e-02, -2.717806e-01)
BAD_TEST_PAIR = (8, 15, 58)


def select_pairs(positions, frames, drive):
    """The pair-selection loop of prepare_kitti_ply for one drive: from the current frame, the first of the next 100 frames that
    lies more than 10 m away, less one, closes a pair and the walk resumes behind it; a frame with no such partner is stepped
    over.  positions [n,3] (row = frame number), frames the sorted frame numbers that have a scan."""
    pos = np.asarray(positions, dtype=np.float64)
    far = np.sqrt(((pos[None, :, :] - pos[:, None, :]) ** 2).sum(-1)) > 10
    have = set(int(f) for f in frames)
    out, t = [], int(frames[0])
    while t in have:
        hits = np.where(far[t][t:t + 100])[0]
        if len(hits) == 0:
            t += 1
            continue
        nxt = int(hits[0]) + t - 1
        if nxt in have:
            out.append((drive, t, nxt))
            t = nxt + 1
    return out


class KITTI_PREDATOR(torch.utils.data.Dataset):
    DATA_FILES = {"train": [0, 1, 2, 3, 4, 5], "val": [6, 7], "test": [8, 9, 10]}

    def __init__(self, root, mode="train", data_augmentation=False, device="cuda"):
        assert mode in self.DATA_FILES, mode
        self.root = root + "/dataset"
        self.icp_path = root + "/icp"
        os.makedirs(self.icp_path, exist_ok=True)
        self.voxel_size = 0.3
        self.icp_radius = 0.2
        self.icp_max_iter = 50000
        self.data_augmentation = data_augmentation
        self.augment_noise = 0.01
        self.augment_shift_range = 2.0
        self.augment_scale_max = 1.2
        self.augment_scale_min = 0.8
        self.device = device
        self.split = mode
        self.files = []
        self.kitti_icp_cache = {}
        self.kitti_cache = {}
        self.prepare_kitti_ply(mode)

    # ------------------------------------------------------------------------------------------------------- selection
    def prepare_kitti_ply(self, split):
        for drive in self.DATA_FILES[split]:
            names = glob.glob(self.root + "/sequences/%02d/velodyne/*.bin" % drive)
            assert len(names) > 0, "no scans of drive %d under %s" % (drive, self.root)
            frames = sorted(int(os.path.split(n)[-1][:-4]) for n in names)
            odo = self.get_video_odometry(drive, return_all=True)
            pos = np.array([self.odometry_to_positions(o) for o in odo])
            self.files += select_pairs(pos[:, :3, 3], frames, drive)
        if split == "test":
            self.files.remove(BAD_TEST_PAIR)
        print("Num_%s: %d" % (split, len(self.files)))

    def __len__(self):
        return len(self.files)

    # ----------------------------------------------------------------------------------------------------------- files
    @property
    def velo2cam(self):
        """The TRANSPOSE of the 4x4 velodyne-to-camera matrix (the reference keeps it that way and its formula for M relies on it)."""
        if not hasattr(self, "_velo2cam"):
            m = np.hstack([np.array(_VELO2CAM_R).reshape(3, 3), np.array(_VELO2CAM_T).reshape(3, 1)])
            self._velo2cam = np.vstack((m, [0, 0, 0, 1])).T
        return self._velo2cam

    def get_video_odometry(self, drive, indices=None, ext=".txt", return_all=False):
        path = self.root + "/poses/%02d.txt" % drive
        if path not in self.kitti_cache:
            self.kitti_cache[path] = np.genfromtxt(path)
        return self.kitti_cache[path] if return_all else self.kitti_cache[path][indices]

    def odometry_to_positions(self, odometry):
        return np.vstack((odometry.reshape(3, 4), [0, 0, 0, 1]))

    def _get_velodyne_fn(self, drive, t):
        return self.root + "/sequences/%02d/velodyne/%06d.bin" % (drive, t)

    def apply_transform(self, pts, trans):
        return pts @ trans[:3, :3].T + trans[:3, 3]

    def _scan(self, drive, t):
        return np.ascontiguousarray(np.fromfile(self._get_velodyne_fn(drive, t), dtype=np.float32).reshape(-1, 4)[:, :3])

    # ----------------------------------------------------------------------------------------------------------- poses
    def icp_key(self, idx):
        return "%d_%d_%d" % self.files[idx]

    def icp_file(self, idx):
        return self.icp_path + "/" + self.icp_key(idx) + ".npy"

    def initial_pose(self, idx):
        """M of the reference's __getitem__: the odometry's pose of scan t0 in the frame of scan t1, float64 4x4."""
        drive, t0, t1 = self.files[idx]
        p0, p1 = (self.odometry_to_positions(o) for o in self.get_video_odometry(drive, [t0, t1]))
        return (self.velo2cam @ p0.T @ np.linalg.inv(p1.T) @ np.linalg.inv(self.velo2cam)).T

    def refine_poses(self, indices=None, batch_pairs=8):
        """Fill the ICP cache (memory and <root>/icp) for the given items (default: all) that have no file yet, batch_pairs pairs
        per GPU call.  Returns the number of poses computed."""
        todo = [i for i in (range(len(self)) if indices is None else indices)
                if self.icp_key(i) not in self.kitti_icp_cache and not os.path.exists(self.icp_file(i))]
        for b0 in range(0, len(todo), batch_pairs):
            part = todo[b0:b0 + batch_pairs]
            Ms = [self.initial_pose(i) for i in part]
            srcs = [self._scan(self.files[i][0], self.files[i][1]) for i in part]
            tgts = [self._scan(self.files[i][0], self.files[i][2]) for i in part]
            T, _, _ = rawicp.icp_raw_batch(srcs, tgts, np.stack(Ms), self.icp_radius, self.icp_max_iter)
            for i, M, Ti in zip(part, Ms, T.cpu().numpy()):
                reg = Ti @ np.linalg.inv(M)
                M2 = M @ reg
                np.save(self.icp_file(i), M2)
                self.kitti_icp_cache[self.icp_key(i)] = M2
        return len(todo)

    def refined_pose(self, idx):
        key = self.icp_key(idx)
        if key not in self.kitti_icp_cache:
            if not os.path.exists(self.icp_file(idx)):
                print("missing ICP files, recompute it")
                self.refine_poses([idx])
            else:
                self.kitti_icp_cache[key] = np.load(self.icp_file(idx))
        return self.kitti_icp_cache[key]

    # ----------------------------------------------------------------------------------------------------------- items
    def __getitem__(self, idx):
        drive, t0, t1 = self.files[idx]
        tsfm = self.refined_pose(idx)
        rot, trans = tsfm[:3, :3].astype(np.float32), tsfm[:3, 3][:, None].astype(np.float32)
        dev = torch.device(self.device)
        down = voxel.voxel_down_sample_batch([torch.from_numpy(self._scan(drive, t)).to(dev) for t in (t0, t1)], self.voxel_size)
        src_pcd, tgt_pcd = (d.cpu().numpy().astype(np.float64) for d in down)
        src_feats = np.ones_like(src_pcd[:, :1]).astype(np.float32)
        tgt_feats = np.ones_like(tgt_pcd[:, :1]).astype(np.float32)
        if self.data_augmentation:
            src_pcd, tgt_pcd = self._augment(src_pcd, tgt_pcd)
        return src_pcd, tgt_pcd, src_feats, tgt_feats, rot, trans

    def _augment(self, src, tgt):
        """The reference's augmentation branch on the host, drawing from numpy's and random's global generators in its order:
        uniform jitter, one random zyx rotation applied to either cloud, a common scale, a shift per cloud."""
        from scipy.spatial.transform import Rotation
        src = src + (np.random.rand(src.shape[0], 3) - 0.5) * self.augment_noise
        tgt = tgt + (np.random.rand(tgt.shape[0], 3) - 0.5) * self.augment_noise
        rot_ab = Rotation.from_euler("zyx", np.random.rand(3) * np.pi * 2).as_matrix()
        if np.random.rand(1)[0] > 0.5:
            src = np.dot(rot_ab, src.T).T
        else:
            tgt = np.dot(rot_ab, tgt.T).T
        scale = self.augment_scale_min + (self.augment_scale_max - self.augment_scale_min) * random.random()
        src, tgt = src * scale, tgt * scale
        shift_src = np.random.uniform(-self.augment_shift_range, self.augment_shift_range, 3)
        shift_tgt = np.random.uniform(-self.augment_shift_range, self.augment_shift_range, 3)
        return src + shift_src, tgt + shift_tgt
