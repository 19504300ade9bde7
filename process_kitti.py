"""Drop-in for the reference's ``process_kitti.py`` on the MI355X: raw KITTI odometry to the ``KITTI_<mode>/src%d / tgt%d /
T%d.npy`` folders that ``evaluate_kitti.KittiPairFiles`` and the training loaders read.

    python process_kitti.py --root /data/KITTI-Registration --mode test --out . --icp

``--root`` holds ``dataset/poses``, ``dataset/sequences/%02d/velodyne`` and (written here) ``icp``.  ``--icp`` first refines
every ground-truth pose on the unvoxelised scans (scream_amd.kitti_raw.KITTI_PREDATOR.refine_poses: the float64 raw-scan ICP of
csrc/icp_raw.hip, eight pairs per call); without it the poses are refined on demand, one pair at a time, as the reference does.
Per pair, as the reference does: the 0.3 m clouds of the data set are down-sampled again at 0.7 m (here sixteen pairs per
batched call), T is assembled from the fp32 rot / trans, item 1 of ``test`` is skipped, and the files are numbered by a counter
of their own.  The clouds are saved as float64 arrays holding the fp32 centroids of voxel_down_sample_batch (the caveat of
process_3d_match.py).  Parity with open3d (its ICP, its voxel order) is not pinned.
"""
import argparse
import os

import numpy as np
import torch

from scream_amd import kitti_raw, voxel

PAIRS_PER_CALL = 16
DOWN_VOXEL = 0.7
MODES = ("train", "val", "test")


def pose_of(rot, trans):
    """The 4x4 the reference stacks from the fp32 rot [3,3] and trans [3,1] (float64 holding fp32 values)."""
    return np.concatenate([np.concatenate([rot, trans], axis=1), np.array([[0, 0, 0, 1]])], axis=0)


def save_icp(root, modes=MODES, batch_pairs=8):
    """Refine and cache the pose of every pair of the given modes; returns {mode: poses computed}."""
    return {m: kitti_raw.KITTI_PREDATOR(root, mode=m, data_augmentation=False).refine_poses(batch_pairs=batch_pairs) for m in modes}


def save_pair(mode="train", root=".", out=".", pairs_per_call=PAIRS_PER_CALL, dataset=None):
    """KITTI_<mode>/{src,tgt,T}%d.npy under `out`; returns the number of pairs written."""
    ds = dataset if dataset is not None else kitti_raw.KITTI_PREDATOR(root, mode=mode, data_augmentation=False)
    folder = os.path.join(out, "KITTI_%s" % mode)
    os.makedirs(folder, exist_ok=True)
    items = [i for i in range(len(ds)) if not (mode == "test" and i == 1)]
    dev = torch.device(ds.device)
    saved = 0
    for b0 in range(0, len(items), pairs_per_call):
        got = [ds[i] for i in items[b0:b0 + pairs_per_call]]
        clouds = [torch.from_numpy(np.asarray(c, dtype=np.float32)).to(dev) for g in got for c in (g[0], g[1])]
        down = voxel.voxel_down_sample_batch(clouds, DOWN_VOXEL)
        for k, g in enumerate(got):
            src, tgt = (down[2 * k + j].cpu().numpy().astype(np.float64) for j in (0, 1))
            print("downsampled  src: %d  tgt: %d" % (src.shape[0], tgt.shape[0]))
            np.save(os.path.join(folder, "src%d.npy" % saved), src)
            np.save(os.path.join(folder, "tgt%d.npy" % saved), tgt)
            np.save(os.path.join(folder, "T%d.npy" % saved), pose_of(g[4], g[5]))
            saved += 1
        print("\r%d / %d" % (min(len(items), b0 + pairs_per_call), len(items)), end="", flush=True)
    print()
    return saved


def check_saved_pairs(mode="test", out="."):
    """The extents of every saved pair once registered, last pair first (the reference's printed line; no viewer)."""
    folder = os.path.join(out, "KITTI_%s" % mode)
    n = len([f for f in os.listdir(folder) if f.startswith("T") and f.endswith(".npy")])
    for i in range(n - 1, -1, -1):
        src, tgt, T = (np.load(os.path.join(folder, "%s%d.npy" % (k, i))) for k in ("src", "tgt", "T"))
        pts = np.concatenate([src @ T[:3, :3].T + T[:3, 3], tgt], axis=0)
        hi, lo = pts.max(axis=0), pts.min(axis=0)
        print("x: %.3f - %.3f, %.3f   y: %.3f - %.3f, %.3f  z: %.3f - %.3f, %.3f  %d"
              % (lo[0], hi[0], hi[0] - lo[0], lo[1], hi[1], hi[1] - lo[1], lo[2], hi[2], hi[2] - lo[2], i))
    return n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the folder holding dataset/poses, dataset/sequences and icp")
    ap.add_argument("--mode", choices=MODES, required=True)
    ap.add_argument("--out", default=".")
    ap.add_argument("--icp", action="store_true", help="refine and cache every pose of the mode first, eight pairs per call")
    ap.add_argument("--check", action="store_true", help="print the extents of the saved pairs instead of writing them")
    ap.add_argument("--pairs-per-call", type=int, default=PAIRS_PER_CALL)
    a = ap.parse_args()
    if a.check:
        check_saved_pairs(a.mode, a.out)
    else:
        if a.icp:
            print(save_icp(a.root, (a.mode,)))
        print(save_pair(a.mode, a.root, a.out, a.pairs_per_call))
