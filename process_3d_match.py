"""Drop-in for the reference's ``process_3d_match.py`` on the MI355X: the PREDATOR fragments of 3DMatch to the
``src%d / tgt%d / T%d.npy`` folders that ``PairFileDataset`` and the ``evaluate_3d_*`` wrappers read.

    python process_3d_match.py --root /data/indoor --info /data/indoor/3DLoMatch.pkl --kind test_3dlomatch \\
        --gt-info /data/3DMatch/info/3DLoMatch --out . --with-info

``--info`` is one of PREDATOR's pickles (a dict with ``rot`` [n,3,3], ``trans`` [n,3,1] or [n,3], ``src`` / ``tgt`` paths
relative to ``--root``; the clouds are the ``.pth`` arrays).  Per pair, as the reference does: the overlap is the set of source
points with a target point within 0.03 m once registered (scream_amd/overlap.py: the exact float64 radius search of
csrc/radius.hip in place of one KD-tree query per point), ``ratio = overlap / points``; the pair goes to

    --kind train / val      3DMatch_train / 3DMatch_val: always, and once more without its overlapping points when ratio <= 0.3
    --kind test_3dmatch     3DMatch_test when ratio > 0.3
    --kind test_3dlomatch   3DLoMatch_test when ratio > 0.1, 3DZeroMatch_test (source without its overlapping points) when ratio <= 0.3

with the clouds down-sampled at 0.0625 m and saved as float64 arrays (the reference's ``np.asarray(pc.points)``), T as the
float64 4x4, under the reference's counters and file names.  ``--with-info`` also writes ``info/scene_names.txt`` (the scene
directory of the source path, as datasets/three_d_match.py:99 takes it), ``info/idx%d.npy`` ([tgt, src] fragment numbers) and,
with ``--gt-info``, ``info/covariance%d.npy`` from the benchmark's ``<scene>/gt.info`` files.

Known difference from the reference: open3d averages the points of a voxel in float64; here the fp32 points are averaged in
float64 and the mean is rounded once to fp32 before it is stored as float64 -- half an fp32 ulp per coordinate, the caveat
make_dsm_dem_batch documents.  Parity with open3d (its KD-tree, its voxel order) is not pinned.
"""
import argparse
import os
import pickle

import numpy as np
import torch

from scream_amd.overlap import ZERO_SET, SETS, select_outputs

PAIRS_PER_CALL = 16


def read_gt_info(path):
    """A benchmark gt.info file -> {(tgt, src): float32 [6,6]}: blocks of seven lines, "tgt src n_fragments" and six rows."""
    with open(path) as f:
        lines = [l.split() for l in f if l.strip()]
    return {(int(lines[k][0]), int(lines[k][1])): np.array(lines[k + 1:k + 7], dtype=np.float32) for k in range(0, len(lines) - 6, 7)}


class PredatorPairs(torch.utils.data.Dataset):
    """The pairs of one PREDATOR info pickle: (src [N,3] fp32, tgt [M,3] fp32 on `device`, rot float32 [3,3], trans float32
    [3,1], idx int [2] = [tgt, src] fragment numbers, covariance float32 [6,6] or None, scene name).  `gt_info`: the directory
    holding <scene>/gt.info (None: no covariances)."""

    def __init__(self, root, info, gt_info=None, device="cuda"):
        if isinstance(info, str):
            with open(info, "rb") as f:
                info = pickle.load(f)
        self.root, self.infos, self.gt_info, self.device = root, info, gt_info, torch.device(device)
        self._cov = {}

    def __len__(self):
        return len(self.infos["rot"])

    def _cloud(self, rel):
        a = torch.load(os.path.join(self.root, rel), weights_only=False)
        return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(device=self.device, dtype=torch.float32).contiguous()

    def __getitem__(self, item):
        src_rel, tgt_rel = self.infos["src"][item], self.infos["tgt"][item]
        number = lambda p: int(p.split("_")[-1].replace(".pth", ""))
        src_idx, tgt_idx = number(src_rel), number(tgt_rel)
        scene = src_rel.replace("\\", "/").split("/")[-2]
        cov = None
        if self.gt_info is not None:
            if scene not in self._cov:
                self._cov[scene] = read_gt_info(os.path.join(self.gt_info, scene, "gt.info"))
            cov = self._cov[scene][(tgt_idx, src_idx)]
        rot = np.asarray(self.infos["rot"][item]).astype(np.float32)
        trans = np.asarray(self.infos["trans"][item]).astype(np.float32).reshape(3, 1)
        return self._cloud(src_rel), self._cloud(tgt_rel), rot, trans, np.array([tgt_idx, src_idx]), cov, scene


def prepare(dataset, pairs_per_call=PAIRS_PER_CALL):
    """Every pair of `dataset` through prepare_3dmatch_batch, `pairs_per_call` pairs per batch: the dicts, with idx, covariance
    and scene added."""
    from scream_amd.overlap import prepare_3dmatch_batch
    n = len(dataset)
    for i0 in range(0, n, pairs_per_call):
        items = [dataset[i] for i in range(i0, min(n, i0 + pairs_per_call))]
        out = prepare_3dmatch_batch([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items])
        for d, it in zip(out, items):
            d.update(idx=it[4], covariance=it[5], scene=it[6])
            yield d
        print("\r%d / %d" % (min(n, i0 + pairs_per_call), n), end="", flush=True)
    print()


def _points64(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def save_pairs(kind, prepared, out=".", clouds=True, info=False):
    """Write the prepared pairs (dicts of prepare_3dmatch_batch) to the folders select_outputs names, under `out`; returns
    {folder: pairs written}.  clouds: src%d / tgt%d / T%d.npy.  info: info/scene_names.txt, info/idx%d.npy and, where the
    dict holds one, info/covariance%d.npy -- at the same counters."""
    folders = [SETS[kind]] + ([ZERO_SET] if kind == "test_3dlomatch" else [])
    counters = {f: 0 for f in folders}
    scenes = {f: [] for f in folders}
    for f in folders:
        os.makedirs(os.path.join(out, f, "info") if info else os.path.join(out, f), exist_ok=True)
    for d in prepared:
        for folder, which in select_outputs(kind, d["n_overlap"], d["n_src"]):
            k, base = counters[folder], os.path.join(out, folder)
            if clouds:
                np.save(os.path.join(base, "src%d.npy" % k), _points64(d[which]))
                np.save(os.path.join(base, "tgt%d.npy" % k), _points64(d["tgt"]))
                np.save(os.path.join(base, "T%d.npy" % k), np.asarray(d["T"], dtype=np.float64))
            if info:
                scenes[folder].append(d["scene"] + "\n")
                np.save(os.path.join(base, "info", "idx%d.npy" % k), np.asarray(d["idx"]))
                if d.get("covariance") is not None:
                    np.save(os.path.join(base, "info", "covariance%d.npy" % k), np.asarray(d["covariance"], dtype=np.float32))
            counters[folder] = k + 1
    if info:
        for f in folders:
            with open(os.path.join(out, f, "info", "scene_names.txt"), "w") as fh:
                fh.writelines(scenes[f])
    return counters


def _run(kind, dataset, out, pairs_per_call, prepared, clouds, info):
    return save_pairs(kind, prepared if prepared is not None else prepare(dataset, pairs_per_call), out, clouds, info)


def save_train(dataset=None, out=".", pairs_per_call=PAIRS_PER_CALL, prepared=None):
    """3DMatch_train/{src,tgt,T}%d.npy: every pair, and once more with the zero-overlap source when ratio <= 0.3."""
    return _run("train", dataset, out, pairs_per_call, prepared, True, False)


def save_val(dataset=None, out=".", pairs_per_call=PAIRS_PER_CALL, prepared=None):
    """3DMatch_val/{src,tgt,T}%d.npy, by the rule of save_train."""
    return _run("val", dataset, out, pairs_per_call, prepared, True, False)


def save_test_3DMatch(dataset=None, out=".", pairs_per_call=PAIRS_PER_CALL, prepared=None):
    """3DMatch_test/{src,tgt,T}%d.npy: the pairs with ratio > 0.3."""
    return _run("test_3dmatch", dataset, out, pairs_per_call, prepared, True, False)


def save_lo_and_zero_match(dataset=None, out=".", pairs_per_call=PAIRS_PER_CALL, prepared=None):
    """3DLoMatch_test (ratio > 0.1) and 3DZeroMatch_test (ratio <= 0.3, the source without its overlapping points)."""
    return _run("test_3dlomatch", dataset, out, pairs_per_call, prepared, True, False)


def save_test_3DMatch_info(dataset=None, out=".", pairs_per_call=PAIRS_PER_CALL, prepared=None):
    """3DMatch_test/info: scene_names.txt, idx%d.npy, covariance%d.npy at the counters of save_test_3DMatch."""
    return _run("test_3dmatch", dataset, out, pairs_per_call, prepared, False, True)


def save_lo_and_zero_match_info(dataset=None, out=".", pairs_per_call=PAIRS_PER_CALL, prepared=None):
    """3DLoMatch_test/info and 3DZeroMatch_test/info at the counters of save_lo_and_zero_match."""
    return _run("test_3dlomatch", dataset, out, pairs_per_call, prepared, False, True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the folder the paths of the info pickle are relative to")
    ap.add_argument("--info", required=True, help="PREDATOR info pickle (train_info.pkl, val_info.pkl, 3DMatch.pkl, 3DLoMatch.pkl)")
    ap.add_argument("--kind", choices=sorted(SETS), required=True)
    ap.add_argument("--gt-info", default=None, help="directory of <scene>/gt.info files (covariances of the test pairs)")
    ap.add_argument("--out", default=".")
    ap.add_argument("--with-info", action="store_true", help="also write info/scene_names.txt, idx and covariance files")
    ap.add_argument("--pairs-per-call", type=int, default=PAIRS_PER_CALL)
    a = ap.parse_args()
    ds = PredatorPairs(a.root, a.info, a.gt_info)
    print(save_pairs(a.kind, prepare(ds, a.pairs_per_call), a.out, True, a.with_info))
