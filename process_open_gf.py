"""Drop-in for the reference's ``process_open_gf.py`` (``split_dataset_as_patch``, lines 193-263) on the MI355X.

    python process_open_gf.py --tiles OpenGF_np/test/T1.npy --kind test --name test --save-center [--root .]

A tile file is a [N,4] array (x, y, z, class with ground = 1), as the reference's ``save_open_gf_as_np`` writes it.
"""
import argparse
import os

import numpy as np
import torch

from scream_amd.dsm import make_dsm_dem_batch, tile_windows, window_mask

WINDOWS_PER_CALL = 16


class TileWindows(torch.utils.data.Dataset):
    """The windows of a list of [N,4] tile files, in the reference's order: (sub_xyz, sub_cls) per window.  The window masks are
    evaluated on the GPU in float64; a tile is loaded once and kept on the device while its windows are read."""

    def __init__(self, files, kind, device="cuda"):
        self.files, self.kind, self.device = list(files), kind, torch.device(device)
        self.xr, self.yr = tile_windows(kind)
        self._loaded = (None, None, None)

    def __len__(self):
        return len(self.files) * len(self.xr) * len(self.yr)

    def __getitem__(self, index):
        per_tile = len(self.xr) * len(self.yr)
        f = self.files[index // per_tile]
        if self._loaded[0] != f:
            tile = torch.from_numpy(np.load(f)).to(self.device)
            self._loaded = (f, tile, tile[:, :3].min(dim=0).values)
        _, tile, lo = self._loaded
        i = index % per_tile
        m = window_mask(tile, lo, self.xr[i % len(self.xr)], self.yr[i // len(self.xr)])
        return tile[m, :3], tile[m, 3]


def split_dataset_as_patch(dataset, dataset_name="train", save_center=False, root=".", windows_per_call=WINDOWS_PER_CALL):
    """Every (sub_xyz, sub_cls) of `dataset` -> <root>/OpenGF_<name>/<i>.npy ([n,6] fp32: dsm - centre | dem - centre, i from
    1) and, with save_center, <root>/OpenGF_<name>/centers/<i>.npy ([1,3]).  `windows_per_call` windows share every launch."""
    out_dir = os.path.join(root, "OpenGF_%s" % dataset_name)
    os.makedirs(os.path.join(out_dir, "centers") if save_center else out_dir, exist_ok=True)
    n = len(dataset)
    for i0 in range(0, n, windows_per_call):
        items = [dataset[i] for i in range(i0, min(n, i0 + windows_per_call))]
        rows, centres = make_dsm_dem_batch([it[0] for it in items], [it[1] for it in items])
        for k, (r, c) in enumerate(zip(rows, centres)):
            np.save(os.path.join(out_dir, "%d.npy" % (i0 + k + 1)), r.cpu().numpy())
            if save_center:
                np.save(os.path.join(out_dir, "centers", "%d.npy" % (i0 + k + 1)), c.cpu().numpy())
        print("\r%s: %d / %d" % (dataset_name, min(n, i0 + windows_per_call), n), end="", flush=True)
    print()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", nargs="+", required=True, help="[N,4] .npy tile files (x, y, z, class)")
    ap.add_argument("--kind", choices=["train", "val", "test"], required=True)
    ap.add_argument("--name", default=None, help="output folder OpenGF_<name> (default: the kind)")
    ap.add_argument("--root", default=".")
    ap.add_argument("--save-center", action="store_true")
    a = ap.parse_args()
    split_dataset_as_patch(TileWindows(a.tiles, a.kind), a.name or a.kind, a.save_center, a.root)
