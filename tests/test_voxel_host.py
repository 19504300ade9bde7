"""voxel_down_sample without a GPU: the yardstick of tests/voxel_ref.py against the restatement that predates the kernels, the
host-side argument checks of the two entry points, and the opt-in switch of the OpenGF datasets (the default stays as it was)."""
import numpy as np
import pytest
import torch

import voxel_ref as VR
from scream_amd import _lib
from scream_amd.evaluate_open_gf import (DEM_COARSE_RESOLUTION, SCALE_FACTOR, OpenGFFiles, SyntheticDEM, make_sample,
                                         voxel_down_sample as host_voxel_down_sample)


@pytest.mark.parametrize("kind,n,voxel", [("3dmatch", 20000, 0.0625), ("kitti", 12000, 0.3), ("kitti", 12000, 0.7),
                                          ("opengf", 4000, 20.0), ("uniform", 5000, 0.05), ("uniform", 1, 0.5)])
def test_voxel_ref_equals_the_restatement_that_predates_the_kernels(kind, n, voxel):
    pts = VR.seeded_cloud(kind, n, seed=n + int(voxel * 1000)).astype(np.float64)
    keys, counts, cent = VR.voxel_ref(pts, voxel)
    want = host_voxel_down_sample(pts, voxel)
    assert np.array_equal(cent, want)  # bit for bit in float64, rows in the order of np.unique(axis=0)
    assert counts.sum() == n and (counts > 0).all()
    flat = (keys[:, 0] * VR.AXIS_CELLS + keys[:, 1]) * VR.AXIS_CELLS + keys[:, 2]
    assert (np.diff(flat) > 0).all()  # strictly ascending (i, j, k)
    origin = pts.min(axis=0) - voxel * 0.5
    assert np.array_equal(np.unique(np.floor((pts - origin) / voxel).astype(np.int64), axis=0), keys)


def test_voxel_ref_sums_in_row_order():
    """1, 2^-60, -1 in one voxel: (1 + 2^-60) - 1 = 0 in row order, (1 - 1) + 2^-60 = 2^-60 for the rows (1, -1, 2^-60)."""
    tiny = 2.0 ** -60
    pts = np.array([[1.0, 0, 0], [tiny, 0, 0], [-1.0, 0, 0]])
    assert VR.voxel_ref(pts, 8.0)[2][0, 0] == 0.0
    assert VR.voxel_ref(pts[[0, 2, 1]], 8.0)[2][0, 0] == tiny / 3
    assert VR.voxel_ref(np.zeros((0, 3)), 1.0)[2].shape == (0, 3)


def _call(lib, **kw):
    a = dict(kw)
    return lib.scream_voxel_down_sample(a["xyz"], a["row0"], a["len"], a["n"], a["max_len"], a["voxel"], a["out"], a["out_len"],
                                        a["count"], a["ws"], a["ws_bytes"], None)


def test_voxel_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    need = lib.scream_voxel_workspace_bytes(1000, 3)
    assert need >= 1000 * (2 * (8 + 4) + 4)  # two (key, row) buffers and the run starts
    assert lib.scream_voxel_workspace_bytes(-1, 3) == -1
    assert lib.scream_voxel_workspace_bytes(1000, -1) == -1
    assert lib.scream_voxel_workspace_bytes(1 << 31, 1) == -1  # rows are int32
    buf = torch.zeros(need // 4 + 16, dtype=torch.float32)  # host memory: every call below must return before touching it
    p = buf.data_ptr()
    p -= p % 16
    ok = dict(xyz=p, row0=p, len=p, n=3, max_len=1000, voxel=p, out=p, out_len=p, count=p, ws=p, ws_bytes=need)
    for name in ("xyz", "row0", "len", "voxel", "out", "out_len", "ws"):
        assert _call(lib, **dict(ok, **{name: None})) == -1, name
    assert _call(lib, **dict(ok, n=-1)) == -1
    assert _call(lib, **dict(ok, max_len=-1)) == -1
    assert _call(lib, **dict(ok, ws_bytes=-1)) == -1
    assert _call(lib, **dict(ok, ws_bytes=lib.scream_voxel_workspace_bytes(1000, 3) - 1)) == -1  # too small for max_len rows
    assert _call(lib, **dict(ok, ws=p + 4)) == -1  # alignment
    assert _call(lib, **dict(ok, n=70000, ws_bytes=lib.scream_voxel_workspace_bytes(1000, 70000))) == -2  # one grid row per cloud


def test_voxel_workspace_is_monotone_in_rows_and_clouds():
    lib = _lib.load()
    sizes = [lib.scream_voxel_workspace_bytes(r, 4) for r in (0, 1, 2047, 2048, 2049, 100000, 100001, 6400000, (1 << 31) - 1)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert lib.scream_voxel_workspace_bytes(5000, 64) >= lib.scream_voxel_workspace_bytes(5000, 1)


def test_voxel_down_sample_of_no_clouds_is_a_no_op():
    lib = _lib.load()
    buf = torch.zeros(1024, dtype=torch.float32)
    p = buf.data_ptr()
    p -= p % 16
    ok = dict(xyz=p, row0=p, len=p, n=0, max_len=0, voxel=p, out=p, out_len=p, count=None, ws=p,
              ws_bytes=lib.scream_voxel_workspace_bytes(0, 0))
    assert _call(lib, **ok) == 0
    assert not buf.any()


def test_python_surface_exists_and_has_no_cpu_path():
    import scream_amd
    from scream_amd.data import downsample_pair  # noqa: F401
    assert scream_amd.voxel_down_sample is scream_amd.voxel.voxel_down_sample
    assert scream_amd.voxel_down_sample_batch([], 0.5) == []
    with pytest.raises(_lib.ScreamHipError):
        scream_amd.voxel_down_sample(torch.zeros(4, 3), 0.5)
    with pytest.raises(ValueError):
        scream_amd.voxel_down_sample_batch([torch.zeros(4, 3)], [0.5, 0.5])
    with pytest.raises(ValueError):
        scream_amd.voxel_down_sample_batch([torch.zeros(4, 2)], 0.5)


def _parent_make_sample(dsm_dem, center):
    """make_sample as it stood before the switch existed, restated."""
    dsm, dem = dsm_dem[:, :3], dsm_dem[:, 3:]
    coarse = host_voxel_down_sample(dem, DEM_COARSE_RESOLUTION)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a / SCALE_FACTOR, dtype=np.float32))
    return f(dsm), f(coarse), f(dem), center


def test_host_coarse_items_are_bitwise_those_of_the_parent(tmp_path):
    rng = np.random.default_rng(5)
    arr = np.concatenate([rng.uniform(0, 500, size=(700, 3)), rng.uniform(0, 500, size=(700, 3))], axis=1)
    center = np.array([250.0, 250.0, 0.0])
    want = _parent_make_sample(arr, center)
    for got in (make_sample(arr, center), make_sample(arr, center, coarse="host")):
        assert all(torch.equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] is center
    (tmp_path / "centers").mkdir()
    np.save(tmp_path / "1.npy", arr)
    np.save(tmp_path / "centers" / "1.npy", center)
    for ds in (OpenGFFiles(str(tmp_path), 1), OpenGFFiles(str(tmp_path), 1, coarse="host")):
        assert all(torch.equal(g, w) for g, w in zip(ds[0][:3], want[:3]))
    a, b = SyntheticDEM(1, seed0=9, points=500)[0], SyntheticDEM(1, seed0=9, points=500, coarse="host")[0]
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    # opt-in: the raw DEM in metres, fp32, in place of the coarse one; everything else untouched
    raw = OpenGFFiles(str(tmp_path), 1, coarse="gpu")[0]
    assert torch.equal(raw[0], want[0]) and torch.equal(raw[2], want[2])
    assert torch.equal(raw[1], torch.from_numpy(arr[:, 3:].astype(np.float32)))
    g = SyntheticDEM(1, seed0=9, points=500, coarse="gpu")[0]
    assert torch.equal(g[0], a[0]) and torch.equal(g[2], a[2]) and g[1].shape == (500, 3) and g[1].dtype == torch.float32
    with pytest.raises(ValueError):
        SyntheticDEM(1, coarse="device")
