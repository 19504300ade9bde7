"""The yardstick of the DSM extraction (tests/dsm_ref.py) pinned on the CPU: against an fp32 torch statement of
the reference's cylinder search (process_open_gf.py:219-228), its window ranges and its centre arithmetic.  No GPU, no native library."""
import numpy as np
import pytest
import torch

import dsm_ref as DR

RADIUS = 0.8
NEAR = 1e-6          # queries with a window point this close to the radius may differ from the fp32 sqrt formulation ...
LEFT_OUT_CAP = 1e-3  # ... and may be left out, up to this share (expected 2 pi r * 2 NEAR * rho = 6e-5 at rho = 5.6 / m^2)
QUERIES = 3000


def fp32_search(window, ground):
    """The search as the reference states it, in fp32 torch on the CPU: a window row is in reach of a ground point when the
    fp32 norm of their fp32 xy difference is <= 0.8; the answer is the first row, in row order, that reaches the largest z
    among those in reach, and the ground point itself when none is."""
    w, g = torch.from_numpy(window), torch.from_numpy(ground)
    w_xy, w_z = w[:, :2], w[:, 2]
    answer = g.clone()
    for k in range(g.shape[0]):
        in_reach = torch.nonzero(torch.linalg.vector_norm(w_xy - g[k, :2], dim=1) <= 0.8).flatten()
        if in_reach.numel():
            z = w_z[in_reach]
            answer[k] = w[in_reach[torch.nonzero(z == z.max()).flatten()[0]]]
    return answer.numpy()


@pytest.mark.parametrize("seed,offset", [(0, 0.0), (1, 4.0e5)])
def test_the_yardstick_is_the_references_loop_away_from_the_radius(seed, offset):
    xyz, cls = DR.seeded_tile(seed, 20000, 60.0, offset)
    dem = xyz[cls == 1][:QUERIES]
    want = fp32_search(xyz, dem)
    got, idx = DR.dsm_ref(xyz, dem, RADIUS)
    p64, q64 = xyz.astype(np.float64), dem.astype(np.float64)
    near = np.zeros(dem.shape[0], dtype=bool)
    for j in range(dem.shape[0]):
        d = np.hypot(p64[:, 0] - q64[j, 0], p64[:, 1] - q64[j, 1])
        near[j] = (np.abs(d - RADIUS) < NEAR).any()
    same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    print("\nseed %d offset %g: %d of %d queries near the radius, %d mismatches away from it, %d with a candidate"
          % (seed, offset, near.sum(), dem.shape[0], (~same & ~near).sum(), (idx >= 0).sum()))
    assert near.sum() <= LEFT_OUT_CAP * dem.shape[0]
    assert same[~near].all()
    hit = idx >= 0
    assert hit.sum() > 0.9 * dem.shape[0]  # a ground point is a window point: it finds at least itself
    assert np.array_equal(got[hit], xyz[idx[hit]]) and np.array_equal(got[~hit], dem[~hit])


def test_equal_heights_go_to_the_lowest_row():
    patch = np.array([[0, 0, 1], [0.1, 0, 3], [0, 0.1, 3], [0.1, 0.1, 2]], dtype=np.float32)
    dem = np.array([[0, 0, 0], [5, 5, 7]], dtype=np.float32)
    got, idx = DR.dsm_ref(patch, dem, RADIUS)
    assert idx.tolist() == [1, -1]
    assert np.array_equal(got[0], patch[1]) and np.array_equal(got[1], dem[1])
    assert np.array_equal(fp32_search(patch, dem), got)
    got, idx = DR.dsm_ref(patch[::-1], dem, RADIUS)  # rows reversed: z = [2, 3, 3, 1], the first 3 is now row 1 = old row 2
    assert idx.tolist() == [1, -1] and np.array_equal(got[0], patch[2])


def test_the_radius_is_inclusive_and_taken_as_fp32():
    r32 = np.float32(0.75)
    beyond = np.nextafter(r32, np.float32(np.inf))
    patch = np.array([[r32, 0, 5], [0, beyond, 9]], dtype=np.float32)
    got, idx = DR.dsm_ref(patch, np.zeros((1, 3), np.float32), 0.75)
    assert idx.tolist() == [0]
    # 0.8 is not an fp32 number: the radius used is float32(0.8) = 0.800000011920929, so a point at exactly that distance is in
    patch = np.array([[np.float32(0.8), 0, 5]], dtype=np.float32)
    assert DR.dsm_ref(patch, np.zeros((1, 3), np.float32), 0.8)[1].tolist() == [0]


def test_window_ranges():
    from scream_amd.dsm import tile_windows, window_mask
    for kind, nx, ny in (("train", 17, 17), ("val", 5, 5), ("test", 26, 25)):
        xr, yr = tile_windows(kind)
        assert (xr, yr) == DR.windows_ref(kind) and len(xr) == nx and len(yr) == ny
        assert all(isinstance(v, int) for w in xr + yr for v in w)
    assert tile_windows("train")[0][:3] == [[0, 100], [25, 125], [50, 150]] and tile_windows("train")[1][-1] == [400, 500]
    assert tile_windows("val")[0][-1] == [400, 500]
    assert tile_windows("test")[0][-1] == [2500, 2600] and tile_windows("test")[1][-1] == [2400, 2500]
    with pytest.raises(ValueError):
        tile_windows("all")
    rng = np.random.default_rng(5)
    inp = rng.uniform(0, 500, size=(4000, 3)) + np.array([4.0e5, 3.0e6, 0.0])
    inp[:4, 0] = inp[:, 0].min() + np.array([0.0, 100.0, 25.0, 125.0])  # rows on the window borders: lo inclusive, hi exclusive
    lo = inp.min(axis=0)
    xs, ys = inp[:, 0] - lo[0], inp[:, 1] - lo[1]
    for x, y in (([0, 100], [0, 100]), ([25, 125], [400, 500]), ([100, 200], [200, 300])):
        want = (xs >= x[0]) & (xs < x[1]) & (ys >= y[0]) & (ys < y[1])
        got = window_mask(torch.from_numpy(inp), torch.from_numpy(lo), x, y)
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), want) and want.any()


def test_centre_arithmetic():
    rng = np.random.default_rng(6)
    dem = (rng.uniform(0, 100, size=(500, 3)) + np.array([4.0e5, 3.0e6, 80.0])).astype(np.float32)
    dsm = dem + rng.uniform(0, 9, size=(500, 3)).astype(np.float32)
    rows, centre = DR.centre_ref(dsm, dem)
    stacked = np.vstack([dsm, dem])  # fp32 throughout: one rounded sum of the two extremes per axis, then an exact halving
    lo, hi = stacked.min(axis=0), stacked.max(axis=0)
    middle = ((lo + hi) * np.float32(0.5))[None, :]
    want = np.hstack([dsm - middle, dem - middle])
    assert middle.dtype == np.float32 and want.dtype == np.float32 and rows.dtype == np.float32
    assert np.array_equal(centre.view(np.uint32), middle.view(np.uint32)) and np.array_equal(rows.view(np.uint32), want.view(np.uint32))
    # one fp32 rounding of the sum, then an exact halving: not the float64 midpoint rounded once
    s32 = (lo.astype(np.float64) + hi.astype(np.float64)).astype(np.float32)
    assert np.array_equal(centre[0], s32 / np.float32(2))


def test_tile_windows_dataset_cuts_a_tile_in_the_references_order(tmp_path):
    """process_open_gf.TileWindows on the CPU: windows measured from the tile's minimum corner, window i = x range i % nx,
    y range i // nx, lower border inclusive and upper exclusive, a second tile after the first."""
    import process_open_gf
    rng = np.random.default_rng(9)
    files = []
    for t in range(2):
        tile = np.concatenate([rng.uniform(0, 500, size=(6000, 2)) + np.array([4.0e5 + 1000 * t, 3.0e6]),
                               rng.uniform(0, 30, size=(6000, 1)), rng.integers(1, 3, size=(6000, 1)).astype(np.float64)], axis=1)
        tile[0, :2] = tile[:, :2].min(axis=0)           # a point on the minimum corner: in window 0 only
        tile[1, :2] = tile[0, :2] + np.array([100.0, 200.0])   # on a border: belongs to the window that starts there
        files.append(str(tmp_path / ("tile%d.npy" % t)))
        np.save(files[-1], tile)
    ds = process_open_gf.TileWindows(files, "val", device="cpu")
    xr, yr = DR.windows_ref("val")
    assert len(ds) == 2 * 25
    seen = 0
    for index in (0, 1, 5, 11, 24, 25, 36, 49):
        tile = np.load(files[index // 25])
        i = index % 25
        x, y = xr[i % 5], yr[i // 5]
        sx, sy = tile[:, 0] - tile[:, 0].min(), tile[:, 1] - tile[:, 1].min()
        keep = (sx >= x[0]) & (sx < x[1]) & (sy >= y[0]) & (sy < y[1])
        xyz, cls = ds[index]
        assert xyz.dtype == torch.float64 and np.array_equal(xyz.numpy(), tile[keep, :3]) and np.array_equal(cls.numpy(), tile[keep, 3])
        assert keep.any()
        seen += int(keep.sum())
    tile = np.load(files[0])
    assert (ds[0][0].numpy() == tile[0, :3]).all(axis=1).any() and (ds[11][0].numpy() == tile[1, :3]).all(axis=1).any()  # 11 = x range 1, y range 2
    assert seen > 1000
