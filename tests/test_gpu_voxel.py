"""voxel_down_sample on the MI355X (csrc/voxel.hip, scream_amd/voxel.py) against the float64 restatement of tests/voxel_ref.py.
Every comparison is exact: output length, (i, j, k) order, counts and the bits of the fp32 centroids.  The contract of
include/scream_hip.h makes both sides the same IEEE sequence, so there is no tolerance anywhere in this file.
Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import voxel_ref as VR
from scream_amd import _lib, ops
from scream_amd.voxel import voxel_down_sample, voxel_down_sample_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 2048   # rows per block of the sort (VX_TILE in csrc/voxel.hip): 256 threads x 8 rounds of 64-lane waves


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def gpu_batch(clouds, voxels):
    """numpy fp32 clouds through the public batch call -> (list of fp32 [M,3] arrays, list of int [M] arrays)."""
    pts, cnt = voxel_down_sample_batch([torch.from_numpy(c).to(DEV) for c in clouds], voxels, return_counts=True)
    return [p.cpu().numpy() for p in pts], [c.cpu().numpy() for c in cnt]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(cloud, voxel, got_pts, got_cnt, what=""):
    """Length, order, counts and centroid bits against the yardstick."""
    keys, counts, want = VR.ref32(cloud, voxel)
    assert got_pts.shape == want.shape, "%s: %d voxels, expected %d" % (what, got_pts.shape[0], want.shape[0])
    assert np.array_equal(got_cnt, counts), what
    # rows of `want` are in ascending (i, j, k): equal rows in equal places is the order check; on top, every row must lie in
    # the voxel the yardstick lists at its place wherever the fp32 rounding of the centroid cannot have left it (count 1: the
    # centroid is the point itself)
    assert np.array_equal(got_pts, want), what
    assert np.array_equal(bits(got_pts), bits(want)), what  # also the sign of zero
    single = counts == 1
    if single.any():
        c64 = np.asarray(cloud, dtype=np.float32).astype(np.float64)
        origin = c64.min(axis=0) - float(voxel) * 0.5
        idx = np.floor((got_pts[single].astype(np.float64) - origin) / float(voxel)).astype(np.int64)
        assert np.array_equal(idx, keys[single]), what


def check_batch(clouds, voxels):
    voxels = list(voxels) if isinstance(voxels, (list, tuple)) else [voxels] * len(clouds)
    pts, cnt = gpu_batch(clouds, voxels)
    for i, (c, v) in enumerate(zip(clouds, voxels)):
        check(c, v, pts[i], cnt[i], "cloud %d (%d points, voxel %g)" % (i, c.shape[0], v))
    return pts, cnt


# ---- 1. smallest shapes

def test_one_point_one_voxel_and_every_point_its_own_voxel():
    rng = np.random.default_rng(0)
    one = np.array([[0.3, -7.0, 2.5]], dtype=np.float32)
    same = (rng.random((300, 3)) * 0.4 + 10.0).astype(np.float32)  # voxel 1: origin = min - 0.5, all inside cell 0
    g = np.stack(np.meshgrid(np.arange(7), np.arange(9), np.arange(11), indexing="ij"), axis=-1).reshape(-1, 3)
    own = rng.permutation(g).astype(np.float32)  # unit lattice, voxel 0.5: 693 points, 693 voxels, shuffled rows
    pts, cnt = check_batch([one, same, own], [0.5, 1.0, 0.5])
    assert pts[0].shape == (1, 3) and np.array_equal(pts[0], one)
    assert pts[1].shape == (1, 3) and cnt[1][0] == 300
    assert pts[2].shape == (693, 3) and (cnt[2] == 1).all()
    assert np.array_equal(pts[2], g.astype(np.float32))  # the lattice comes back in ascending (i, j, k)


def test_a_run_of_5000_points_among_singletons():
    """One thread sums the long run serially in row order; its rows are scattered over three blocks of the sort."""
    rng = np.random.default_rng(1)
    run = (rng.random((5000, 3)) * 0.4 + 40.0).astype(np.float32)  # origin -0.5: cell 40 on every axis
    singles = (np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3)
               * 3.0).astype(np.float32)
    cloud = rng.permutation(np.concatenate([run, singles]))
    pts, cnt = check_batch([cloud], 1.0)
    assert cnt[0].max() == 5000 and (cnt[0] == 1).sum() == 1000


LENGTHS = [63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1]


def test_lengths_around_the_wave_the_round_the_block_and_several_blocks():
    clouds = [VR.seeded_cloud("uniform", n, seed=n) for n in LENGTHS]
    check_batch(clouds, 0.05)   # 8000 cells in the unit cube, runs and singletons mixed: 15 key bits, two sort passes
    check_batch(clouds, 0.004)  # 250 cells per axis, nearly every point alone: 24 key bits, three passes (an odd number)
    for c in clouds[6:9]:       # each alone: the grids are then sized by this length
        check_batch([c], 0.05)


def test_an_empty_cloud_between_two_others():
    a, b = VR.seeded_cloud("uniform", 1000, 3), VR.seeded_cloud("uniform", 2500, 4)
    empty = np.zeros((0, 3), dtype=np.float32)
    pts, cnt = check_batch([a, empty, b], 0.1)
    assert pts[1].shape == (0, 3) and cnt[1].shape == (0,)
    pts, _ = check_batch([empty, empty], 0.1)
    assert [p.shape for p in pts] == [(0, 3), (0, 3)]
    assert voxel_down_sample(torch.zeros(0, 3, device=DEV), 0.1).shape == (0, 3)


# ---- 2. boundaries

def _boundary_cloud(k_lo, k_hi, seed):
    """Coordinates exactly on multiples of 0.25 and one fp32 ulp either side, the minimum point at (k_lo + 0.5) * 0.25 on every
    axis so that origin = k_lo * 0.25 exactly and the multiples ARE the cell faces; the first 50 rows are repeated."""
    rng = np.random.default_rng(seed)
    g = (np.arange(k_lo + 1, k_hi + 1) * 0.25).astype(np.float32)
    vals = np.concatenate([g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))])
    p = vals[rng.integers(0, vals.shape[0], size=(2000, 3))]
    low = np.full((1, 3), (k_lo + 0.5) * 0.25, dtype=np.float32)
    return np.concatenate([p, low, p[:50]]).astype(np.float32)


def test_points_on_cell_faces_and_one_ulp_either_side():
    pos = _boundary_cloud(0, 8, seed=5)     # minimum 0.125: origin exactly 0
    neg = _boundary_cloud(-4, 4, seed=6)    # minimum -0.875: origin exactly -1, faces at negative multiples and at 0
    assert pos.min() == np.float32(0.125) and neg.min() == np.float32(-0.875) and (neg < 0).any()
    keys, _, _ = VR.ref32(pos, 0.25)
    on_face = np.float32(1.0)  # 1.0 / 0.25 = 4 exactly: a point at 1.0 is in cell 4, one ulp below in cell 3
    assert np.floor(np.float64(on_face) / 0.25) == 4 and np.floor(np.float64(np.nextafter(on_face, np.float32(0))) / 0.25) == 3
    assert keys.min() == 0 and keys.max() == 8
    check_batch([pos, neg], 0.25)
    check_batch([-pos[::-1].copy()], 0.25)  # all negative


@pytest.mark.parametrize("kind,n,voxel", [("3dmatch", 30000, 0.0625), ("kitti", 30000, 0.3), ("kitti", 30000, 0.7),
                                          ("opengf", 5000, 20.0)])
def test_dataset_voxels_on_dataset_scaled_clouds(kind, n, voxel):
    pts, cnt = check_batch([VR.seeded_cloud(kind, n, seed=17)], voxel)
    assert 8 < pts[0].shape[0] < n


@pytest.mark.parametrize("top,passes", [(2.0 ** 12 - 1, 5), (2.0 ** 21 - 1, 8)])
def test_wide_grids_take_every_pass_of_the_sort(top, passes):
    """Cells 0 .. top on every axis: 3 x 12 key bits = five 8-bit passes, 3 x 21 bits = all eight (the widest grid accepted)."""
    rng = np.random.default_rng(int(top))
    p = np.floor(rng.random((TILE + 500, 3)) * (top + 1))
    p[0], p[1] = 0.0, top
    p[100:140] = p[60:100]  # some shared voxels
    cloud = p.astype(np.float32)
    keys = VR.ref32(cloud, 1.0)[0]
    assert keys.max(axis=0).tolist() == [top] * 3 and (3 * int(top).bit_length() + 7) // 8 == passes
    check_batch([cloud, VR.seeded_cloud("uniform", 700, 2)], [1.0, 0.05])


# ---- 3. stability: the sums run in ascending row index

def test_sum_order_is_the_row_order():
    """All three points of a triple lie in one voxel (voxel 8, origin = -1 - 4).  float64 sums, then / 3, then one rounding:
        rows (1, 2^-60, -1):  (1 + 2^-60) = 1 (2^-60 is below half an ulp of 1 in float64), 1 - 1 = 0           -> 0.0
        rows (1, -1, 2^-60):  (1 - 1) = 0, 0 + 2^-60 = 2^-60, / 3                                              -> 3.0e-19 (0x20aaaaab)
        rows (2^-60, 1, -1):  2^-60 + 1 = 1, 1 - 1 = 0                                                          -> 0.0
    so a kernel that summed a voxel's rows in any other order than the one given returns a different float for the first two
    clouds.  The issue's triple (1, 2^-30, -1) is exact in float64 in EVERY order ((1 + 2^-30) needs 31 bits): it returns
    2^-30 / 3 = 3.1044e-10 (0x2faaaaab) whatever the order, where an fp32 accumulator would lose the 2^-30 ((1 + 2^-30) = 1 in
    fp32) and return 0.0 -- it pins the float64 accumulator, the 2^-60 triples pin the order."""
    t60, t30 = np.float32(2.0 ** -60), np.float32(2.0 ** -30)

    def triple(a, b, c):
        p = np.zeros((3, 3), dtype=np.float32)
        p[:, 0] = [a, b, c]
        return p

    clouds = [triple(1, t60, -1), triple(1, -1, t60), triple(t60, 1, -1), triple(1, t30, -1), triple(1, -1, t30), triple(t30, -1, 1)]
    pts, cnt = check_batch(clouds, 8.0)
    assert all(c.tolist() == [3] for c in cnt)
    x = [float(p[0, 0]) for p in pts]
    assert x[0] == 0.0 and x[2] == 0.0
    assert x[1] == float(np.float32(2.0 ** -60 / 3)) and x[1] != x[0]      # the reordering IS a different float
    assert x[3] == x[4] == x[5] == float(np.float32(2.0 ** -30 / 3)) != 0.0  # float64 sums: exact in every order
    # the same inside a crowd: 600 points in the voxel, the large pair first and last
    rng = np.random.default_rng(8)
    crowd = np.zeros((600, 3), dtype=np.float32)
    crowd[:, 0] = (rng.random(600) * 2.0 ** -40).astype(np.float32)
    crowd[0, 0], crowd[-1, 0] = 3.0, -3.0
    shuffled = crowd[rng.permutation(600)]
    (a, b), _ = check_batch([crowd, shuffled], 16.0)
    assert a.shape == b.shape == (1, 3)


# ---- 4. batched == single, bitwise

def test_batched_equals_single_repeatable_and_order_independent():
    spec = [("uniform", 1, 0.0625), ("3dmatch", 777, 0.0625), ("kitti", TILE, 0.3), ("kitti", 5000, 0.7), ("opengf", 12345, 20.0),
            ("uniform", 3000, 0.25)]
    clouds = [VR.seeded_cloud(k, n, seed=100 + i) for i, (k, n, _) in enumerate(spec)]
    voxels = [v for _, _, v in spec]
    pts, cnt = check_batch(clouds, voxels)
    pts2, cnt2 = gpu_batch(clouds, voxels)
    for i in range(6):
        single = voxel_down_sample(torch.from_numpy(clouds[i]).to(DEV), voxels[i]).cpu().numpy()
        assert np.array_equal(bits(single), bits(pts[i])), i
        assert np.array_equal(bits(pts2[i]), bits(pts[i])) and np.array_equal(cnt2[i], cnt[i]), i
    perm = [4, 0, 5, 2, 1, 3]
    ptsp, cntp = gpu_batch([clouds[i] for i in perm], [voxels[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(bits(ptsp[j]), bits(pts[i])) and np.array_equal(cntp[j], cnt[i]), i


# ---- 5. refused clouds are reported, not faulted

def _packed(clouds, voxels):
    lens = [c.shape[0] for c in clouds]
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    xyz = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    out, out_len, cnt = ops.voxel_down_sample_packed(xyz, torch.from_numpy(row0).to(DEV), torch.tensor(lens, dtype=torch.int32).to(DEV),
                                                     max(lens), torch.tensor(voxels, dtype=torch.float64).to(DEV), want_counts=True)
    return out.cpu().numpy(), out_len.cpu().tolist(), cnt.cpu().numpy(), row0


@pytest.mark.parametrize("bad", ["extent", "nan", "inf"])
def test_a_refused_cloud_reports_minus_one_and_leaves_its_neighbours_alone(bad):
    a, b = VR.seeded_cloud("uniform", 3000, 21), VR.seeded_cloud("kitti", 2100, 22)
    if bad == "extent":
        mid = np.array([[0.0, 0.0, 0.0], [3.0e6, 0.0, 0.0]], dtype=np.float32)  # 3 x 10^6 voxels of 1.0 apart: more than 2^21 cells
    else:
        mid = VR.seeded_cloud("uniform", 500, 23)
        mid[321, 1] = np.nan if bad == "nan" else np.inf
    clouds, voxels = [a, mid, b], [0.05, 1.0, 0.7]
    out, out_len, cnt, row0 = _packed(clouds, voxels)
    assert out_len[1] == -1
    for i in (0, 2):
        m = out_len[i]
        check(clouds[i], voxels[i], out[row0[i]:row0[i] + m], cnt[row0[i]:row0[i] + m], "neighbour %d" % i)
    with pytest.raises(ValueError, match="cloud 1"):
        voxel_down_sample_batch([torch.from_numpy(c).to(DEV) for c in clouds], voxels)
    # exactly 2^21 cells on an axis is still inside: two points 2^21 - 1 voxels apart
    edge = np.array([[0.0, 0.0, 0.0], [2.0 ** 21 - 1, 0.0, 0.0]], dtype=np.float32)
    check_batch([edge], 1.0)


# ---- 6. integration

def test_open_gf_evaluation_builds_its_coarse_dems_on_the_gpu():
    from models.pointnet import DEMTransformer
    from scream_amd.evaluate_open_gf import SCALE_FACTOR, SyntheticDEM, coarse_dems, evaluate_samples
    from scream_amd.synthetic import make_state_dict
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    net = net.to(DEV).eval()
    ds = SyntheticDEM(4, seed0=31, points=600, coarse="gpu")
    samples = [ds[i] for i in range(4)]
    metres = coarse_dems([s[1] for s in samples], DEV, scaled=False)
    for s, c in zip(samples, metres):
        want = VR.ref32(s[1].numpy(), 20.0)[2]
        assert np.array_equal(bits(c.cpu().numpy()), bits(want))
    rows = evaluate_samples(net, samples, coarse="gpu")
    scaled = coarse_dems([s[1] for s in samples], DEV)
    assert all(torch.equal(a, b / SCALE_FACTOR) for a, b in zip(scaled, metres))
    existing = evaluate_samples(net, [(s[0], c.cpu(), s[2], s[3]) for s, c in zip(samples, scaled)])  # the path as it was
    assert np.array_equal(rows, existing) and np.isfinite(rows).all() and rows.shape == (4, 3)


def test_downsample_pair_is_normalize_pair_of_the_yardstick_clouds():
    from scream_amd.data import downsample_pair, normalize_pair
    from scream_amd.synthetic import random_rotation
    rng = np.random.default_rng(41)
    world = VR.seeded_cloud("3dmatch", 24000, 42).astype(np.float64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = random_rotation(rng, 30.0), rng.uniform(-0.5, 0.5, size=3)
    tgt_raw = world[:20000]
    src_raw = (T[:3, :3].T @ (world[4000:] - T[:3, 3]).T).T  # 20 k points each, registered by T
    for mode in ("ball", "bbox"):
        got = downsample_pair(src_raw, tgt_raw, T, 0.0625, mode=mode)
        src = VR.ref32(src_raw.astype(np.float32), 0.0625)[2].astype(np.float64)
        tgt = VR.ref32(tgt_raw.astype(np.float32), 0.0625)[2].astype(np.float64)
        want = normalize_pair(src, tgt, T, mode)
        assert len(got) == len(want) == 6 and got[4] == want[4]
        for g, w in zip(got[:4] + got[5:], want[:4] + want[5:]):
            assert torch.equal(g, w)
        assert 1000 < got[0].shape[0] < 20000
