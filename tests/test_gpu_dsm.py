"""DSM extraction on the MI355X (csrc/dsm.hip, scream_amd/dsm.py) against the brute-force float64 restatement of
tests/dsm_ref.py.  Every comparison covers out_xyz AND out_idx and is exact: the contract of include/scream_hip.h makes both
sides the same IEEE sequence, so there is no tolerance anywhere in this file.  Run with `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dsm_ref as DR
import voxel_ref as VR
from scream_amd import ScreamHipError, _lib, ops
from scream_amd.dsm import extract_dsm, extract_dsm_batch, make_dsm_dem, make_dsm_dem_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_batch(patches, dems, radius=0.8):
    """numpy fp32 clouds through the public batch call -> list of (xyz fp32 [N,3], idx int32 [N])."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)).to(DEV)
    pts, idx = extract_dsm_batch([t(p) for p in patches], [t(d) for d in dems], radius, return_index=True)
    return [(p.cpu().numpy(), i.cpu().numpy()) for p, i in zip(pts, idx)]


def same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits(got[0]), bits(want[0])), what


def check_batch(patches, dems, radius=0.8):
    got = gpu_batch(patches, dems, radius)
    want = [DR.dsm_ref(p, d, radius) for p, d in zip(patches, dems)]
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, "cloud %d (%d window points, %d ground points, radius %g)" % (i, len(patches[i]), len(dems[i]), radius))
    return want


# ---- 1. seeded tiles

@functools.lru_cache(maxsize=None)
def tile(seed, offset):
    xyz, cls = DR.seeded_tile(seed, 20000, 60.0, offset)
    dem = xyz[cls == 1]
    return xyz, dem, DR.dsm_ref(xyz, dem, 0.8)


@pytest.mark.parametrize("seed,offset", [(0, 0.0), (1, 4.0e5)])
def test_seeded_tile_with_all_its_ground_points(seed, offset):
    xyz, dem, want = tile(seed, offset)
    same(gpu_batch([xyz], [dem])[0], want)
    assert (want[1] >= 0).all() and (want[0][:, 2] > dem[:, 2]).sum() > 1000  # vegetation over much of the ground


# ---- 2. at the radius, on the cell borders

LATTICE_PROBES = ((0.0, 0.0), (3.0, 3.0), (6.0, 6.0), (1.5, 5.25), (4.5, 0.75))


LATTICE_ANCHORS = np.asarray([[-8, -8, 99], [24, 24, 99]], dtype=np.float32)


def lattice_cloud(k):
    """Coordinates on multiples of 1/4 (radius 0.75: points at distance exactly 0.75 of every query, included), shifted as a
    whole by k/8; heights from {0..3}, so equal maxima across cells are everywhere.  Around some queries: a very high point one
    fp32 step beyond the radius (excluded), and a higher one two cells away.
    Two anchor rows at (-8, -8) and (24, 24) are NOT shifted: they fix the kernel's grid at 32 x 32 cells of exactly 1 m from
    (-8, -8) (652 rows give 32 cells per axis, 32 m / 32 > 1.001 x 0.75), so the shifts move lattice and queries against the
    grid: at k = 0 every fourth query sits exactly on a cell border or corner, at the other k the borders cut the discs
    elsewhere.  The anchors are out of every query's reach."""
    rng = np.random.default_rng(100 + k)
    g = np.stack(np.meshgrid(np.arange(25), np.arange(25), indexing="ij"), axis=-1).reshape(-1, 2) * 0.25
    lat = np.concatenate([g, rng.integers(0, 4, size=(g.shape[0], 1)).astype(np.float64)], axis=1).astype(np.float32)
    r32, up, down = np.float32(0.75), np.float32(np.inf), np.float32(-np.inf)
    extra = []
    for qx, qy in LATTICE_PROBES:  # far enough apart that the points planted around one are out of reach of the others
        qx, qy = np.float32(qx), np.float32(qy)
        extra += [[np.nextafter(qx + r32, up), qy, 50.0], [qx, np.nextafter(qy + r32, up), 60.0], [np.nextafter(qx - r32, down), qy, 70.0],
                  [qx + np.float32(1.5), qy, 80.0], [qx + r32, qy + np.float32(0.0625), 90.0]]
    patch = np.concatenate([lat, np.asarray(extra, dtype=np.float32)], axis=0)
    patch = patch[rng.permutation(patch.shape[0])]
    dem = lat.copy()
    dem[:, 2] = -1.0
    shift = np.array([k / 8.0, k / 8.0, 0.0], dtype=np.float32)
    return np.concatenate([patch + shift, LATTICE_ANCHORS], axis=0), dem + shift


def test_lattice_at_the_radius_through_eight_shifts():
    clouds = [lattice_cloud(k) for k in range(8)]
    want = check_batch([c[0] for c in clouds], [c[1] for c in clouds], 0.75)
    xyz, idx = want[0]  # the unshifted cloud, for the properties the construction is about
    p, q = clouds[0]
    d2 = (xyz[:, 0].astype(np.float64) - q[:, 0]) ** 2 + (xyz[:, 1].astype(np.float64) - q[:, 1]) ** 2
    assert (idx >= 0).all() and (d2 <= 0.5625).all() and (d2 == 0.5625).sum() > 50  # winners exactly at the radius
    for qx, qy in LATTICE_PROBES:  # none of the high points one step outside the disc, or two cells away, was taken
        j = np.nonzero((q[:, 0] == qx) & (q[:, 1] == qy))[0]
        assert j.size == 1 and xyz[j[0], 2] <= 3.0
        planted = p[(p[:, 2] >= 50) & (np.hypot(p[:, 0] - qx, p[:, 1] - qy) < 1.6)]
        assert planted.shape[0] == 5 and (np.hypot(planted[:, 0].astype(np.float64) - qx, planted[:, 1].astype(np.float64) - qy) > 0.75).all()
    on_border = (q[:, 0] == np.floor(q[:, 0])) | (q[:, 1] == np.floor(q[:, 1]))  # 1 m cells from (-8, -8): integer coordinates
    assert on_border.sum() == 7 * 25 + 7 * 25 - 49 and np.array_equal(p[-2:], LATTICE_ANCHORS)
    assert xyz[:, 2].max() == 90.0  # ... while each of them is the winner of the queries it does lie within reach of


# ---- 3. ties

def test_equal_heights_in_one_cell_in_two_cells_and_in_the_cell_scanned_last():
    anchor = [[0, 0, 0], [20, 20, 0]]  # fix the grid: ten rows get 8 x 8 cells, 2.5 m each from (0, 0); the last two queries sit on cell corners
    a = [[10.1, 10.1, 5], [10.15, 10.1, 5]]              # same cell
    b = [[29.5 - 15, 5.0, 7], [30.5 - 15, 5.0, 7]]       # either side of the border at x = 15: two cells of one grid row
    c = [[5.3, 15.5, 9], [5.3, 14.5, 9], [4.6, 15.5, 9], [4.6, 14.5, 9]]  # the four cells around the corner (5, 15); the first row lies in the one scanned last
    patch = np.asarray(anchor + a + b + c, dtype=np.float32)
    dem = np.asarray([[10.12, 10.1, 0], [15.0, 5.0, 0], [5.0, 15.0, 0]], dtype=np.float32)
    want = check_batch([patch], [dem])[0]
    assert want[1].tolist() == [2, 4, 6]
    tied = [[2, 3], [4, 5], [6, 7, 8, 9]]
    rng = np.random.default_rng(7)
    perms = [rng.permutation(patch.shape[0]) for _ in range(6)] + [np.arange(patch.shape[0])[::-1].copy()]
    got = gpu_batch([patch[perm] for perm in perms], [dem] * len(perms))
    for perm, (xyz, idx) in zip(perms, got):
        pos = np.argsort(perm)  # new row of every old row
        expect = [min(pos[t] for t in rows) for rows in tied]
        assert idx.tolist() == expect
        assert np.array_equal(bits(xyz), bits(patch[perm][idx]))
        same((xyz, idx), DR.dsm_ref(patch[perm], dem))


# ---- 4. no candidate, outside the bounds, one point

def test_no_candidate_returns_the_ground_point_itself():
    rng = np.random.default_rng(8)
    patch = np.concatenate([rng.uniform(0, 10, size=(400, 2)), rng.uniform(0, 5, size=(400, 1))], axis=1).astype(np.float32)
    patch = np.concatenate([patch, np.asarray([[0, 0, 1], [10, 10, 2], [0, 5, 3]], dtype=np.float32)])
    dem = np.asarray([[30, 30, 1], [-50, -50, 2], [1.0e4, 5, 3], [5, -1.0e4, 4],   # far outside the bounding box
                      [-0.5, 0, 5], [10.5, 10.5, 6], [-0.7, 5.0, 7], [-0.81, 5.0, 8],  # outside it, some within reach of a border point
                      [5, 5, 9]], dtype=np.float32)
    want = check_batch([patch], [dem])[0]
    assert want[1][:4].tolist() == [-1] * 4 and np.array_equal(bits(want[0][:4]), bits(dem[:4]))
    assert want[1][4] == 400 and want[1][5] == 401 and want[1][6] == 402 and want[1][7] == -1 and want[1][8] >= 0


def test_a_window_of_one_point():
    patch = np.asarray([[1, 2, 3]], dtype=np.float32)
    dem = np.asarray([[1.5, 2.5, 0], [1, 2.8, 0], [1, 2.81, 0], [1, 2, 3], [-7, 2, 1]], dtype=np.float32)
    want = check_batch([patch], [dem])[0]
    assert want[1].tolist() == [0, 0, -1, 0, -1]


# ---- 5. density

def test_twenty_thousand_points_in_one_cell():
    rng = np.random.default_rng(9)
    dense = np.concatenate([rng.uniform(20.0, 20.5, size=(20000, 2)), rng.uniform(0, 30, size=(20000, 1))], axis=1)
    spread = np.concatenate([rng.uniform(0, 50, size=(100, 2)), rng.uniform(0, 30, size=(100, 1))], axis=1)
    patch = np.concatenate([dense, spread]).astype(np.float32)
    patch[[17, 15000], 2] = 31.0  # the two highest, equal
    dem = np.concatenate([[[20.25, 20.25, 0.0]], np.concatenate([spread[:99, :2] + 0.1, np.zeros((99, 1))], axis=1)]).astype(np.float32)
    want = check_batch([patch], [dem])[0]
    assert want[1][0] == 17 and (want[1][1:] >= 0).all()


# ---- 6. lengths

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000]


def test_lengths_around_the_wave_and_the_block():
    patches, dems = [], []
    for n in LENGTHS:
        rng = np.random.default_rng(1000 + n)
        patches.append(rng.uniform(0, 12, size=(n, 3)).astype(np.float32))
        dems.append(rng.uniform(0, 12, size=(n, 3)).astype(np.float32))
    want = check_batch(patches, dems)
    check_batch(patches, dems[::-1])  # every window length against another ground length
    assert (want[-1][1] >= 0).sum() > 500


# ---- 7. batches

def ragged():
    rng = np.random.default_rng(11)
    mk = lambda n, s: (rng.uniform(0, s, size=(n, 3)) + rng.uniform(-100, 100, size=(1, 3))).astype(np.float32)
    a, b, c, d = mk(700, 15), mk(0, 1), mk(1300, 25), mk(300, 10)
    qa = (a[:333] + np.float32(0.2)).astype(np.float32)
    qb = mk(50, 5)
    qc = (c[:900] - np.float32(0.3)).astype(np.float32)
    return [a, b, c, d], [qa, qb, qc, np.zeros((0, 3), np.float32)]


def test_batched_is_single_repeatable_and_independent_of_the_order_of_the_clouds():
    patches, dems = ragged()
    want = check_batch(patches, dems)
    assert want[1][1].tolist() == [-1] * 50 and np.array_equal(bits(want[1][0]), bits(dems[1]))  # the empty window
    assert want[3][0].shape == (0, 3) and want[3][1].shape == (0,)
    first = gpu_batch(patches, dems)
    again = gpu_batch(patches, dems)
    rev = gpu_batch(patches[::-1], dems[::-1])[::-1]
    for i in range(4):
        single = gpu_batch([patches[i]], [dems[i]])[0]
        for other in (again[i], rev[i], single):
            same(other, first[i], "cloud %d" % i)
    t = lambda a: torch.from_numpy(a).to(DEV)
    one = extract_dsm(t(patches[0]), t(dems[0]))
    assert isinstance(one, torch.Tensor) and np.array_equal(bits(one.cpu().numpy()), bits(first[0][0]))
    assert extract_dsm_batch([], []) == [] and extract_dsm_batch([], [], return_index=True) == ([], [])


# ---- 8. a grid that must coarsen

def test_a_three_kilometre_strip():
    rng = np.random.default_rng(12)
    patch = np.concatenate([rng.uniform(0, 3000, size=(5000, 1)), rng.uniform(0, 10, size=(5000, 1)), rng.uniform(0, 40, size=(5000, 1))],
                           axis=1).astype(np.float32)
    dem = patch[rng.permutation(5000)[:1500]].copy()
    dem[:, :2] += rng.uniform(-0.4, 0.4, size=(1500, 2)).astype(np.float32)
    dem[:, 2] = 0
    for radius in (0.8, 6.0):
        want = check_batch([patch], [dem], radius)[0]
        assert (want[1] >= 0).all()


# ---- 9. refusals

def raw_call(radius, n_clouds, out_xyz, out_idx):
    lib = _lib.load()
    patch = torch.zeros(4, 3, device=DEV)
    dem = torch.ones(4, 3, device=DEV)
    meta = torch.tensor([[0], [4]], dtype=torch.int32).to(DEV)
    ws = torch.empty(max(lib.scream_dsm_workspace_bytes(4, n_clouds, 4), 16), device=DEV, dtype=torch.uint8)
    return lib.scream_dsm_extract(patch.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), 4, 4, dem.data_ptr(), meta[0].data_ptr(),
                                  meta[1].data_ptr(), 4, 4, n_clouds, C.c_float(radius), out_xyz.data_ptr(), out_idx.data_ptr(),
                                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)


def test_refusals_return_their_status_and_launch_nothing():
    out_xyz = torch.full((4, 3), -77.0, device=DEV)
    out_idx = torch.full((4,), -77, device=DEV, dtype=torch.int32)
    for radius in (0.0, -0.8, float("inf"), float("-inf"), float("nan")):
        assert raw_call(radius, 1, out_xyz, out_idx) == -1, radius  # SCREAM_EINVAL
    assert raw_call(0.8, 65536, out_xyz, out_idx) == -2  # SCREAM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (out_xyz == -77.0).all() and (out_idx == -77).all()
    assert raw_call(0.8, 0, out_xyz, out_idx) == 0
    torch.cuda.synchronize()
    assert (out_xyz == -77.0).all() and (out_idx == -77).all()
    assert raw_call(0.8, 1, out_xyz, out_idx) == 0  # the same arguments with nothing to refuse: all four rows written
    torch.cuda.synchronize()
    assert (out_idx == -1).all() and (out_xyz == 1.0).all()
    lib = _lib.load()
    assert lib.scream_dsm_workspace_bytes(-1, 1, 0) == -1 and lib.scream_dsm_workspace_bytes(4, 1, 5) == -1
    assert lib.scream_abi_version() == 21


def test_a_cloud_whose_rows_leave_the_arrays_is_skipped_on_the_device():
    """The row arrays live on the device and the call does not synchronise, so such a cloud cannot be refused by the host: it
    reads and writes nothing, in the extraction and in the assembly, and its neighbours are as if it were not there."""
    lib = _lib.load()
    rng = np.random.default_rng(13)
    patch = rng.uniform(0, 6, size=(300, 3)).astype(np.float32)
    dem = rng.uniform(0, 6, size=(90, 3)).astype(np.float32)
    want = [DR.dsm_ref(patch[0:100], dem[0:30]), None, DR.dsm_ref(patch[200:300], dem[60:90])]
    tp, td = torch.from_numpy(patch).to(DEV), torch.from_numpy(dem).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    good = [[0, 100, 200], [100, 100, 100], [0, 30, 60], [30, 30, 30]]
    for what, row, value in (("patch rows past the array", 0, 250), ("patch longer than max_p_len", 1, 101), ("negative patch row", 0, -1),
                             ("dem rows past the array", 2, 70), ("dem longer than max_d_len", 3, 31), ("negative dem length", 3, -5)):
        meta = [list(r) for r in good]
        meta[row][1] = value
        m = torch.tensor(meta, dtype=torch.int32).to(DEV)
        out_xyz = torch.full((90, 3), -77.0, device=DEV)
        out_idx = torch.full((90,), -77, device=DEV, dtype=torch.int32)
        ws = torch.empty(lib.scream_dsm_workspace_bytes(300, 3, 100), device=DEV, dtype=torch.uint8)
        rc = lib.scream_dsm_extract(tp.data_ptr(), m[0].data_ptr(), m[1].data_ptr(), 100, 300, td.data_ptr(), m[2].data_ptr(),
                                    m[3].data_ptr(), 30, 90, 3, C.c_float(0.8), out_xyz.data_ptr(), out_idx.data_ptr(), ws.data_ptr(),
                                    ws.numel(), stream)
        assert rc == 0, what
        xyz, idx = out_xyz.cpu().numpy(), out_idx.cpu().numpy()
        same((xyz[0:30], idx[0:30]), want[0], what)
        same((xyz[60:90], idx[60:90]), want[2], what)
        assert (xyz[30:60] == -77.0).all() and (idx[30:60] == -77).all(), what
    # the assembly: the same skip, and a zero centre for the skipped cloud
    dsm = torch.from_numpy(np.concatenate([want[0][0], dem[30:60], want[2][0]])).to(DEV)
    for value_row0, value_len in ((70, 30), (30, 31), (-1, 30)):
        m = torch.tensor([[0, value_row0, 60], [30, value_len, 30]], dtype=torch.int32).to(DEV)
        out = torch.full((90, 6), -77.0, device=DEV)
        centre = torch.full((3, 3), -77.0, device=DEV)
        rc = lib.scream_dsm_dem_assemble(dsm.data_ptr(), td.data_ptr(), m[0].data_ptr(), m[1].data_ptr(), 3, 30, 90, out.data_ptr(),
                                         centre.data_ptr(), stream)
        assert rc == 0
        out, centre = out.cpu().numpy(), centre.cpu().numpy()
        for c, (a, b) in ((0, (0, 30)), (2, (60, 90))):
            rows, mid = DR.centre_ref(dsm[a:b].cpu().numpy(), dem[a:b])
            assert np.array_equal(bits(out[a:b]), bits(rows)) and np.array_equal(bits(centre[c]), bits(mid[0]))
        assert (out[30:60] == -77.0).all() and (centre[1] == 0.0).all()


def test_a_dirty_workspace_changes_nothing():
    """The call zeroes the grid's counters itself (csrc/cell_grid.h) and reads nothing else of the workspace before writing it:
    a workspace full of 0xFF and one full of 0x00 give the same bits, those of the reference.  Two clouds of 300 and 70 patch
    rows (two blocks and a part of one) and 130 and 5 ground rows."""
    lib = _lib.load()
    rng = np.random.default_rng(17)
    patch = rng.uniform(0, 6, size=(370, 3)).astype(np.float32)
    dem = rng.uniform(-2, 8, size=(135, 3)).astype(np.float32)  # about half of the ground points lie beyond the patch's reach
    want = [DR.dsm_ref(patch[:300], dem[:130]), DR.dsm_ref(patch[300:], dem[130:])]
    assert all((w[1] >= 0).any() and (w[1] < 0).any() for w in want)
    tp, td = torch.from_numpy(patch).to(DEV), torch.from_numpy(dem).to(DEV)
    m = torch.tensor([[0, 300], [300, 70], [0, 130], [130, 5]], dtype=torch.int32).to(DEV)
    need = lib.scream_dsm_workspace_bytes(370, 2, 300)
    assert need > 0
    got = []
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, device=DEV, dtype=torch.uint8)
        out_xyz = torch.full((135, 3), -77.0, device=DEV)
        out_idx = torch.full((135,), -77, device=DEV, dtype=torch.int32)
        rc = lib.scream_dsm_extract(tp.data_ptr(), m[0].data_ptr(), m[1].data_ptr(), 300, 370, td.data_ptr(), m[2].data_ptr(),
                                    m[3].data_ptr(), 130, 135, 2, C.c_float(0.8), out_xyz.data_ptr(), out_idx.data_ptr(), ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        got.append((out_xyz.cpu().numpy(), out_idx.cpu().numpy()))
    same(got[0], got[1], "0xFF against 0x00")
    for xyz, idx in got:
        same((xyz[:130], idx[:130]), want[0], "cloud 0")
        same((xyz[130:], idx[130:]), want[1], "cloud 1")


def test_wrong_dtype_device_shape_or_radius_raise():
    good = torch.zeros(5, 3, device=DEV)
    for bad in (torch.zeros(5, 3, device=DEV, dtype=torch.float64), torch.zeros(5, 3), torch.zeros(5, 2, device=DEV),
                torch.zeros(15, device=DEV)):
        with pytest.raises(ScreamHipError):
            extract_dsm(bad, good)
        with pytest.raises(ScreamHipError):
            extract_dsm(good, bad)
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ScreamHipError):
            extract_dsm(good, good, radius)
    with pytest.raises(ScreamHipError):
        extract_dsm_batch([good, good], [good])
    with pytest.raises(ScreamHipError):
        ops.dsm_extract_packed(good, *(torch.tensor([[0], [5]], dtype=torch.int32).to(DEV)), 5, good,
                               *(torch.tensor([[0], [5]], dtype=torch.int32).to(DEV)), 5, float("nan"))


# ---- 10. the pipeline

def host_chain(xyz, cls):
    patch = VR.ref32(xyz, 1.0)[2]
    dem = VR.ref32(xyz[cls == 1], 1.0)[2]
    return DR.centre_ref(DR.dsm_ref(patch, dem, 0.8)[0], dem)


@functools.lru_cache(maxsize=None)
def four_windows():
    out = []
    for k in range(4):
        xyz, cls = DR.seeded_tile(20 + k, 6000 + 500 * k, 30.0, offset=100.0 * k)
        out.append((xyz, cls) + host_chain(xyz, cls))
    return out


def test_make_dsm_dem_is_the_host_chain():
    xyz, cls = DR.seeded_tile(2, 40000, 60.0)
    rows, centre = host_chain(xyz, cls)
    got, c = make_dsm_dem(xyz, cls)
    assert got.dtype == torch.float32 and c.dtype == torch.float32 and got.is_cuda and tuple(c.shape) == (1, 3)
    assert tuple(got.shape) == rows.shape and rows.shape[0] > 3000
    assert np.array_equal(bits(c.cpu().numpy()), bits(centre)) and np.array_equal(bits(got.cpu().numpy()), bits(rows))
    got_t, c_t = make_dsm_dem(torch.from_numpy(xyz).to(DEV), torch.from_numpy(cls))  # tensors, on either device
    assert torch.equal(got_t, got) and torch.equal(c_t, c)
    # an origin taken off in float64 before the cast: the same tile at UTM-sized coordinates gives the same sample
    far = xyz.astype(np.float64) + np.array([4.0e5, 3.0e6, 0.0])
    got_o, c_o = make_dsm_dem(far, cls, origin=np.array([4.0e5, 3.0e6, 0.0]))
    assert torch.equal(got_o, got) and torch.equal(c_o, c)


def test_make_dsm_dem_batch_is_four_single_calls():
    w = four_windows()
    rows, centres = make_dsm_dem_batch([x[0] for x in w], [x[1] for x in w])
    for k, (xyz, cls, want, centre) in enumerate(w):
        one, c = make_dsm_dem(xyz, cls)
        assert torch.equal(rows[k], one) and torch.equal(centres[k], c)
        assert np.array_equal(bits(one.cpu().numpy()), bits(want)) and np.array_equal(bits(c.cpu().numpy()), bits(centre))


def test_split_dataset_as_patch_writes_what_open_gf_files_reads(tmp_path):
    import process_open_gf
    from models.pointnet import DEMTransformer
    from scream_amd.evaluate_open_gf import SCALE_FACTOR, OpenGFFiles, evaluate_samples
    from scream_amd.synthetic import make_state_dict
    w = four_windows()
    process_open_gf.split_dataset_as_patch([(x[0].astype(np.float64), x[1]) for x in w], "unit", True, root=str(tmp_path),
                                           windows_per_call=3)
    root = tmp_path / "OpenGF_unit"
    ds = OpenGFFiles(str(root), count=4)
    samples = [ds[i] for i in range(4)]
    for k, (s, (_, _, want, centre)) in enumerate(zip(samples, w)):
        arr = np.load(root / ("%d.npy" % (k + 1)))
        assert arr.dtype == np.float32 and np.array_equal(bits(arr), bits(want))
        assert np.array_equal(bits(np.load(root / "centers" / ("%d.npy" % (k + 1)))), bits(centre))
        assert np.array_equal(bits(s[0].numpy()), bits(want[:, :3] / np.float32(SCALE_FACTOR)))
        assert np.array_equal(bits(s[2].numpy()), bits(want[:, 3:] / np.float32(SCALE_FACTOR)))
        assert np.array_equal(np.asarray(s[3]), centre)
    net = DEMTransformer(256, 1, 1)
    net.load_state_dict(make_state_dict(6, 256, 1, 1, dem=True))
    net = net.to(DEV).eval()
    rows = evaluate_samples(net, samples[:1])
    assert rows.shape == (1, 3) and np.isfinite(rows).all()
