"""The fixed-radius search on the MI355X (csrc/radius.hip, scream_amd/overlap.py, process_3d_match.py) against the brute-force
float64 restatement of tests/radius_ref.py.  Every comparison is exact: the contract of include/scream_hip.h makes both sides
the same IEEE sequence, so counts and pairs are array_equal and there is no tolerance anywhere in this file.  Run with
`pytest -m gpu`."""
import ctypes as C
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import radius_ref as RR
import voxel_ref as VR
from scream_amd import ScreamHipError, _lib, ops
from scream_amd.overlap import (overlap_batch, prepare_3dmatch_batch, radius_count_batch, radius_pairs_batch, select_outputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)).to(DEV)


def gpu_batch(srcs, tgts, Ts, radius, K=None):
    """numpy clouds through the two public batch calls -> list of (count int32 [N], pairs int64 [n,2])."""
    s, t = [dev(a) for a in srcs], [dev(a) for a in tgts]
    counts = radius_count_batch(s, t, Ts, radius)
    pairs = radius_pairs_batch(s, t, Ts, radius, K)
    for c, p in zip(counts, pairs):
        assert c.dtype == torch.int32 and c.is_cuda and p.dtype == torch.int64 and p.is_cuda and p.dim() == 2 and p.shape[1] == 2
    return [(c.cpu().numpy(), p.cpu().numpy()) for c, p in zip(counts, pairs)]


def same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), what
    assert got[1].shape == want[1].shape and got[1].dtype == np.int64 and np.array_equal(got[1], want[1]), what


def check_batch(srcs, tgts, Ts, radius, K=None, what=""):
    got = gpu_batch(srcs, tgts, Ts, radius, K)
    want = [RR.radius_ref(s, t, T, radius, K) for s, t, T in zip(srcs, tgts, Ts)]
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, "%s pair %d (%d source, %d target points, radius %r, K %r)" % (what, i, len(srcs[i]), len(tgts[i]), radius, K))
    return want


# ---- 1. seeded rooms

@functools.lru_cache(maxsize=None)
def room(kind):
    return RR.room_pair(7, 4096, 4096, kind)


@pytest.mark.parametrize("kind", ["identity", "rigid", "far"])
def test_seeded_room_at_both_radii(kind):
    src, tgt, T = room(kind)
    for radius in (0.03, 0.1):
        count, pairs = check_batch([src], [tgt], [T], radius, what=kind)[0]
        assert (count > 0).sum() > 800 and pairs.shape[0] == count.sum()  # 2 048 points at N(0, 0.02) of a target: 48 % within 0.03
    if kind == "far":
        assert np.abs(src).max() > 900


# ---- 2. at the radius, on the cell borders

def test_lattice_at_the_radius_through_four_shifts():
    clouds = [RR.lattice_pair(k) for k in range(4)]
    srcs, tgts, Ts = ([c[i] for c in clouds] for i in range(3))
    at = check_batch(srcs, tgts, Ts, RR.LATTICE_RADIUS, what="at 5/8")
    above = check_batch(srcs, tgts, Ts, float(np.nextafter(RR.LATTICE_RADIUS, 1.0)), what="one step above 5/8")
    for (c0, _), (c1, _) in zip(at, above):
        assert (c1 >= c0).all() and int((c1 - c0).sum()) > 10000  # the pairs exactly at the radius: excluded, then included
    assert all(np.array_equal(at[0][0], a[0]) for a in at[1:])  # the shift moves the grid's borders, not the answer


# ---- 3. outside the target's bounding box

def test_sources_beyond_every_face_edge_and_corner():
    for radius in (0.05, 0.3):
        src, tgt, T, within, beyond = RR.outside_pair(radius)
        count, _ = check_batch([src], [tgt], [T], radius, what="outside")[0]
        assert (count[within] >= 1).all() and (count[beyond] == 0).all()


def test_a_source_entirely_out_of_reach():
    src, tgt, T = room("identity")
    far_T = T.copy()
    far_T[:3, 3] = [50.0, -70.0, 8.0]
    count, pairs = check_batch([src[:1000]], [tgt], [far_T], 0.03)[0]
    assert not count.any() and pairs.shape == (0, 2)
    masks, n = overlap_batch([dev(src[:1000])], [dev(tgt)], [far_T])
    assert n == [0] and masks[0].dtype == torch.bool and not bool(masks[0].any())


# ---- 4. degenerate extents, empty clouds

def test_degenerate_targets_and_empty_clouds():
    cases = RR.degenerate_pairs()
    want = check_batch([c[1] for c in cases], [c[2] for c in cases], [np.eye(4)] * len(cases), 0.03, what="degenerate")
    by = {c[0]: w for c, w in zip(cases, want)}
    assert (by["coincident"][0] % 300 == 0).all() and by["coincident"][0].max() == 300 and by["coincident"][0].min() == 0
    assert by["line"][0].max() > 0 and by["plane"][0].max() > 0 and by["one target"][0].max() == 1 and by["one source"][0][0] > 10
    assert by["one and one"][0].tolist() == [1] and by["one and one"][1].tolist() == [[0, 0]]
    assert by["no target"][0].tolist() == [0] * 200 and by["no source"][0].shape == (0,) and by["no source"][1].shape == (0, 2)
    for name, s, t in cases:  # and each alone: its own grid size
        check_batch([s], [t], [np.eye(4)], 0.03, K=2, what=name)
    assert radius_count_batch([], [], [], 0.03) == [] and radius_pairs_batch([], [], [], 0.03) == [] and overlap_batch([], [], []) == ([], [])


# ---- 5. cells larger than the radius

def test_two_hundred_metres_at_three_centimetres():
    src, tgt, T = RR.room_pair(8, 4096, 4096, "rigid", size=200.0)
    count, _ = check_batch([src], [tgt], [T], 0.03, what="200 m")[0]
    assert (count > 0).sum() > 800


def test_every_point_neighbours_every_point():
    rng = np.random.default_rng(9)
    src, tgt = rng.uniform(0, 1, size=(512, 3)).astype(np.float32), rng.uniform(0, 1, size=(512, 3)).astype(np.float32)
    count, pairs = check_batch([src], [tgt], [np.eye(4)], 2.0, what="radius 2")[0]
    assert (count == 512).all() and pairs.shape == (512 * 512, 2)
    check_batch([src], [tgt], [np.eye(4)], 2.0, K=3, what="radius 2")


# ---- 6. lengths

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000]


def test_lengths_around_the_wave_and_the_block():
    srcs, tgts = [], []
    for n in LENGTHS:
        rng = np.random.default_rng(2000 + n)
        tgts.append(rng.uniform(0, 0.5, size=(n, 3)).astype(np.float32))
        srcs.append(rng.uniform(0, 0.5, size=(n, 3)).astype(np.float32))
    Ts = [np.eye(4)] * len(LENGTHS)
    want = check_batch(srcs, tgts, Ts, 0.06, what="lengths")
    check_batch(srcs, tgts[::-1], Ts, 0.06, what="lengths crossed")  # every source length against another target length
    assert want[-1][0].sum() > 1000


# ---- 7. batches

@functools.lru_cache(maxsize=None)
def eight_pairs():
    out = []
    for k, (n, m, kind) in enumerate([(700, 900, "rigid"), (1, 300, "identity"), (1300, 40, "far"), (300, 300, "rigid"), (65, 2000, "identity"),
                                      (2000, 65, "rigid"), (512, 511, "far"), (257, 1025, "rigid")]):
        out.append(RR.room_pair(60 + k, n, m, kind, size=1.0 + 0.5 * k))
    return out


def test_eight_pairs_in_one_call_are_the_eight_single_calls():
    pairs = eight_pairs()
    srcs, tgts, Ts = ([p[i] for p in pairs] for i in range(3))
    for K in (None, 2):
        check_batch(srcs, tgts, Ts, 0.05, K, what="eight")
        first = gpu_batch(srcs, tgts, Ts, 0.05, K)
        again = gpu_batch(srcs, tgts, Ts, 0.05, K)
        for i in range(8):
            single = gpu_batch([srcs[i]], [tgts[i]], [Ts[i]], 0.05, K)[0]
            same(again[i], first[i], "repeat %d" % i)
            same(single, first[i], "single %d" % i)
    # a pair's result does not change when its neighbours in the call do
    other = [RR.room_pair(90 + k, 400 + 37 * k, 3000 - 300 * k, "rigid") for k in range(8)]
    for i in (0, 3, 7):
        s2, t2, T2 = [o[0] for o in other], [o[1] for o in other], [o[2] for o in other]
        s2[i], t2[i], T2[i] = srcs[i], tgts[i], Ts[i]
        same(gpu_batch(s2, t2, T2, 0.05)[i], first_none(i), "pair %d among other pairs" % i)


def first_none(i):
    s, t, T = eight_pairs()[i]
    return RR.radius_ref(s, t, T, 0.05)


# ---- 8. K, and the reference's own entry point

def test_K_through_the_batch_call_and_get_correspondences():
    import utils
    src, tgt, T = RR.room_pair(11, 1500, 1500, "rigid")
    for K in (1, 3, None):
        count, want = RR.radius_ref(src, tgt, T, 0.05, K)
        got = radius_pairs_batch([dev(src)], [dev(tgt)], [T], 0.05, K)[0]
        assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
        i, j = want[:, 0], want[:, 1]
        assert (np.diff(i) >= 0).all() and np.array_equal(np.bincount(i, minlength=1500), np.minimum(count, K if K else count.max()))
        for a in ((src, tgt, T), (torch.from_numpy(src), dev(tgt), torch.from_numpy(T))):  # arrays, tensors on either device
            corr = utils.get_correspondences(a[0], a[1], a[2], 0.05, K)
            assert isinstance(corr, torch.Tensor) and corr.dtype == torch.int64 and np.array_equal(corr.cpu().numpy(), want)
    assert count.max() > 3  # K = 3 did cut


# ---- 9. refusals

def raw_count(radius, n_pairs, count, ws_bytes=None, max_t=4, t_rows=4):
    lib = _lib.load()
    src, tgt = torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, device=DEV)
    meta = torch.tensor([[0], [4]], dtype=torch.int32).to(DEV)
    T = torch.eye(4, dtype=torch.float64).reshape(1, 16).to(DEV)
    need = lib.scream_radius_workspace_bytes(4, 1, 4)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    return lib.scream_radius_count(src.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), 4, 4, tgt.data_ptr(), meta[0].data_ptr(),
                                   meta[1].data_ptr(), max_t, t_rows, T.data_ptr(), n_pairs, C.c_double(radius), count.data_ptr(),
                                   ws.data_ptr(), need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)


def test_refusals_return_their_status_and_launch_nothing():
    lib = _lib.load()
    count = torch.full((4,), -77, device=DEV, dtype=torch.int32)
    for radius in (0.0, -0.03, float("inf"), float("-inf"), float("nan")):
        assert raw_count(radius, 1, count) == -1, radius  # SCREAM_EINVAL
    need = lib.scream_radius_workspace_bytes(4, 1, 4)
    assert need > 0 and raw_count(0.03, 1, count, ws_bytes=need - 1) == -1 and raw_count(0.03, 1, count, ws_bytes=0) == -1
    assert raw_count(0.03, 1, count, max_t=5) == -1 and raw_count(0.03, 1, count, t_rows=-1) == -1 and raw_count(0.03, -1, count) == -1
    assert raw_count(0.03, 65536, count) == -2  # SCREAM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (count == -77).all()
    assert raw_count(0.03, 0, count) == 0
    torch.cuda.synchronize()
    assert (count == -77).all()
    assert raw_count(0.03, 1, count) == 0  # the same arguments with nothing to refuse: four coincident points
    torch.cuda.synchronize()
    assert (count == 4).all()
    assert lib.scream_radius_workspace_bytes(-1, 1, 0) == -1 and lib.scream_radius_workspace_bytes(4, 1, 5) == -1
    assert lib.scream_radius_workspace_bytes(4, -1, 4) == -1


def test_the_fill_call_refuses_the_same_and_the_next_valid_call_is_correct():
    lib = _lib.load()
    src, tgt, T = RR.room_pair(12, 300, 300, "rigid")
    ts, tt = dev(src), dev(tgt)
    meta = torch.tensor([[0], [300]], dtype=torch.int32).to(DEV)
    Td = torch.from_numpy(T).reshape(1, 4, 4).to(DEV)
    count, ws = ops.radius_count_packed(ts, meta[0], meta[1], 300, tt, meta[0], meta[1], 300, Td, 0.05)
    offset = torch.zeros(301, device=DEV, dtype=torch.int64)
    offset[1:] = torch.cumsum(count.to(torch.int64), dim=0)
    total = int(offset[-1])
    pair_j = torch.full((total,), -77, device=DEV, dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda radius, n_pairs, ws_bytes: lib.scream_radius_pairs(
        ts.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), 300, 300, tt.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), 300, 300,
        Td.data_ptr(), n_pairs, C.c_double(radius), ws.data_ptr(), ws_bytes, 0, offset.data_ptr(), pair_j.data_ptr(), stream)
    assert call(float("nan"), 1, ws.numel()) == -1 and call(-1.0, 1, ws.numel()) == -1
    assert call(0.05, 1, ws.numel() - 1) == -1 and call(0.05, 65536, ws.numel()) == -2
    torch.cuda.synchronize()
    assert (pair_j == -77).all()
    assert call(0.05, 1, ws.numel()) == 0
    want_count, want = RR.radius_ref(src, tgt, T, 0.05)
    assert np.array_equal(count.cpu().numpy(), want_count) and np.array_equal(pair_j.cpu().numpy().astype(np.int64), want[:, 1])
    with pytest.raises(ScreamHipError):
        ops.radius_count_packed(ts, meta[0], meta[1], 300, tt, meta[0], meta[1], 300, Td, float("nan"))


def test_a_pair_whose_rows_leave_the_arrays_is_skipped_on_the_device():
    lib = _lib.load()
    rng = np.random.default_rng(13)
    src = rng.uniform(0, 0.4, size=(90, 3)).astype(np.float32)
    tgt = rng.uniform(0, 0.4, size=(300, 3)).astype(np.float32)
    want = [RR.radius_ref(src[0:30], tgt[0:100], np.eye(4), 0.06)[0], None, RR.radius_ref(src[60:90], tgt[200:300], np.eye(4), 0.06)[0]]
    ts, tt = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    T = torch.eye(4, dtype=torch.float64).reshape(1, 16).repeat(3, 1).contiguous().to(DEV)
    good = [[0, 30, 60], [30, 30, 30], [0, 100, 200], [100, 100, 100]]
    for what, row, value in (("source rows past the array", 0, 70), ("source longer than max_s_len", 1, 31), ("negative source row", 0, -1),
                             ("target rows past the array", 2, 250), ("target longer than max_t_len", 3, 101), ("negative target length", 3, -5)):
        meta = [list(r) for r in good]
        meta[row][1] = value
        m = torch.tensor(meta, dtype=torch.int32).to(DEV)
        count = torch.full((90,), -77, device=DEV, dtype=torch.int32)
        ws = torch.empty(lib.scream_radius_workspace_bytes(300, 3, 100), device=DEV, dtype=torch.uint8)
        rc = lib.scream_radius_count(ts.data_ptr(), m[0].data_ptr(), m[1].data_ptr(), 30, 90, tt.data_ptr(), m[2].data_ptr(), m[3].data_ptr(),
                                     100, 300, T.data_ptr(), 3, C.c_double(0.06), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, what
        c = count.cpu().numpy()
        assert np.array_equal(c[0:30], want[0]) and np.array_equal(c[60:90], want[2]) and (c[30:60] == -77).all(), what


def test_a_dirty_workspace_changes_nothing():
    """The count call zeroes the grid's counters itself (csrc/cell_grid.h) and reads nothing else of the workspace before writing
    it: a workspace full of 0xFF and one full of 0x00 give the same counts and, through the fill launch, the same pairs -- those
    of the reference.  Two pairs of 300 and 70 target rows (two blocks and a part of one) and 130 and 5 source rows."""
    lib = _lib.load()
    rng = np.random.default_rng(19)
    tgt = rng.uniform(0, 0.4, size=(370, 3)).astype(np.float32)
    src = rng.uniform(0, 0.4, size=(135, 3)).astype(np.float32)
    refs = [RR.radius_ref(src[:130], tgt[:300], np.eye(4), 0.06), RR.radius_ref(src[130:], tgt[300:], np.eye(4), 0.06)]
    want_count = np.concatenate([r[0] for r in refs])
    want_j = np.concatenate([r[1][:, 1] for r in refs])
    assert all((r[0] > 0).any() and (r[0] == 0).any() for r in refs)
    ts, tt = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    T = torch.eye(4, dtype=torch.float64).reshape(1, 16).repeat(2, 1).contiguous().to(DEV)
    m = torch.tensor([[0, 130], [130, 5], [0, 300], [300, 70]], dtype=torch.int32).to(DEV)
    need = lib.scream_radius_workspace_bytes(370, 2, 300)
    assert need > 0
    stream = torch.cuda.current_stream().cuda_stream
    got = []
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, device=DEV, dtype=torch.uint8)
        count = torch.full((135,), -77, device=DEV, dtype=torch.int32)
        head = (ts.data_ptr(), m[0].data_ptr(), m[1].data_ptr(), 130, 135, tt.data_ptr(), m[2].data_ptr(), m[3].data_ptr(), 300, 370,
                T.data_ptr(), 2, C.c_double(0.06))
        assert lib.scream_radius_count(*head, count.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
        offset = torch.zeros(136, device=DEV, dtype=torch.int64)
        torch.cumsum(count.to(torch.int64), dim=0, out=offset[1:])
        pair_j = torch.full((135 * 300,), -77, device=DEV, dtype=torch.int32)  # room for whatever the counts say
        assert lib.scream_radius_pairs(*head, ws.data_ptr(), ws.numel(), 0, offset.data_ptr(), pair_j.data_ptr(), stream) == 0
        got.append((count.cpu().numpy(), pair_j[:int(offset[-1])].cpu().numpy().astype(np.int64)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    for count, pair_j in got:
        assert np.array_equal(count, want_count) and np.array_equal(pair_j, want_j)


def test_targets_of_257_rows_on_a_plane_and_on_a_line():
    """A grid of n = (k, k, 1) and one of n = (k, 1, 1) cells, two blocks of target rows each (256 + 1); the sources lie at N(0, 0.02)
    of target points, on both sides of the 0.03 radius."""
    rng = np.random.default_rng(51)
    line = np.stack([rng.uniform(0, 2, size=257), np.full(257, 0.5), np.full(257, -0.5)], axis=1).astype(np.float32)
    plane = np.stack([rng.uniform(0, 2, size=257), rng.uniform(0, 2, size=257), np.full(257, 1.0)], axis=1).astype(np.float32)
    tgts = [plane, line]
    srcs = [(t[rng.integers(0, 257, size=200)] + rng.normal(0, 0.02, size=(200, 3))).astype(np.float32) for t in tgts]
    for want in check_batch(srcs, tgts, [np.eye(4)] * 2, 0.03, what="257 rows"):
        assert (want[0] > 0).sum() > 50 and (want[0] == 0).sum() > 50
    for s, t in zip(srcs, tgts):  # and each alone
        check_batch([s], [t], [np.eye(4)], 0.03, what="257 rows alone")


def test_wrong_dtype_device_shape_or_radius_raise():
    good = torch.zeros(5, 3, device=DEV)
    eye = [np.eye(4)]
    for bad in (torch.zeros(5, 3, device=DEV, dtype=torch.float64), torch.zeros(5, 3), torch.zeros(5, 2, device=DEV), torch.zeros(15, device=DEV)):
        with pytest.raises(ScreamHipError):
            radius_count_batch([bad], [good], eye, 0.03)
        with pytest.raises(ScreamHipError):
            radius_pairs_batch([good], [bad], eye, 0.03)
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ScreamHipError):
            radius_count_batch([good], [good], eye, radius)
    for Ts in ([], [np.eye(3)], [np.eye(4), np.eye(4)]):
        with pytest.raises(ScreamHipError):
            radius_count_batch([good], [good], Ts, 0.03)
    with pytest.raises(ScreamHipError):
        radius_pairs_batch([good], [good], eye, 0.03, K=0)
    with pytest.raises(ScreamHipError):
        prepare_3dmatch_batch([torch.zeros(0, 3, device=DEV)], [good], [np.eye(3)], [np.zeros(3)])


# ---- 10. the pipeline

def overlap_pair(seed, ratio, n=3000):
    """A raw pair whose overlap ratio is about `ratio`: that share of the source points lies within 5 mm of a target point, the
    rest half a metre off the walls.  rot / trans as the info pickles hold them (float64)."""
    rng = np.random.default_rng(seed)
    world_t = RR.room_points(rng, 4000)
    k = int(round(ratio * n))
    on = world_t[rng.permutation(4000)[:k]] + rng.normal(0, 0.003, size=(k, 3))
    off = rng.uniform(0.5, 2.5, size=(n - k, 3))
    world_s = np.concatenate([on, off])[rng.permutation(n)]
    R, t = RR.rotation(rng), rng.uniform(-1.5, 1.5, size=(3, 1))
    return ((world_s - t.T) @ R).astype(np.float32), world_t.astype(np.float32), R, t


@functools.lru_cache(maxsize=None)
def three_pairs():
    out = []
    for seed, ratio in ((21, 0.05), (22, 0.2), (23, 0.6)):
        src, tgt, R, t = overlap_pair(seed, ratio)
        T = np.concatenate([np.concatenate([R.astype(np.float32), t.astype(np.float32)], axis=1), np.array([[0, 0, 0, 1]])], axis=0)
        count, _ = RR.radius_ref(src, tgt, T, 0.03)
        out.append(dict(src=src, tgt=tgt, rot=R, trans=t, T=T, mask=count > 0))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_prepared(d, w):
    n_overlap = int(w["mask"].sum())
    assert d["n_overlap"] == n_overlap and d["n_src"] == 3000 and type(d["n_overlap"]) is int
    assert d["overlap_ratio"] == n_overlap / 3000
    assert isinstance(d["T"], np.ndarray) and d["T"].dtype == np.float64 and np.array_equal(d["T"].view(np.uint64), w["T"].view(np.uint64))
    for key, cloud in (("src", w["src"]), ("tgt", w["tgt"]), ("src_zero", w["src"][~w["mask"]])):
        assert d[key].is_cuda and d[key].dtype == torch.float32
        assert np.array_equal(bits(d[key].cpu().numpy()), bits(VR.ref32(cloud, 0.0625)[2])), key


def test_prepare_3dmatch_batch_is_the_host_chain():
    want = three_pairs()
    got = prepare_3dmatch_batch([dev(w["src"]) for w in want], [dev(w["tgt"]) for w in want], [w["rot"] for w in want],
                                [w["trans"] for w in want])
    assert len(got) == 3
    for d, w in zip(got, want):
        check_prepared(d, w)
    ratios = [d["overlap_ratio"] for d in got]
    assert ratios[0] < 0.1 < ratios[1] < 0.3 < ratios[2], ratios
    masks, n = overlap_batch([dev(w["src"]) for w in want], [dev(w["tgt"]) for w in want], [w["T"] for w in want])
    for m, k, w in zip(masks, n, want):
        assert np.array_equal(m.cpu().numpy(), w["mask"]) and k == int(w["mask"].sum())
    route = lambda kind: [select_outputs(kind, d["n_overlap"], d["n_src"]) for d in got]
    lo, zero = ("3DLoMatch_test", "src"), ("3DZeroMatch_test", "src_zero")
    assert route("test_3dlomatch") == [[zero], [lo, zero], [lo]]
    assert route("test_3dmatch") == [[], [], [("3DMatch_test", "src")]]
    assert [len(r) for r in route("train")] == [2, 2, 1]
    # tensors for rot / trans, trans as [3], one pair alone: the same
    one = prepare_3dmatch_batch([dev(want[1]["src"])], [dev(want[1]["tgt"])], [torch.from_numpy(want[1]["rot"])], [want[1]["trans"].reshape(3)])
    check_prepared(one[0], want[1])


def test_save_lo_and_zero_match_end_to_end(tmp_path):
    import process_3d_match as P
    from scream_amd.data import PairFileDataset
    want = three_pairs()
    scene = "7-scenes-redkitchen"
    os.makedirs(tmp_path / "indoor" / "test" / scene)
    os.makedirs(tmp_path / "gt" / scene)
    info = dict(rot=[], trans=[], src=[], tgt=[])
    rng = np.random.default_rng(5)
    cov = {}
    with open(tmp_path / "gt" / scene / "gt.info", "w") as f:
        for k, w in enumerate(want):
            s, t = "test/%s/cloud_bin_%d.pth" % (scene, 10 + k), "test/%s/cloud_bin_%d.pth" % (scene, k)
            torch.save(w["src"], str(tmp_path / "indoor" / s))
            torch.save(w["tgt"], str(tmp_path / "indoor" / t))
            info["src"].append(s), info["tgt"].append(t), info["rot"].append(w["rot"]), info["trans"].append(w["trans"])
            cov[k] = rng.uniform(1, 2, size=(6, 6)).astype(np.float32)
            f.write("%d\t %d\t 60\n" % (k, 10 + k) + "".join(" ".join("%.9g" % v for v in row) + "\n" for row in cov[k]))
    with open(tmp_path / "3DLoMatch.pkl", "wb") as f:
        pickle.dump(info, f)
    ds = P.PredatorPairs(str(tmp_path / "indoor"), str(tmp_path / "3DLoMatch.pkl"), str(tmp_path / "gt"))
    assert len(ds) == 3 and ds[1][6] == scene and ds[1][4].tolist() == [1, 11] and ds[1][0].is_cuda
    out = str(tmp_path / "out")
    assert P.save_lo_and_zero_match(ds, out, pairs_per_call=2) == {"3DLoMatch_test": 2, "3DZeroMatch_test": 2}
    assert P.save_lo_and_zero_match_info(ds, out, pairs_per_call=2) == {"3DLoMatch_test": 2, "3DZeroMatch_test": 2}
    for folder, members, which in (("3DLoMatch_test", (1, 2), "src"), ("3DZeroMatch_test", (0, 1), "src_zero")):
        path = os.path.join(out, folder)
        assert sorted(os.listdir(path)) == sorted(["info"] + ["%s%d.npy" % (n, k) for n in ("src", "tgt", "T") for k in range(2)])
        assert open(os.path.join(path, "info", "scene_names.txt")).read() == (scene + "\n") * 2
        loaded = PairFileDataset(path)
        assert len(loaded) == 2
        for k, p in enumerate(members):
            w = want[p]
            cloud = w["src"] if which == "src" else w["src"][~w["mask"]]
            src, tgt, T = (np.load(os.path.join(path, "%s%d.npy" % (n, k))) for n in ("src", "tgt", "T"))
            assert src.dtype == np.float64 and tgt.dtype == np.float64 and T.dtype == np.float64
            assert np.array_equal(src, VR.ref32(cloud, 0.0625)[2].astype(np.float64))
            assert np.array_equal(tgt, VR.ref32(w["tgt"], 0.0625)[2].astype(np.float64)) and np.array_equal(T, w["T"])
            assert np.load(os.path.join(path, "info", "idx%d.npy" % k)).tolist() == [p, 10 + p]
            assert np.array_equal(np.load(os.path.join(path, "info", "covariance%d.npy" % k)), cov[p])
            item = loaded[k]
            assert tuple(item[0].shape) == src.shape and tuple(item[1].shape) == tgt.shape and item[8] == 0
            assert item[5].tolist() == [p, 10 + p] and np.array_equal(item[6].numpy(), cov[p])
