"""The host layer of the ops on lists of clouds (scream_amd/clouds.py) and the exception class every public entry point raises for
a bad input.  Nothing here needs a GPU: the checks run before anything touches the device or the library."""
import numpy as np
import pytest
import torch

from scream_amd import ScreamHipError
from scream_amd.clouds import PackedPairs, check_clouds, check_radius, pack_clouds, pose_stack
from scream_amd.dsm import extract_dsm, extract_dsm_batch, make_dsm_dem, make_dsm_dem_batch
from scream_amd.overlap import overlap_batch, prepare_3dmatch_batch, radius_count_batch, radius_pairs_batch
from scream_amd.prep import prepare_3dmatch_val, prepare_pairs
from scream_amd.rawicp import icp_raw_batch, raw_nn_batch
from scream_amd.voxel import voxel_down_sample, voxel_down_sample_batch


def cloud(n, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, size=(n, 3)).astype(np.float32))


def test_pack_clouds_with_empty_clouds_between():
    clouds = [cloud(n, n) for n in (0, 5, 0, 3)]
    rows, row0, lens = pack_clouds(clouds)
    assert row0 == [0, 0, 5, 5] and lens == [0, 5, 0, 3] and rows.shape == (8, 3) and rows.is_contiguous()
    assert torch.equal(rows[0:5], clouds[1]) and torch.equal(rows[5:8], clouds[3])
    rows, row0, lens = pack_clouds([])
    assert row0 == [] and lens == [] and rows.shape == (0, 3) and rows.dtype == torch.float32


def test_pack_clouds_pads_only_a_list_without_rows():
    rows, row0, lens = pack_clouds([cloud(0), cloud(0)], pad_device="cpu")
    assert row0 == [0, 0] and lens == [0, 0] and rows.shape == (1, 3) and not rows.any()
    assert pack_clouds([], pad_device="cpu")[0].shape == (1, 3)
    assert pack_clouds([cloud(0), cloud(2)], pad_device="cpu")[0].shape == (2, 3)


def test_packed_pairs_uploads_the_four_rows_once():
    srcs, tgts = [cloud(4, 1), cloud(0), cloud(2, 2)], [cloud(1, 3), cloud(6, 4), cloud(0)]
    pk = PackedPairs(srcs, tgts, "cpu")
    assert pk.meta.dtype == torch.int32 and pk.meta.tolist() == [[0, 4, 4], [4, 0, 2], [0, 1, 7], [1, 6, 0]]
    assert (pk.n, pk.s_rows, pk.t_rows, pk.max_s_len, pk.max_t_len) == (3, 6, 7, 4, 6)
    assert all(torch.equal(a, b) for a, b in zip(pk.split_src(pk.src), srcs)) and all(torch.equal(a, b) for a, b in zip(pk.split_tgt(pk.tgt), tgts))
    assert pk.split_src(pk.src)[0].data_ptr() != pk.src.data_ptr() and pk.split_src(pk.src, clone=False)[0].data_ptr() == pk.src.data_ptr()
    empty = PackedPairs([], [], "cpu", pad=True)
    assert empty.meta.shape == (4, 0) and empty.src.shape == (1, 3) and empty.max_s_len == 0


def test_pose_stack_gives_the_same_float64_bits_for_a_list_an_array_and_a_tensor():
    rng = np.random.default_rng(5)
    M = rng.normal(size=(3, 4, 4)) * np.pi  # float64 values that fp32 cannot hold
    want = M.view(np.uint64)
    for given in ([m for m in M], [torch.from_numpy(m.copy()) for m in M], M, torch.from_numpy(M.copy()), np.broadcast_to(M, (3, 4, 4))):
        got = pose_stack(given, 3, "cpu")
        assert got.dtype == torch.float64 and got.shape == (3, 4, 4) and got.is_contiguous()
        assert np.array_equal(got.numpy().view(np.uint64), want)
    M32 = M.astype(np.float32)  # a narrower type converts exactly
    assert np.array_equal(pose_stack(list(M32), 3, "cpu").numpy(), M32.astype(np.float64))
    t = torch.from_numpy(M.copy())
    assert pose_stack(t, 3, "cpu").data_ptr() == t.data_ptr()              # a tensor that is where it should be stays there
    own = pose_stack(t, 3, "cpu", copy=True)
    assert own.data_ptr() != t.data_ptr() and torch.equal(own, t)          # ... unless the caller will write to it
    assert pose_stack([], 0, "cpu").shape == (0, 4, 4)


def test_pose_stack_refuses_a_wrong_shape_and_a_wrong_count():
    for bad in ([np.eye(3)], [np.eye(4), np.eye(4)], [], np.zeros((1, 3, 4)), torch.zeros(2, 4, 4), np.eye(4)):
        with pytest.raises(ScreamHipError):
            pose_stack(bad, 1, "cpu")
        with pytest.raises(ValueError):
            pose_stack(bad, 1, "cpu", "poses", ValueError)


def test_check_radius_refuses_zero_negative_infinite_and_nan():
    assert check_radius(0.8) == 0.8 and check_radius(np.float32(0.03)) == float(np.float32(0.03)) and check_radius(1) == 1.0
    for bad in (0, -1, float("inf"), float("nan")):
        with pytest.raises(ScreamHipError, match="the radius"):
            check_radius(bad)
        with pytest.raises(ValueError, match="cloud 1: voxel size"):
            check_radius(bad, "cloud 1: voxel size", ValueError)


def test_check_clouds_names_the_cloud_and_picks_the_class():
    good = cloud(5)
    for bad in (torch.zeros(5, 2), torch.zeros(15), np.zeros((5, 3), np.float32)):  # the shape comes first: no device is needed
        with pytest.raises(ScreamHipError, match="patch 0"):
            check_clouds([bad, good], "patch")
        with pytest.raises(ValueError, match="cloud 0"):
            check_clouds([bad, good], "cloud", builtin_errors=True)
    with pytest.raises(ScreamHipError, match="dem 0 is on cpu"):
        check_clouds([good, torch.zeros(5, 2)], "dem", op="extract_dsm")
    with pytest.raises(ScreamHipError, match="no CPU path"):  # the device comes before the dtype, and is never a builtin error
        check_clouds([good.double()], "cloud", builtin_errors=True)
    assert check_clouds([], "cloud") is None


# The classes below are those of the code before the checks were shared: voxel_down_sample_batch and the raw-scan ICP raise
# ValueError for a wrong shape or count and TypeError for a wrong dtype; dsm, overlap and prep raise ScreamHipError for every
# bad cloud; a tensor that is not on the GPU is a ScreamHipError everywhere ("there is no CPU path").

def test_every_entry_point_keeps_its_exception_class():
    a, eye = cloud(5), [np.eye(4)]
    with pytest.raises(ValueError, match="cloud 0"):
        voxel_down_sample_batch([torch.zeros(5, 2), a], 1.0)
    with pytest.raises(ValueError):
        voxel_down_sample_batch([a, a], [1.0])
    with pytest.raises(ScreamHipError):
        voxel_down_sample(a, 1.0)
    for call in (lambda: extract_dsm(a, a), lambda: extract_dsm(torch.zeros(5, 2), a), lambda: extract_dsm_batch([a, a], [a]),
                 lambda: extract_dsm_batch([], [], radius=0.0), lambda: make_dsm_dem(a.numpy(), np.ones(5), radius=float("nan")),
                 lambda: make_dsm_dem_batch([a.numpy()], [])):
        with pytest.raises(ScreamHipError):
            call()
    for call in (lambda: radius_count_batch([a], [a], eye, 0.03), lambda: radius_pairs_batch([a], [torch.zeros(15)], eye, 0.03),
                 lambda: overlap_batch([a], [a, a], eye), lambda: radius_count_batch([], [], [], -1.0),
                 lambda: prepare_3dmatch_batch([a], [a], [np.eye(3)], [])):
        with pytest.raises(ScreamHipError):
            call()
    for call in (lambda: prepare_pairs([a], [a], eye, mode="ball", center="trans"), lambda: prepare_pairs([], [], [], mode="ball", center="trans"),
                 lambda: prepare_3dmatch_val([a], [a, a], eye)):
        with pytest.raises(ScreamHipError):
            call()
    with pytest.raises(ValueError):
        prepare_pairs([a], [a], eye, mode="cube", center="trans")
    with pytest.raises(ValueError):
        icp_raw_batch([a], [a, a], eye)
    with pytest.raises(ValueError):
        raw_nn_batch([a, a], [a], eye, 0.2)
    with pytest.raises(ScreamHipError):  # tensors on the CPU, wherever this runs
        icp_raw_batch([a], [a], np.eye(4)[None])
