"""Host side of the 3DMatch pair preparation: the float64 restatement of the radius search (tests/radius_ref.py) on cases
computed by hand, the routing rules of scream_amd.overlap.select_outputs, and the file naming of process_3d_match.py with the
prepared pairs injected.  No GPU anywhere in this file."""
import os

import numpy as np
import pytest

import radius_ref as RR
from scream_amd.overlap import select_outputs

I4 = np.eye(4)


# ---- 1. the restatement

def test_strict_at_the_radius_on_exact_coordinates():
    src = np.asarray([[1.0, 2.0, 3.0]], dtype=np.float32)
    tgt = src + np.asarray([[0.375, 0.5, 0.0], [0.0, -0.375, 0.5], [0.625, 0.0, 0.0], [0.375, 0.5, 0.125], [0.25, 0.5, 0.0]], dtype=np.float32)
    d = tgt.astype(np.float64) - src.astype(np.float64)
    assert ((d * d).sum(axis=1)[:3] == 0.625 * 0.625).all()  # 9/64 + 16/64 = 25/64, every step exact
    count, pairs = RR.radius_ref(src, tgt, I4, 0.625)
    assert count.dtype == np.int32 and count.tolist() == [1] and pairs.dtype == np.int64 and pairs.tolist() == [[0, 4]]
    up = np.nextafter(0.625, 1.0)  # one float64 step: the three points at the radius are inside
    assert up * up > 0.390625
    count, pairs = RR.radius_ref(src, tgt, I4, up)
    assert count.tolist() == [4] and pairs.tolist() == [[0, 4], [0, 0], [0, 1], [0, 2]]
    assert RR.radius_ref(src, tgt, I4, np.nextafter(0.625, 0.0))[0].tolist() == [1]
    # one float64 step inside the radius along x: included at 5/8
    inside = np.asarray([[np.nextafter(np.float64(1.625), 0.0), 2.0, 3.0]])
    a = RR.transform64(np.asarray([[1.0, 2.0, 3.0]]), I4)
    assert a[0, 0] == 1.0
    T = I4.copy()
    T[0, 3] = 1.625 - inside[0, 0]  # moves the query one float64 step of 1.625 towards the point at the radius
    assert RR.radius_ref(src, tgt[2:3], T, 0.625)[0].tolist() == [1] and RR.radius_ref(src, tgt[2:3], I4, 0.625)[0].tolist() == [0]


def test_order_is_distance_then_target_row_with_duplicated_targets():
    src = np.asarray([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    tgt = np.asarray([[0.5, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0.25, 0, 0], [0, 0, -0.25], [5, 5, 5], [0.5, 0, 0]], dtype=np.float32)
    count, pairs = RR.radius_ref(src, tgt, I4, 0.6)
    assert count.tolist() == [7, 3]
    assert pairs[pairs[:, 0] == 0][:, 1].tolist() == [1, 3, 4, 5, 0, 2, 7]  # four at 0.25 by row, then the three copies at 0.5 by row
    assert pairs[pairs[:, 0] == 1][:, 1].tolist() == [0, 2, 7]
    assert (np.diff(pairs[:, 0]) >= 0).all()


def test_K_limits_the_list_and_never_the_count():
    src = np.asarray([[0, 0, 0], [1, 0, 0], [9, 9, 9]], dtype=np.float32)
    tgt = np.asarray([[0.5, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0, 0.25, 0]], dtype=np.float32)
    full_count, full = RR.radius_ref(src, tgt, I4, 0.6, None)
    assert full_count.tolist() == [4, 2, 0] and full.tolist() == [[0, 1], [0, 3], [0, 0], [0, 2], [1, 0], [1, 2]]
    c1, p1 = RR.radius_ref(src, tgt, I4, 0.6, 1)
    assert c1.tolist() == [4, 2, 0] and p1.tolist() == [[0, 1], [1, 0]]
    c3, p3 = RR.radius_ref(src, tgt, I4, 0.6, 3)
    assert c3.tolist() == [4, 2, 0] and p3.tolist() == [[0, 1], [0, 3], [0, 0], [1, 0], [1, 2]]
    c9, p9 = RR.radius_ref(src, tgt, I4, 0.6, 9)
    assert np.array_equal(p9, full) and np.array_equal(c9, full_count)
    ce, pe = RR.radius_ref(np.zeros((0, 3), np.float32), tgt, I4, 0.6)
    assert ce.shape == (0,) and pe.shape == (0, 2)
    ce, pe = RR.radius_ref(src, np.zeros((0, 3), np.float32), I4, 0.6)
    assert ce.tolist() == [0, 0, 0] and pe.shape == (0, 2)


def test_a_translation_of_a_thousand_needs_float64():
    """The source of a "far" pair is stored at coordinates of about 1000, where fp32 has a spacing of 6e-5: a transform carried
    out in fp32 moves points by that much and classifies those near the radius differently.  The float64 transform of the
    contract stays within 1e-12 of the exact one."""
    src, tgt, T = RR.room_pair(3, 4096, 4096, "far")
    assert np.abs(src).max() > 900 and np.abs(T[:3, 3]).min() > 900
    count, pairs = RR.radius_ref(src, tgt, T, 0.03)
    assert count.sum() == pairs.shape[0] > 1000
    differs = int((RR.count_fp32(src, tgt, T, 0.03) != count).sum())
    print("rows whose fp32 count differs: %d of %d" % (differs, count.shape[0]))
    assert differs > 0
    # the float64 transform itself loses nothing that matters: a_k is within 1e-12 of the exact product
    a = RR.transform64(src, T)
    exact = (T[:3, :3].astype(np.longdouble) @ src.astype(np.longdouble).T).T + T[:3, 3].astype(np.longdouble)
    assert np.abs(a - exact).max() < 1e-12


def test_seeded_pairs_have_neighbours_on_both_sides_of_the_radius():
    for kind in ("identity", "rigid", "far"):
        src, tgt, T = RR.room_pair(1, 1024, 1024, kind)
        c3, _ = RR.radius_ref(src, tgt, T, 0.03)
        c10, _ = RR.radius_ref(src, tgt, T, 0.1)
        assert 100 < (c3 > 0).sum() < 600 and (c10 >= c3).all() and (c10 > c3).sum() > 100, kind


def test_lattice_and_outside_fixtures_are_what_they_claim():
    src, tgt, T = RR.lattice_pair(0)
    count, _ = RR.radius_ref(src, tgt, T, RR.LATTICE_RADIUS)
    more, _ = RR.radius_ref(src, tgt, T, np.nextafter(RR.LATTICE_RADIUS, 1.0))
    assert (more >= count).all() and int((more - count).sum()) > 10000  # pairs exactly at the radius
    src, tgt, T, within, beyond = RR.outside_pair(0.05)
    count, _ = RR.radius_ref(src, tgt, T, 0.05)
    assert (count[within] >= 1).all() and (count[beyond] == 0).all()
    assert ((src < 0) | (src > 1)).any(axis=1).all()  # every query lies outside the target's box


# ---- 2. select_outputs

@pytest.mark.parametrize("n_overlap,n_src,train,test,lo", [
    (0, 1000, 2, 0, ["zero"]),
    (99, 1000, 2, 0, ["zero"]),
    (100, 1000, 2, 0, ["zero"]),           # 0.1 is not > 0.1
    (101, 1000, 2, 0, ["lo", "zero"]),
    (299, 1000, 2, 0, ["lo", "zero"]),
    (300, 1000, 2, 0, ["lo", "zero"]),     # 0.3 is <= 0.3 and not > 0.3
    (301, 1000, 1, 1, ["lo"]),
    (1000, 1000, 1, 1, ["lo"]),
    (3, 10, 2, 0, ["lo", "zero"]),         # 3 / 10 == 0.3 as Python divides
    (1, 10, 2, 0, ["zero"]),
])
def test_select_outputs_at_the_thresholds(n_overlap, n_src, train, test, lo):
    for kind, folder in (("train", "3DMatch_train"), ("val", "3DMatch_val")):
        assert select_outputs(kind, n_overlap, n_src) == [(folder, "src"), (folder, "src_zero")][:train]
    assert select_outputs("test_3dmatch", n_overlap, n_src) == [("3DMatch_test", "src")][:test]
    want = [{"lo": ("3DLoMatch_test", "src"), "zero": ("3DZeroMatch_test", "src_zero")}[k] for k in lo]
    assert select_outputs("test_3dlomatch", n_overlap, n_src) == want
    # the reference's own expressions
    ratio = n_overlap / n_src
    assert (("lo" in lo) == (0.1 < ratio)) and (("zero" in lo) == (ratio <= 0.3)) and ((test == 1) == (ratio > 0.3))


def test_select_outputs_refuses_what_has_no_ratio():
    with pytest.raises(ValueError):
        select_outputs("test", 1, 10)
    with pytest.raises(ValueError):
        select_outputs("train", 0, 0)


# ---- 3. the files

def prepared_pairs():
    """Five prepared pairs with ratios 0.05, 0.2, 0.3, 0.6, 0.1: distinguishable clouds, as prepare_3dmatch_batch returns them
    (fp32 clouds, float64 T) with the idx / covariance / scene that process_3d_match.prepare adds."""
    out = []
    for k, n_overlap in enumerate((50, 200, 300, 600, 100)):
        f = lambda v, n: np.full((n, 3), v + k, dtype=np.float32) + np.float32(0.1)
        T = np.eye(4)
        T[0, 3] = k + 0.5
        out.append(dict(src=f(100, 4), tgt=f(200, 5), src_zero=f(300, 3), T=T, n_overlap=n_overlap, n_src=1000, overlap_ratio=n_overlap / 1000,
                        idx=np.array([k, k + 7]), covariance=np.full((6, 6), k, dtype=np.float32), scene="scene-%d" % (k % 2)))
    return out


def folder_state(path):
    return sorted(f for f in os.listdir(path) if f.endswith(".npy"))


def check_pair_files(folder, k, d, which):
    src, tgt, T = (np.load(os.path.join(folder, "%s%d.npy" % (n, k))) for n in ("src", "tgt", "T"))
    assert src.dtype == np.float64 and tgt.dtype == np.float64 and T.dtype == np.float64 and T.shape == (4, 4)
    assert np.array_equal(src, d[which].astype(np.float64)) and np.array_equal(tgt, d["tgt"].astype(np.float64)) and np.array_equal(T, d["T"])
    assert np.array_equal(src.astype(np.float32).view(np.uint32), d[which].view(np.uint32))  # float64 arrays holding the fp32 values


def test_save_train_and_val_write_the_zero_overlap_pair_behind_the_full_one(tmp_path):
    import process_3d_match as P
    pairs = prepared_pairs()
    for fn, folder in ((P.save_train, "3DMatch_train"), (P.save_val, "3DMatch_val")):
        counters = fn(out=str(tmp_path), prepared=pairs)
        assert counters == {folder: 9}  # five pairs, four of them with ratio <= 0.3
        path = str(tmp_path / folder)
        assert folder_state(path) == sorted("%s%d.npy" % (n, k) for n in ("src", "tgt", "T") for k in range(9))
        order = [(0, "src"), (0, "src_zero"), (1, "src"), (1, "src_zero"), (2, "src"), (2, "src_zero"), (3, "src"), (4, "src"), (4, "src_zero")]
        for k, (p, which) in enumerate(order):
            check_pair_files(path, k, pairs[p], which)
        assert not os.path.exists(os.path.join(path, "info"))


def test_save_test_3dmatch_keeps_the_pairs_above_point_three(tmp_path):
    import process_3d_match as P
    pairs = prepared_pairs()
    assert P.save_test_3DMatch(out=str(tmp_path), prepared=pairs) == {"3DMatch_test": 1}
    path = str(tmp_path / "3DMatch_test")
    assert folder_state(path) == ["T0.npy", "src0.npy", "tgt0.npy"]
    check_pair_files(path, 0, pairs[3], "src")
    assert P.save_test_3DMatch_info(out=str(tmp_path), prepared=pairs) == {"3DMatch_test": 1}
    assert open(os.path.join(path, "info", "scene_names.txt")).read() == "scene-1\n"
    assert np.load(os.path.join(path, "info", "idx0.npy")).tolist() == [3, 10]
    assert np.array_equal(np.load(os.path.join(path, "info", "covariance0.npy")), pairs[3]["covariance"])


def test_save_lo_and_zero_match_count_separately(tmp_path):
    import process_3d_match as P
    pairs = prepared_pairs()
    assert P.save_lo_and_zero_match(out=str(tmp_path), prepared=pairs) == {"3DLoMatch_test": 3, "3DZeroMatch_test": 4}
    lo, zero = str(tmp_path / "3DLoMatch_test"), str(tmp_path / "3DZeroMatch_test")
    for k, p in enumerate((1, 2, 3)):
        check_pair_files(lo, k, pairs[p], "src")
    for k, p in enumerate((0, 1, 2, 4)):
        check_pair_files(zero, k, pairs[p], "src_zero")
    assert len(folder_state(lo)) == 9 and len(folder_state(zero)) == 12
    assert P.save_lo_and_zero_match_info(out=str(tmp_path), prepared=pairs) == {"3DLoMatch_test": 3, "3DZeroMatch_test": 4}
    assert open(os.path.join(lo, "info", "scene_names.txt")).read() == "scene-1\nscene-0\nscene-1\n"
    assert open(os.path.join(zero, "info", "scene_names.txt")).read() == "scene-0\nscene-1\nscene-0\nscene-0\n"
    assert [np.load(os.path.join(zero, "info", "idx%d.npy" % k)).tolist()[0] for k in range(4)] == [0, 1, 2, 4]
    assert len(folder_state(lo)) == 9 and len(folder_state(os.path.join(lo, "info"))) == 6  # the info run writes no clouds


def test_gt_info_files_are_read_by_pair(tmp_path):
    import process_3d_match as P
    rng = np.random.default_rng(0)
    blocks = {(0, 2): rng.normal(size=(6, 6)).astype(np.float32), (3, 11): rng.normal(size=(6, 6)).astype(np.float32)}
    with open(tmp_path / "gt.info", "w") as f:
        for (a, b), m in blocks.items():
            f.write("%d\t %d\t 37\n" % (a, b))
            for row in m:
                f.write(" ".join("%.9g" % v for v in row) + "\n")
    got = P.read_gt_info(str(tmp_path / "gt.info"))
    assert sorted(got) == sorted(blocks)
    for key, m in blocks.items():
        assert got[key].dtype == np.float32 and np.array_equal(got[key], m)
