"""The host side of batch preparation (scream_amd/prep.py) and the numpy restatement of its device contract (tests/prep_ref.py):
Philox against the Random123 known answer, the restatement against the existing normalize_pair, the perturbation sampler's
distribution, and the invariant of the augmented pose.  No GPU."""
import math

import numpy as np
import pytest

import prep_ref as PR
from scream_amd import _lib, synthetic
from scream_amd.data import normalize_pair
from scream_amd.prep import sample_perturbations


def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: the zero counter under the zero key; all ones; the digits of pi."""
    assert (PR.M0, PR.M1, PR.W0, PR.W1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)
    got = PR.philox4x32_10(np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32))
    assert [int(v) for v in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = PR.philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint32), np.full(2, 0xFFFFFFFF, dtype=np.uint32))
    assert [int(v) for v in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = PR.philox4x32_10(np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], dtype=np.uint32),
                          np.array([0xa4093822, 0x299f31d0], dtype=np.uint32))
    assert [int(v) for v in pi] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # vectorised over rows: row r of a batch equals the single call
    ctr = np.zeros((5, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(5)
    many = PR.philox4x32_10(ctr, np.array([7, 9], dtype=np.uint32))
    assert np.array_equal(many[3], PR.philox4x32_10(ctr[3], np.array([7, 9], dtype=np.uint32)))


def test_gauss3_depends_on_seed_sample_cloud_and_row_only():
    a = PR.gauss3(5, 2 ** 40 + 3, 1, 300)
    assert np.array_equal(a[:100], PR.gauss3(5, 2 ** 40 + 3, 1, 100))
    for other in (PR.gauss3(6, 2 ** 40 + 3, 1, 300), PR.gauss3(5, 3, 1, 300), PR.gauss3(5, 2 ** 40 + 3, 0, 300)):
        assert not np.array_equal(a, other)
    assert np.isfinite(a).all()


def _adjacent(got, want):
    """fp32 arrays equal or neighbours."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return ((got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))).all()


@pytest.mark.parametrize("mode", ["ball", "bbox"])
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_against_normalize_pair(mode, seed):
    """Identity perturbation, no noise: the contract computes what normalize_pair computes; only the order of the sums (and of
    the 3x3 products inside BLAS) differs."""
    src, tgt, T = synthetic.make_3dmatch_pair(seed)[:3]
    src_n, tgt_n, rot, trans, s, c = normalize_pair(src, tgt, T, mode)
    r = PR.prep_pair(src, tgt, T, mode=mode, center_rule=1)
    assert _adjacent(r["src_n"], src_n.numpy()) and _adjacent(r["tgt_n"], tgt_n.numpy())
    assert _adjacent(r["rot"], rot.numpy()) and _adjacent(r["trans"], trans.numpy().reshape(3))
    assert abs(r["s"] - s) <= 1e-12 * abs(s)
    # normalize_pair returns c rounded to fp32: that value is a neighbour, and the float64 c is held to the float64 value that
    # normalize_pair rounds (its own two lines)
    assert _adjacent(r["c"].astype(np.float32), c.numpy())
    reg = np.concatenate([(T[:3, :3] @ src.T + T[:3, 3:]).T, tgt], axis=0)
    want_c = reg.mean(axis=0) if mode == "ball" else (reg.min(axis=0) + reg.max(axis=0)) / 2
    assert np.all(np.abs(r["c"] - want_c) <= 1e-12 * np.abs(want_c))
    assert np.array_equal(r["T_aug"], T) and np.array_equal(r["center"], r["trans"])


def test_sample_perturbations_reproducible_and_rigid():
    P, side = sample_perturbations(64, 0.1, 12)
    P2, side2 = sample_perturbations(64, 0.1, np.random.default_rng(12))
    assert P.dtype == np.float64 and P.shape == (64, 4, 4) and side.shape == (64,)
    assert np.array_equal(P, P2) and np.array_equal(side, side2)
    P3, _ = sample_perturbations(64, 0.1, 13)
    assert not np.array_equal(P, P3)
    R = P[:, :3, :3]
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12
    assert np.array_equal(P[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (64, 4)))
    assert set(np.unique(side)) == {0, 1}
    assert not sample_perturbations(64, 0.1, 12, side="source")[1].any()
    with pytest.raises(ValueError):
        sample_perturbations(4, 0.1, 0, side="target")


def test_sample_perturbations_distribution():
    """Over n = 20 000 samples: the rotation angle is N(0, (0.1 pi / sqrt 3)^2) and every translation axis N(0, (0.1 / sqrt 3)^2).
    The angle recovered from the trace is |angle| (axis and angle flip together), so the estimate is the root mean square, whose
    standard error for a zero-mean normal is sigma / sqrt(2 n); the sides are a fair coin (standard error 0.5 / sqrt n)."""
    n = 20000
    P, side = sample_perturbations(n, 0.1, 2024)
    cos_a = np.clip((np.trace(P[:, :3, :3], axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    sig_a = 0.1 * math.pi / math.sqrt(3.0)
    rms = math.sqrt(np.mean(np.arccos(cos_a) ** 2))
    assert abs(rms - sig_a) <= 5 * sig_a / math.sqrt(2 * n), (rms, sig_a)
    sig_t = 0.1 / math.sqrt(3.0)
    for k in range(3):
        t = P[:, k, 3]
        assert abs(t.std() - sig_t) <= 5 * sig_t / math.sqrt(2 * n), (k, t.std(), sig_t)
        assert abs(t.mean()) <= 5 * sig_t / math.sqrt(n)
    assert abs(side.mean() - 0.5) <= 5 * 0.5 / math.sqrt(n)
    # the axis is uniform on the sphere: every component has mean 0 and variance 1/3 (fourth moment 1/5: se of the variance)
    R = P[:, :3, :3]
    axis = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)  # up to its sign, which the squares do not see
    assert np.all(np.abs((axis ** 2).mean(axis=0) - 1.0 / 3.0) <= 5 * math.sqrt((1.0 / 5.0 - 1.0 / 9.0) / n))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("mode", ["ball", "bbox"])
def test_augmented_pose_still_registers_the_augmented_clouds(side, mode):
    """No noise: T' a_src equals T x_src (side 0: the target did not move), moved by P' for side 1."""
    src, tgt, T = PR.raw_pair(40 + side, 700, 900)
    P = sample_perturbations(1, 0.1, 99)[0][0]
    r = PR.prep_pair(src, tgt, T, perturb=P, side=side, mode=mode, center_rule=2)
    m = (src if side == 0 else tgt).mean(axis=0)
    C = np.eye(4)
    C[:3, 3] = -m
    Pc = np.linalg.inv(C) @ P @ C  # the reference's se3_cat(se3_cat(se3_inv(center), perturb), center)
    hom = lambda M, x: x @ M[:3, :3].T + M[:3, 3]
    want = hom(T, src) if side == 0 else hom(Pc, hom(T, src))
    assert np.abs(hom(r["T_aug"], r["a_src"]) - want).max() <= 1e-12
    assert np.abs(r["a_tgt"] - (tgt if side == 0 else hom(Pc, tgt))).max() <= 1e-12
    assert np.abs(r["a_src"] - (hom(Pc, src) if side == 0 else src)).max() <= 1e-12
    # and the normalised ground truth registers the normalised clouds: rot x + trans = s (T' a - c)
    reg_n = r["src_n"].astype(np.float64) @ r["rot"].astype(np.float64).T + r["trans"].astype(np.float64)
    assert np.abs(reg_n - r["s"] * (hom(r["T_aug"], r["a_src"]) - r["c"])).max() <= 1e-5
    assert np.abs(r["center"].astype(np.float64) + r["rot"].astype(np.float64).T @ r["trans"].astype(np.float64)).max() <= 1e-6


def test_loss_restatement_against_float64_torch_and_its_seeded_inputs():
    """The seeded inputs of the GPU loss tests hold no element with |pred - g| < 1e-6 (where the sign of the gradient would hang on
    the last bit), and the restated loss is the float64 torch loss of the same fp32 tensors."""
    import torch
    L = PR.loss_inputs()
    for kw in (dict(xyz=L["xyz"], rot=L["rot"], trans=L["trans"]), dict(target=L["target"])):
        loss, pair, ds = PR.l1_pairs(L["pred"], L["lens"], L["row0"], **kw)
        assert min(np.abs(d).min() for d in ds) >= 1e-6
        want = []
        for p, n in enumerate(L["lens"]):
            sl = slice(int(L["row0"][p]), int(L["row0"][p]) + int(n))
            q = torch.from_numpy(L["pred"][sl]).double()
            if "target" in kw:
                g = torch.from_numpy(L["target"][sl]).double()
            else:
                g = (torch.from_numpy(L["rot"][p]).double() @ torch.from_numpy(L["xyz"][sl]).double().T).T + torch.from_numpy(L["trans"][p]).double()
            want.append(torch.mean(torch.sum(torch.abs(q - g), dim=-1)).item())
        assert np.all(np.abs(pair - np.array(want)) <= 1e-12 * np.abs(want))
        assert abs(float(loss) - np.mean(want)) <= 2.0 ** -22 * np.mean(want)
        g = PR.l1_pairs_grad(np.float32(1.0), ds, L["lens"], L["row0"], L["rows_src"])
        assert g.shape == L["pred"].shape and not g[int(L["lens"][0]):int(L["row0"][1])].any()


def test_binding_declares_the_new_entry_points():
    for name in ("scream_prep_pairs_workspace_bytes", "scream_prep_pairs", "scream_l1_pairs_workspace_bytes", "scream_l1_pairs_fwd",
                 "scream_l1_pairs_bwd"):
        assert name in _lib.SIGNATURES
    import scream_amd
    for name in ("sample_perturbations", "prepare_pairs", "prepare_3dmatch_train", "prepare_3dmatch_val", "prepare_kitti_train",
                 "prepare_kitti_val", "packed_l1_loss", "PreparedPairs"):
        assert hasattr(scream_amd, name) and name in scream_amd.__all__
