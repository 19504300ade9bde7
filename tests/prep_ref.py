"""Float64 numpy restatement of the batch-preparation and packed-loss contract of include/scream_hip.h (csrc/prep.hip), step for
step: one IEEE float64 operation per step, the 256-row chunk order of every sum, Philox4x32-10 and the Box-Muller normals.
Written from the header, not from the kernels; shared by tests/test_prep_host.py and tests/test_gpu_prep.py."""
import numpy as np

CHUNK = 256
TILE = 128
TWO_PI = 6.283185307179586
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [...,4], key [...,2] (broadcastable) uint32 -> uint32 [...,4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & np.uint64(MASK)]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def gauss3(seed, sample_id, cloud, n):
    """z float64 [n,3] of rows 0 .. n - 1 of one cloud."""
    seed, sid = int(seed) & (2 ** 64 - 1), int(sample_id) & (2 ** 64 - 1)
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    ctr[:, 1] = cloud
    ctr[:, 2] = sid & MASK
    ctr[:, 3] = sid >> 32
    w = philox4x32_10(ctr, np.array([seed & MASK, seed >> 32], dtype=np.uint32)).astype(np.float64)
    u = (w + 0.5) * (1.0 / 4294967296.0)
    r, th = np.sqrt(-2.0 * np.log(u[:, 0])), TWO_PI * u[:, 1]
    return np.stack([r * np.cos(th), r * np.sin(th), np.sqrt(-2.0 * np.log(u[:, 2])) * np.cos(TWO_PI * u[:, 3])], axis=1)


def chunk_sums(v):
    """v [n, ...] -> [ceil(n / 256), ...]: every chunk summed in ascending row order (cumsum is sequential)."""
    return np.stack([np.cumsum(v[i:i + CHUNK], axis=0)[-1] for i in range(0, v.shape[0], CHUNK)], axis=0)


def cloud_sum(*clouds):
    """The chunk sums of the clouds, in the order given, added in ascending chunk order."""
    return np.cumsum(np.concatenate([chunk_sums(v) for v in clouds], axis=0), axis=0)[-1]


def dot3(R, x):
    """(R[k][0]*x0 + R[k][1]*x1) + R[k][2]*x2 for x [...,3] -> [...,3]."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([(R[k, 0] * x[..., 0] + R[k, 1] * x[..., 1]) + R[k, 2] * x[..., 2] for k in range(3)], axis=-1)


def apply(R, t, x):
    return dot3(R, x) + t


def matmul3(A, B):
    return np.array([[(A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)])


def prep_pair(src, tgt, T, perturb=None, side=0, noise_std=0.0, seed=0, sample_id=0, mode="ball", center_rule=0):
    """One pair through steps 1-7.  src / tgt: float32 or float64 [n,3].  Returns a dict: src_n / tgt_n fp32 [n,3], rot fp32 [3,3],
    trans fp32 [3], s, c, T_aug float64, center fp32 [3], and a_src / a_tgt (the augmented metric clouds, float64)."""
    x = [np.asarray(src).astype(np.float64), np.asarray(tgt).astype(np.float64)]
    T = np.asarray(T, dtype=np.float64)
    P = np.eye(4) if perturb is None else np.asarray(perturb, dtype=np.float64)
    sd = 1 if side else 0
    TR, Tt, PR = T[:3, :3], T[:3, 3], P[:3, :3]
    m = cloud_sum(x[sd]) / float(x[sd].shape[0])
    Pt = (P[:3, 3] + m) - dot3(PR, m)
    if sd == 0:
        q = -dot3(PR.T, Pt)
        R2, t2 = matmul3(TR, PR.T), apply(TR, Tt, q)
    else:
        R2, t2 = matmul3(PR, TR), apply(PR, Pt, Tt)
    a = [apply(PR, Pt, x[c]) if c == sd else x[c].copy() for c in range(2)]
    if noise_std > 0.0:
        a = [a[c] + noise_std * gauss3(seed, sample_id, c, a[c].shape[0]) for c in range(2)]
    reg = [apply(R2, t2, a[0]), a[1]]
    n_all = reg[0].shape[0] + reg[1].shape[0]
    if mode == "ball":
        c = cloud_sum(reg[0], reg[1]) / float(n_all)
        d = np.concatenate(reg, axis=0) - c
        s = 1.0 / np.sqrt(np.max((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    else:
        both = np.concatenate(reg, axis=0)
        lo, hi = both.min(axis=0), both.max(axis=0)
        c = (lo + hi) / 2.0
        s = 1.0 / (np.max(hi - lo) / 2.0)
    out = [(s * (a[k] - c)).astype(np.float32) for k in range(2)]
    tr = s * ((t2 - c) + dot3(R2, c))
    if center_rule == 0:
        cen = cloud_sum(out[0].astype(np.float64)) / float(out[0].shape[0])
    elif center_rule == 1:
        cen = tr
    else:
        cen = -dot3(R2.T, tr)
    T_aug = np.eye(4)
    T_aug[:3, :3], T_aug[:3, 3] = R2, t2
    return dict(src_n=out[0], tgt_n=out[1], rot=R2.astype(np.float32), trans=tr.astype(np.float32), s=float(s), c=c, T_aug=T_aug,
                center=np.asarray(cen).astype(np.float32), a_src=a[0], a_tgt=a[1])


def pad_rows(n):
    return (n + TILE - 1) // TILE * TILE


def pack(per_pair, key_src="src_n", key_tgt="tgt_n"):
    """The packed xyz [rows_total,3] fp32 of a list of prep_pair results (zero padding), and each cloud's first row."""
    clouds = [r[key_src] for r in per_pair] + [r[key_tgt] for r in per_pair]
    row0 = np.concatenate([[0], np.cumsum([pad_rows(c.shape[0]) for c in clouds])]).astype(np.int64)
    xyz = np.zeros((int(row0[-1]), 3), dtype=np.float32)
    for r, c in zip(row0[:-1], clouds):
        xyz[r:r + c.shape[0]] = c
    return xyz, row0[:-1]


def raw_pair(seed, n, m, dtype=np.float64):
    """A seeded metric pair: n source and m target points of a 3 m room and the 4x4 that registers the source onto the target."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-1.0, 1.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    T[:3, 3] = rng.uniform(-1.0, 1.0, size=3)
    tgt = rng.uniform(0.0, 3.0, size=(m, 3))
    world = rng.uniform(0.0, 3.0, size=(n, 3))
    src = (world - T[:3, 3]) @ T[:3, :3]  # T^-1 world
    return src.astype(dtype), tgt.astype(dtype), T


LOSS_LENS = [(129, 300), (257, 2), (1000, 255)]


def loss_inputs(seed=3):
    """The seeded inputs of the loss tests, identical on the host and on the GPU: three normalised pairs (prep_pair, ball), a
    packed fp32 prediction and a packed fp32 target.  Returns a dict of numpy arrays."""
    pairs = [prep_pair(*raw_pair(seed * 10 + i, n, m), mode="ball", center_rule=1) for i, (n, m) in enumerate(LOSS_LENS)]
    xyz, row0 = pack(pairs)
    B = len(pairs)
    lens = np.array([p["src_n"].shape[0] for p in pairs])
    rows_src = int(row0[B])
    rng = np.random.default_rng(seed)
    pred = np.zeros((rows_src, 3), dtype=np.float32)
    target = np.zeros((rows_src, 3), dtype=np.float32)
    for p in range(B):
        sl = slice(int(row0[p]), int(row0[p]) + int(lens[p]))
        g = apply(pairs[p]["rot"].astype(np.float64), pairs[p]["trans"].astype(np.float64), xyz[sl].astype(np.float64))
        # errors of either sign and at least 1e-3 in size: no difference sits where its sign would hang on the last bit
        e1, e2 = rng.normal(scale=0.05, size=g.shape), rng.normal(scale=0.05, size=g.shape)
        pred[sl] = (g + (e1 + np.copysign(1e-3, e1))).astype(np.float32)
        target[sl] = (pred[sl].astype(np.float64) - (e2 + np.copysign(1e-3, e2))).astype(np.float32)
    return dict(pairs=pairs, xyz=xyz, row0=row0, lens=lens, rows_src=rows_src, pred=pred, target=target,
                rot=np.stack([p["rot"] for p in pairs]), trans=np.stack([p["trans"] for p in pairs]))


def l1_pairs(pred, lens, row0, xyz=None, rot=None, trans=None, target=None):
    """(loss fp32, loss_pair float64 [B], d: list of float64 [N_p,3] differences pred - g) of the packed fp32 tensors."""
    B = len(lens)
    pair, ds = np.zeros(B), []
    for p in range(B):
        sl = slice(int(row0[p]), int(row0[p]) + int(lens[p]))
        q = pred[sl].astype(np.float64)
        if target is not None:
            g = target[sl].astype(np.float64)
        else:
            g = apply(rot[p].astype(np.float64).reshape(3, 3), trans[p].astype(np.float64).reshape(3), xyz[sl].astype(np.float64))
        d = q - g
        ds.append(d)
        pair[p] = cloud_sum((np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])) / float(lens[p])
    return np.float32(np.cumsum(pair)[-1] / float(B)), pair, ds


def l1_pairs_grad(dout, ds, lens, row0, rows_src):
    """dpred fp32 [rows_src,3] for the fp32 upstream gradient dout."""
    B = len(lens)
    g = np.zeros((rows_src, 3), dtype=np.float32)
    for p in range(B):
        g[int(row0[p]):int(row0[p]) + int(lens[p])] = ((float(dout) * np.sign(ds[p])) / (float(lens[p]) * float(B))).astype(np.float32)
    return g
