"""The Chamfer contract of include/scream_hip.h (scream_chamfer_fwd / scream_chamfer_bwd) restated in numpy, operation by
operation.  The product code never imports this file; the tests compare the kernels with it bit for bit, and compare IT with the
reference's five lines (evaluate_open_gf.py:25-41) in float64.

numpy evaluates an fp32 (float64) array expression one IEEE operation per ufunc call, rounded once, with no fma: the bracketing
below is the order of operations.  np.cumsum adds strictly one element after the other, which is the chunk sum and the cloud sum
of the contract (np.sum is pairwise and is NOT)."""
import numpy as np

CHUNK = 256    # rows per chunk sum
ROW_TILE = 128  # a PackedBatch pads every cloud to this


def _seq_sum(v: np.ndarray) -> np.float64:
    """s = v[0]; s += v[1]; ... in float64."""
    return np.cumsum(np.asarray(v, dtype=np.float64))[-1]


def cloud_sum(d: np.ndarray) -> np.float64:
    """The float64 sum of the widened fp32 values of one cloud: 256-row chunks in ascending row order, then the chunks in
    ascending order."""
    d = np.asarray(d, dtype=np.float32).astype(np.float64)
    return _seq_sum([_seq_sum(d[c:c + CHUNK]) for c in range(0, d.shape[0], CHUNK)])


def nearest(a: np.ndarray, b: np.ndarray, block: int = 256):
    """(idx_ab int32 [N], d_ab fp32 [N], idx_ba int32 [M], d_ba fp32 [M]) of one pair, N, M >= 1: the fp32 difference form
    d(n,m) = ((dx*dx + dy*dy) + dz*dz) and the lowest index among equal minima on either side."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    N, M = a.shape[0], b.shape[0]
    idx_ab, d_ab = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float32)
    idx_ba, d_ba = np.full(M, -1, dtype=np.int32), np.full(M, np.inf, dtype=np.float32)
    for n0 in range(0, N, block):
        blk = a[n0:n0 + block]
        dx, dy, dz = (blk[:, None, k] - b[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        j = d.argmin(axis=1)  # the first occurrence: the lowest m
        idx_ab[n0:n0 + block], d_ab[n0:n0 + block] = j, d[np.arange(blk.shape[0]), j]
        i = d.argmin(axis=0)  # the lowest n of this block; an earlier block keeps an equal minimum (strict <)
        col = d[i, np.arange(M)]
        better = col < d_ba
        idx_ba[better], d_ba[better] = (n0 + i[better]).astype(np.int32), col[better]
    return idx_ab, d_ab, idx_ba, d_ba


def pair_value(d_ab: np.ndarray, d_ba: np.ndarray) -> np.float64:
    """loss_pair = S_ab / N + S_ba / M in float64; 0 for an empty side."""
    if d_ab.shape[0] == 0 or d_ba.shape[0] == 0:
        return np.float64(0.0)
    return cloud_sum(d_ab) / np.float64(d_ab.shape[0]) + cloud_sum(d_ba) / np.float64(d_ba.shape[0])


def pair_grad(a, b, idx_ab, idx_ba, g: np.float64):
    """(da, db) fp32 of one pair for g = float64(dout) / n_pairs: the nearest-neighbour term plus the scatter term, the latter
    accumulated in ascending index of the other side, one addition after the other from 0.0."""
    A, B = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    N, M = A.shape[0], B.shape[0]
    if N == 0 or M == 0:
        return np.zeros((N, 3), dtype=np.float32), np.zeros((M, 3), dtype=np.float32)
    w_ab, w_ba = (np.float64(2.0) * g) / np.float64(N), (np.float64(2.0) * g) / np.float64(M)
    acc_a, acc_b = np.zeros((N, 3)), np.zeros((M, 3))
    for m in range(M):
        n = idx_ba[m]
        acc_a[n] = acc_a[n] + (A[n] - B[m])
    for n in range(N):
        m = idx_ab[n]
        acc_b[m] = acc_b[m] + (B[m] - A[n])
    da = (A - B[idx_ab]) * w_ab + acc_a * w_ba
    db = (B - A[idx_ba]) * w_ba + acc_b * w_ab
    return da.astype(np.float32), db.astype(np.float32)


class Result:
    """What scream_chamfer_fwd and scream_chamfer_bwd write for a packed batch."""


def chamfer(a, a_row0, a_len, b, b_row0, b_len, dout=1.0) -> Result:
    """The whole contract over packed clouds a [a_rows,3], b [b_rows,3] and B pairs: idx / d per packed row (-1 / 0 outside every
    cloud and in a pair with an empty side), loss_pair float64 [B], loss fp32, da / db fp32 (zero outside every cloud)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    B = len(a_len)
    r = Result()
    r.idx_ab, r.d_ab = np.full(a.shape[0], -1, dtype=np.int32), np.zeros(a.shape[0], dtype=np.float32)
    r.idx_ba, r.d_ba = np.full(b.shape[0], -1, dtype=np.int32), np.zeros(b.shape[0], dtype=np.float32)
    r.da, r.db = np.zeros_like(a), np.zeros_like(b)
    r.loss_pair = np.zeros(B, dtype=np.float64)
    g = np.float64(np.float32(dout)) / np.float64(B)
    for p in range(B):
        sa, sb = slice(int(a_row0[p]), int(a_row0[p]) + int(a_len[p])), slice(int(b_row0[p]), int(b_row0[p]) + int(b_len[p]))
        if a_len[p] == 0 or b_len[p] == 0:
            continue
        r.idx_ab[sa], r.d_ab[sa], r.idx_ba[sb], r.d_ba[sb] = nearest(a[sa], b[sb])
        r.loss_pair[p] = pair_value(r.d_ab[sa], r.d_ba[sb])
        r.da[sa], r.db[sb] = pair_grad(a[sa], b[sb], r.idx_ab[sa], r.idx_ba[sb], g)
    r.loss = np.float32(_seq_sum(r.loss_pair) / np.float64(B))
    return r


def pack(clouds):
    """Clouds back to back, each zero padded to a multiple of 128 rows like a PackedBatch: (packed fp32 [rows,3], row0, len)."""
    row0, rows = [], 0
    for c in clouds:
        row0.append(rows)
        rows += (len(c) + ROW_TILE - 1) // ROW_TILE * ROW_TILE
    out = np.zeros((max(rows, ROW_TILE), 3), dtype=np.float32)
    for r0, c in zip(row0, clouds):
        out[r0:r0 + len(c)] = c
    return out, np.array(row0, dtype=np.int32), np.array([len(c) for c in clouds], dtype=np.int32)
