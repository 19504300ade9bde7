#!/usr/bin/env python3
"""Fixed-radius overlap search (csrc/radius.hip) timing against a dense torch formulation of the same search, on the same GPU in
the same run.

    python tools/overlap_bench.py [--runs 20] [--warmup 3] [--json profiles/overlap_bench.json]

Data: seeded synthetic 3DMatch pairs (scream_amd.synthetic.make_3dmatch_pair) voxelised at VOXEL so that a cloud has about
25 000 points, the size of a PREDATOR fragment at its 0.025 m voxel.  Radius 0.03 m, the reference's overlap radius.

Timed, HIP events around the calls, median / min / max of --runs after --warmup:
  count    ops.radius_count_packed on packed rows (plan, cell count, scan, scatter, query; workspace allocation included)
           at 1 pair and at 32 pairs per call
  pairs    the public radius_pairs_batch (count, prefix sum, one host read, fill, slicing) at the same two sizes
  prepare  the public prepare_3dmatch_batch (overlap, src[~mask], the 3 B clouds down-sampled at 0.0625 m) at the same two sizes
  dense    a chunked N x M torch formulation of the contract's predicate in float64 (one elementwise kernel per operation, so
           no step is contracted), per pair -- at 1 and 32
Before anything is timed the dense counts are compared with the kernel's on every point of all 32 pairs, and the 32-pair call
with the single calls.  Nothing here falls back to the CPU: no GPU is an error."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOXEL = 0.036
SAMPLES = 300000
RADIUS = 0.03
BATCH = 32
INNER = 5
CHUNK = 1024


def main():
    import torch
    from scream_amd import ops, synthetic
    from scream_amd.overlap import prepare_3dmatch_batch, radius_pairs_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "overlap_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    host = [synthetic.make_3dmatch_pair(700 + i, "3dmatch" if i % 2 == 0 else "lo", voxel=VOXEL, n_samples=SAMPLES)[:3] for i in range(BATCH)]
    srcs = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).to(dev) for s, _, _ in host]
    tgts = [torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for _, t, _ in host]
    rots = [T[:3, :3] for _, _, T in host]
    transs = [T[:3, 3:] for _, _, T in host]
    # the transform the preparation builds: float64 from the float32 rot | trans
    Ts = [np.concatenate([np.concatenate([r.astype(np.float32), t.astype(np.float32)], axis=1), np.array([[0, 0, 0, 1]])], axis=0)
          for r, t in zip(rots, transs)]
    Td = torch.from_numpy(np.stack(Ts)).to(dev)

    def packed(n):
        sl, tl = [int(s.shape[0]) for s in srcs[:n]], [int(t.shape[0]) for t in tgts[:n]]
        starts = lambda lens: [int(v) for v in np.cumsum([0] + lens[:-1])]
        meta = torch.tensor([starts(sl), sl, starts(tl), tl], dtype=torch.int32).to(dev)
        return (torch.cat(srcs[:n]).contiguous(), meta[0], meta[1], max(sl), torch.cat(tgts[:n]).contiguous(), meta[2], meta[3], max(tl),
                Td[:n].contiguous(), RADIUS)

    r2 = torch.tensor(RADIUS, dtype=torch.float64, device=dev) * torch.tensor(RADIUS, dtype=torch.float64, device=dev)

    def dense_one(src, tgt, M):  # the contract's operations in its order, one torch kernel each
        x, b = src.double(), tgt.double()
        A = [((M[k, 0] * x[:, 0] + M[k, 1] * x[:, 1]) + M[k, 2] * x[:, 2]) + M[k, 3] for k in range(3)]
        out = []
        for s in range(0, x.shape[0], CHUNK):
            d0, d1, d2 = (A[k][s:s + CHUNK, None] - b[None, :, k] for k in range(3))
            out.append((((d0 * d0 + d1 * d1) + d2 * d2) < r2).sum(dim=1))
        return torch.cat(out).to(torch.int32)

    def timed(fn, runs, warmup, inner=1):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / inner)
        return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), runs=runs, calls_per_timing=inner)

    one, many = packed(1), packed(BATCH)
    k_count, _ = ops.radius_count_packed(*one)
    b_count, _ = ops.radius_count_packed(*many)
    d_count = torch.cat([dense_one(s, t, Td[i]) for i, (s, t) in enumerate(zip(srcs, tgts))])
    agree = dict(points=int(b_count.shape[0]), overlapping_points=int((b_count > 0).sum()), neighbours=int(b_count.sum()),
                 neighbours_per_overlapping_point=float(b_count.sum()) / max(int((b_count > 0).sum()), 1),
                 dense_count_mismatches=int((d_count != b_count).sum()),
                 batch_first_pair_differs_from_single=int((b_count[:k_count.shape[0]] != k_count).sum()))
    print("agreement: %s" % agree, flush=True)
    assert agree["dense_count_mismatches"] == 0, "the dense formulation is the contract's own predicate: it must agree"
    assert agree["batch_first_pair_differs_from_single"] == 0

    res = dict(voxel=VOXEL, radius=RADIUS, pairs=BATCH, source_points_mean=float(np.mean([s.shape[0] for s in srcs])),
               target_points_mean=float(np.mean([t.shape[0] for t in tgts])), agreement=agree, device=torch.cuda.get_device_name(0))
    res["count_1"] = timed(lambda: ops.radius_count_packed(*one), a.runs, a.warmup, INNER)
    res["count_32"] = timed(lambda: ops.radius_count_packed(*many), a.runs, a.warmup, INNER)
    res["pairs_1"] = timed(lambda: radius_pairs_batch(srcs[:1], tgts[:1], Ts[:1], RADIUS), a.runs, a.warmup)
    res["pairs_32"] = timed(lambda: radius_pairs_batch(srcs, tgts, Ts, RADIUS), a.runs, a.warmup)
    res["prepare_1"] = timed(lambda: prepare_3dmatch_batch(srcs[:1], tgts[:1], rots[:1], transs[:1]), a.runs, a.warmup)
    res["prepare_32"] = timed(lambda: prepare_3dmatch_batch(srcs, tgts, rots, transs), a.runs, a.warmup)
    res["dense_1"] = timed(lambda: dense_one(srcs[0], tgts[0], Td[0]), a.runs, a.warmup)
    res["dense_32"] = timed(lambda: [dense_one(s, t, Td[i]) for i, (s, t) in enumerate(zip(srcs, tgts))], max(a.runs // 4, 3), 1)
    res["dense_1_over_count_1"] = res["dense_1"]["median_ms"] / res["count_1"]["median_ms"]
    res["dense_32_over_count_32"] = res["dense_32"]["median_ms"] / res["count_32"]["median_ms"]
    res["count_faster_than_dense_at_32"] = bool(res["count_32"]["median_ms"] < res["dense_32"]["median_ms"])
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
