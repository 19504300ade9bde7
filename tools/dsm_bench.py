#!/usr/bin/env python3
"""DSM extraction (csrc/dsm.hip) timing against two torch formulations of the same search, on the same GPU in the same run.

    python tools/dsm_bench.py [--runs 20] [--warmup 3] [--json profiles/dsm_bench.json]

Data: seeded synthetic 100 m windows as they look AFTER the 1 m down-sampling -- POINTS window points uniform on [0, 100)^2
(1.4 / m^2) over a smooth relief, 30 % of them lifted 1-12 m ("vegetation"); the ground points are the other 70 %
(about 0.98 / m^2, ~9 800 queries per window).  Radius 0.8 m.

Timed, HIP events around the calls, median / min / max of --runs after --warmup:
  kernel   ops.dsm_extract_packed on packed rows (plan, count, scan, scatter, query; workspace allocation included), at 1 window
           and at 64 windows per call; every kernel and call timing repeats the call INNER times inside one event pair (a
           single one is too short to time) and the figure is per call
  call     the public extract_dsm_batch (packing, launches, slicing) at the same two sizes
  loop     (i) the reference's formulation restated: a Python loop over the ground points, each with one norm over the whole
           window and two .item() synchronisations -- at 1 window, --loop-runs times
  dense    (ii) a chunked masked M x N maximum in torch (float64 distances, the contract's predicate), per window -- at 1 and 64
Before anything is timed the three results are compared on the first window, and the 64-window call with the dense formulation
on all its windows (heights and hit / miss; the torch formulations do not pin which of two equally high points they return).  Nothing here falls back to the CPU: no GPU is an error."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POINTS = 14000
SIDE = 100.0
VEGETATION = 0.3
RADIUS = 0.8
BATCH = 64
INNER = 20
CHUNK = 2048


def make_window(seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, SIDE, size=(POINTS, 2))
    z = 8 * np.sin(0.01 * xy[:, 0] + seed) + 6 * np.cos(0.015 * xy[:, 1])
    veg = rng.random(POINTS) < VEGETATION
    z = z + np.where(veg, rng.uniform(1.0, 12.0, size=POINTS), 0.0)
    xyz = np.ascontiguousarray(np.concatenate([xy, z[:, None]], axis=1), dtype=np.float32)
    return xyz, xyz[~veg]


def main():
    import torch
    from scream_amd import ops
    from scream_amd.dsm import extract_dsm_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-runs", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dsm_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    host = [make_window(500 + i) for i in range(BATCH)]
    patches = [torch.from_numpy(p).to(dev) for p, _ in host]
    dems = [torch.from_numpy(d).to(dev) for _, d in host]

    def packed(n):
        ps, ds = patches[:n], dems[:n]
        pl, dl = [int(p.shape[0]) for p in ps], [int(d.shape[0]) for d in ds]
        starts = lambda lens: [int(v) for v in np.cumsum([0] + lens[:-1])]
        meta = torch.tensor([starts(pl), pl, starts(dl), dl], dtype=torch.int32).to(dev)
        return torch.cat(ps).contiguous(), meta[0], meta[1], max(pl), torch.cat(ds).contiguous(), meta[2], meta[3], max(dl)

    def loop_one(window, ground):  # (i) one pass over the whole window and two host synchronisations per ground point
        answer = ground.clone()
        w_xy, w_z = window[:, :2], window[:, 2]
        for k in range(ground.shape[0]):
            in_reach = torch.linalg.vector_norm(w_xy - ground[k, :2], dim=1) <= 0.8
            if int(in_reach.sum()) == 0:
                continue
            rows = window[in_reach]
            answer[k] = rows[int(rows[:, 2].argmax())]
        return answer

    r2 = float(np.float64(np.float32(RADIUS)) ** 2)

    def dense_one(patch, dem):  # (ii) chunked masked M x N maximum
        out = []
        px, py, pz = patch[:, 0][None], patch[:, 1][None], patch[:, 2][None]
        for s in range(0, dem.shape[0], CHUNK):
            q = dem[s:s + CHUNK]
            dx, dy = (px - q[:, 0:1]).double(), (py - q[:, 1:2]).double()
            z = torch.where(dx * dx + dy * dy <= r2, pz, torch.full_like(pz, float("-inf")))
            zmax, arg = z.max(dim=1)
            out.append(torch.where((zmax > float("-inf"))[:, None], patch[arg], q))
        return torch.cat(out, dim=0)

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

    # the three formulations on the first window, and kernel against dense on all 64, before any timing
    one, many = packed(1), packed(BATCH)
    k_xyz, k_idx = ops.dsm_extract_packed(*one, RADIUS)
    d_xyz, l_xyz = dense_one(patches[0], dems[0]), loop_one(patches[0], dems[0])
    b_xyz, b_idx = ops.dsm_extract_packed(*many, RADIUS)
    bd_xyz = torch.cat([dense_one(p, d) for p, d in zip(patches, dems)], dim=0)
    agree = dict(queries=int(dems[0].shape[0]), hits=int((k_idx >= 0).sum()),
                 dense_height_mismatches=int((d_xyz[:, 2] != k_xyz[:, 2]).sum()),
                 loop_row_mismatches=int((l_xyz != k_xyz).any(dim=1).sum()),
                 batch_queries=int(b_idx.shape[0]), batch_hits=int((b_idx >= 0).sum()),
                 batch_dense_height_mismatches=int((bd_xyz[:, 2] != b_xyz[:, 2]).sum()),
                 batch_first_window_differs_from_single=int((b_xyz[:k_xyz.shape[0]] != k_xyz).any(dim=1).sum()))
    print("agreement: %s" % agree, flush=True)
    assert agree["dense_height_mismatches"] == 0 and agree["batch_dense_height_mismatches"] == 0, \
        "the dense formulation uses the contract's own predicate: it must agree"
    assert agree["batch_first_window_differs_from_single"] == 0
    assert agree["loop_row_mismatches"] <= max(1, agree["queries"] // 1000), "the fp32 sqrt formulation differs only at the radius"

    res = dict(points_per_window=POINTS, side_m=SIDE, window_points_per_m2=POINTS / SIDE ** 2, vegetation_share=VEGETATION,
               ground_points_per_window_mean=float(np.mean([d.shape[0] for d in dems])), radius=RADIUS, agreement=agree,
               device=torch.cuda.get_device_name(0))
    res["kernel_1"] = timed(lambda: ops.dsm_extract_packed(*one, RADIUS), a.runs, a.warmup, INNER)
    res["kernel_64"] = timed(lambda: ops.dsm_extract_packed(*many, RADIUS), a.runs, a.warmup, INNER)
    res["call_1"] = timed(lambda: extract_dsm_batch(patches[:1], dems[:1], RADIUS), a.runs, a.warmup, INNER)
    res["call_64"] = timed(lambda: extract_dsm_batch(patches, dems, RADIUS), a.runs, a.warmup, INNER)
    res["dense_1"] = timed(lambda: dense_one(patches[0], dems[0]), a.runs, a.warmup)
    res["dense_64"] = timed(lambda: [dense_one(p, d) for p, d in zip(patches, dems)], max(a.runs // 4, 3), 1)
    res["loop_1"] = timed(lambda: loop_one(patches[0], dems[0]), a.loop_runs, 0)  # the comparison above was its warm-up
    res["dense_64_over_kernel_64"] = res["dense_64"]["median_ms"] / res["kernel_64"]["median_ms"]
    res["dense_1_over_kernel_1"] = res["dense_1"]["median_ms"] / res["kernel_1"]["median_ms"]
    res["loop_1_over_kernel_1"] = res["loop_1"]["median_ms"] / res["kernel_1"]["median_ms"]
    res["kernel_faster_than_dense_at_64"] = bool(res["kernel_64"]["median_ms"] < res["dense_64"]["median_ms"])
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
