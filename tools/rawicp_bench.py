"""Times of the raw-scan ICP (scream_amd.rawicp, csrc/icp_raw.hip) on synthetic KITTI-sized scans -> profiles/rawicp_bench.json.

    python tools/rawicp_bench.py [--out profiles/rawicp_bench.json]

Workload: a street canyon (ground plane, four walls) ray-cast from two poses 10 m apart by a 64-beam scanner, about 120 k
returns per scan within 80 m, 1 cm of range noise; the start pose is the truth moved by 0.2 m and 0.3 degrees (what KITTI odometry
leaves).  One and eight pairs per call.  Every figure is the median of REPS = 20 runs, the host clock around a synchronise (the two slow
comparison figures, ops.icp_p2p and the dense evaluation of eight pairs, of 5 runs; the file records the counts):
  set-up              grid, records and status (the it_begin == 0 part of scream_icp_raw_range)
  time per iteration  from a schedule of ITERS iterations with both thresholds 0
  whole refinement    RawIcpRun.run(32) under 1e-6 / 1e-6 with max_iter 50000, set-up included; and its number of iterations
Two comparisons in the same run on the same clouds:
  ops.icp_p2p         its time per iteration, and the number of source rows whose first-evaluation correspondence (the fp32
                      expanded selection, through ops.nn_search on the fp32-transformed source) differs from the float64 brute
                      force.  The count is why it cannot be used; its time is context.
  dense torch         one evaluation as chunked float64 tensors (direct differences, argmin, strict radius); its first-evaluation
                      idx is compared with the kernel's on ALL rows before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scream_amd import ops  # noqa: E402
from scream_amd.rawicp import RawIcpRun, raw_nn_batch  # noqa: E402

REPS, ITERS, DENSE_REPS_8, P2P_REPS = 20, 10, 5, 5
RADIUS = 0.2


def rot_z(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def scan(pose, seed, steps=2083):
    """Returns of a 64-beam scanner at `pose` (4x4, sensor in world) in the sensor's frame, fp32 [N,3]."""
    rng = np.random.default_rng(seed)
    elev = np.radians(np.linspace(-24.8, 2.0, 64))[:, None] + np.zeros((1, steps))
    azim = (np.arange(steps) * (2 * np.pi / steps))[None, :] + rng.uniform(0, 2 * np.pi / steps) + np.zeros((64, 1))
    d = np.stack([np.cos(elev) * np.cos(azim), np.cos(elev) * np.sin(azim), np.sin(elev)], axis=-1).reshape(-1, 3)
    dw, o = d @ pose[:3, :3].T, pose[:3, 3]
    t = np.full(len(d), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, planes in ((2, (0.0,)), (0, (-9.0, 11.0)), (1, (-70.0, 75.0))):
            for p in planes:
                tt = (p - o[axis]) / dw[:, axis]
                t = np.where((tt > 0.5) & (tt < t), tt, t)
    keep = t < 80.0
    t = t[keep] + 0.01 * rng.normal(size=int(keep.sum()))
    return (d[keep] * t[:, None]).astype(np.float32)


def make_pair(seed):
    """(src, tgt, T0, T_true): T_true maps the source scan's frame onto the target scan's."""
    rng = np.random.default_rng(seed)
    P0, P1 = np.eye(4), np.eye(4)
    P0[:3, 3] = [rng.uniform(-2, 2), rng.uniform(-20, 20), 1.73]
    P0[:3, :3] = rot_z(90 + rng.uniform(-5, 5))
    P1[:3, :3] = P0[:3, :3] @ rot_z(rng.uniform(-4, 4))
    P1[:3, 3] = P0[:3, 3] + P0[:3, :3] @ np.array([10.5, rng.uniform(-0.3, 0.3), 0.0])
    Tt = np.linalg.inv(P1) @ P0
    D = np.eye(4)
    D[:3, :3] = rot_z(0.3)
    u = rng.normal(size=3)
    D[:3, 3] = 0.2 * u / np.linalg.norm(u)
    return scan(P0, seed), scan(P1, seed + 1000), D @ Tt, Tt


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), out


def dense_eval(srcs, tgts, Ts, r2, chunk=1024):
    """One evaluation per pair as dense chunked float64 torch: (idx int64 with -1 for none, count, sum d2) per pair."""
    res = []
    for s, t, T in zip(srcs, tgts, Ts):
        x, b = s.double(), t.double()
        a = torch.stack([((T[k, 0] * x[:, 0] + T[k, 1] * x[:, 1]) + T[k, 2] * x[:, 2]) + T[k, 3] for k in range(3)], dim=1)
        idx = torch.empty(len(a), dtype=torch.int64, device=a.device)
        lo = torch.empty(len(a), dtype=torch.float64, device=a.device)
        for i0 in range(0, len(a), chunk):
            q = a[i0:i0 + chunk]
            d = (q[:, 0:1] - b[None, :, 0]) ** 2
            d += (q[:, 1:2] - b[None, :, 1]) ** 2
            d += (q[:, 2:3] - b[None, :, 2]) ** 2
            lo[i0:i0 + chunk], idx[i0:i0 + chunk] = d.min(dim=1)
        ok = lo < r2
        res.append((torch.where(ok, idx, -1), int(ok.sum()), float(lo[ok].sum())))
    return res


def bench(n_pairs, dev):
    pairs = [make_pair(7 + k) for k in range(n_pairs)]
    srcs = [torch.from_numpy(p[0]).to(dev) for p in pairs]
    tgts = [torch.from_numpy(p[1]).to(dev) for p in pairs]
    T0 = np.stack([p[2] for p in pairs])
    out = {"pairs": n_pairs, "src_points": [len(s) for s in srcs], "tgt_points": [len(t) for t in tgts]}

    # ---- the kernel's first evaluation against dense torch, on all rows, before anything is timed
    kidx, _ = raw_nn_batch(srcs, tgts, T0, RADIUS)
    dense = dense_eval(srcs, tgts, torch.from_numpy(T0).to(dev), RADIUS * RADIUS)
    differ = [int((k.long() != d[0]).sum()) for k, d in zip(kidx, dense)]
    assert sum(differ) == 0, "kernel and dense torch disagree on %s rows" % differ
    out["first_eval_rows_differing_from_dense_torch"] = differ
    out["first_eval_fitness"] = [d[1] / len(s) for d, s in zip(dense, srcs)]

    # ---- the kernel
    def setup():
        RawIcpRun(srcs, tgts, T0, RADIUS, ITERS, 0.0, 0.0).advance(0)

    def setup_and_iters():
        RawIcpRun(srcs, tgts, T0, RADIUS, ITERS, 0.0, 0.0).advance(ITERS)

    whole = {}

    def refine():
        run = RawIcpRun(srcs, tgts, T0, RADIUS, 50000, 1e-6, 1e-6).run(32)
        whole["iters"], whole["fitness_rmse"], whole["T"] = run.iters.cpu().tolist(), run.fitness_rmse.cpu().tolist(), run.T.cpu().numpy()

    setup(), refine()  # warm-up
    out["setup_ms"], _ = median_ms(setup, REPS)
    both, _ = median_ms(setup_and_iters, REPS)
    out["iteration_ms"] = (both - out["setup_ms"]) / ITERS
    out["refinement_ms"], _ = median_ms(refine, REPS)
    out["refinement_iters"] = whole["iters"]
    out["refinement_fitness_rmse"] = whole["fitness_rmse"]
    out["pose_error_m_deg"] = [[float(np.linalg.norm(T[:3, 3] - p[3][:3, 3])),
                                float(np.degrees(np.arccos(np.clip((np.trace(T[:3, :3] @ p[3][:3, :3].T) - 1) / 2, -1, 1))))]
                               for T, p in zip(whole["T"], pairs)]

    # ---- ops.icp_p2p on the same clouds
    src_p, tgt_p = torch.cat(srcs), torch.cat(tgts)
    sl, tl = [len(s) for s in srcs], [len(t) for t in tgts]
    meta = torch.from_numpy(np.array([np.concatenate([[0], np.cumsum(sl)[:-1]]), sl, np.concatenate([[0], np.cumsum(tl)[:-1]]), tl], dtype=np.int32)).to(dev)
    ones, zeros = torch.ones(n_pairs, device=dev), torch.zeros(n_pairs, 3, device=dev)
    T32 = torch.from_numpy(T0.astype(np.float32)).to(dev)

    def p2p(iters):
        return ops.icp_p2p(src_p, tgt_p, meta[0], meta[1], meta[2], meta[3], ones, zeros, T32, max(sl), max(tl), RADIUS, iters, 0.0, 0.0)

    p2p(1)
    t1, _ = median_ms(lambda: p2p(1), P2P_REPS)
    tk, _ = median_ms(lambda: p2p(1 + ITERS), P2P_REPS)
    out["icp_p2p_reps"] = P2P_REPS
    out["icp_p2p_iteration_ms"] = (tk - t1) / ITERS
    q = torch.cat([(s @ T32[k, :3, :3].T + T32[k, :3, 3]) for k, s in enumerate(srcs)]).contiguous()
    idx32, _, valid32 = ops.nn_search(q, tgt_p, meta[0], meta[1], meta[2], meta[3], ones, max(sl), max(tl), float(np.float32(RADIUS) * np.float32(RADIUS)))
    idx32 = torch.where(valid32.bool(), idx32.long(), -1)
    want = torch.cat([d[0] for d in dense])
    out["icp_p2p_first_eval_rows_differing_from_float64"] = int((idx32 != want).sum())

    # ---- dense torch, one evaluation
    Td = torch.from_numpy(T0).to(dev)
    reps = REPS if n_pairs == 1 else DENSE_REPS_8
    out["dense_torch_evaluation_ms"], _ = median_ms(lambda: dense_eval(srcs, tgts, Td, RADIUS * RADIUS), reps)
    out["dense_torch_reps"] = reps
    out["kernel_iteration_speedup_over_dense_torch"] = out["dense_torch_evaluation_ms"] / out["iteration_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "rawicp_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rawicp_bench needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "iters_timed": ITERS, "radius": RADIUS,
           "runs": [bench(1, dev), bench(8, dev)]}
    assert res["runs"][1]["iteration_ms"] < res["runs"][1]["dense_torch_evaluation_ms"], "the kernel is not faster than dense torch"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
