#!/usr/bin/env python3
"""Training throughput of PointTransformer (6 + 6 layers) on 3DMatch-like pairs, and the weight-gradient GEMM's rate; or, with
--model dem, of DEMTransformer (6 + 6 layers) on OpenGF-like terrain.

    python tools/train_bench.py [--batches 4,32] [--steps 3] [--warmup 1] [--train-backend f32|split|bf16] [--wgrad-only | --no-wgrad] [--json OUT]
    python tools/train_bench.py --model dem [--batches 1,8] [--points 4000,16000] [--train-backend f32|split|bf16] [--json OUT]

One step = training forward + loss + backward + Adam (lr 2e-4) over a packed batch of B pairs; pairs/s = B / step time
(wall clock around torch.cuda.synchronize) in the arithmetic of --train-backend (net.train_backend).  The wgrad part times
scream_gemm_wgrad_f32 and scream_gemm_wgrad_split_f32 (partial and reduce launches) with events at 64 k and 330 k rows and
reports fp32-equivalent TFLOP/s = 2 rows N K / t, the first against the 157 TF fp32 MFMA peak, the second against the bf16 x 3
roof (2 500 TF bf16 peak / 6 products = 417 TF).  The DEM leg is
train_open_gf.py's step (L1 loss, two stems) on scream_amd.evaluate_open_gf.SyntheticDEM samples of `points` DSM points and
their coarse DEM (20 m voxels); it reports samples/s and the peak memory of each (points, B) leg.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/train_bench.py` for the per-kernel split (tools/rocprof_summary.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd import train  # noqa: E402
from scream_amd.evaluate_open_gf import SyntheticDEM  # noqa: E402
from scream_amd.model import DEMTransformer, PointTransformer  # noqa: E402
from scream_amd.packing import PackedBatch  # noqa: E402
from scream_amd.synthetic import make_3dmatch_pair, make_state_dict  # noqa: E402

PEAK_TF = 157.0
PEAK_TF_BF3 = 2500.0 / 6  # six bf16 products per fp32-accurate one
DEV = "cuda:0"


def pair(seed):
    """A 3DMatch-like pair, normalised as datasets/three_d_match.py:228-242 does (unit ball around the registered union)."""
    src, tgt, T = make_3dmatch_pair(seed)[:3]
    rot, t = T[:3, :3], T[:3, 3:]
    reg = np.concatenate([(rot @ src.T + t).T, tgt])
    c = reg.mean(0)
    s = 1.0 / np.linalg.norm(reg - c, axis=1).max()
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return f(s * (src - c)), f(s * (tgt - c)), f(rot), f(s * (t - c.reshape(3, 1) + rot @ c.reshape(3, 1)))


def bench_training(B, steps, warmup, backend):
    net = PointTransformer(256, 6, 6)
    net.load_state_dict(make_state_dict(0, 256, 6, 6))
    net.train_backend = backend
    net = net.to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=2e-4)
    pairs = [pair(100 + i) for i in range(B)]
    batch = PackedBatch.from_pairs([p[0] for p in pairs], [p[1] for p in pairs], [p[3].reshape(3) for p in pairs])

    def step():
        pred = net.forward_packed_train(batch)
        loss = torch.stack([net.loss(x[None], p[0][None], p[2][None], p[3][None])
                            for x, p in zip(batch.unpack_src(pred), pairs)]).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []  # per step, each ended by a synchronise: the median is what two legs of a comparison are compared by
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t1)
    dt = (time.perf_counter() - t0) / steps
    pts = sum(p[0].shape[0] + p[1].shape[0] for p in pairs) / B
    return dict(B=B, train_backend=backend, step_s=dt, step_median_s=float(np.median(times)), pairs_per_s=B / dt, mean_points_per_pair=pts, rows_total=batch.rows_total,
                loss=float(loss.detach()), peak_mem_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def bench_dem_training(B, points, steps, warmup, backend):
    """train_open_gf.py:79-116 (use_GAN=False) on B SyntheticDEM samples packed into one batch (zero centres, raw coordinates)."""
    net = DEMTransformer(256, 6, 6)
    net.load_state_dict(make_state_dict(0, 256, 6, 6, dem=True))
    net.train_backend = backend
    net = net.to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=2e-4)
    samples = [[t.to(DEV) for t in SyntheticDEM(1, 200 + i, points)[0][:3]] for i in range(B)]
    zero = torch.zeros(3, device=DEV)
    batch = PackedBatch.from_pairs([s[0] for s in samples], [s[1] for s in samples], [zero] * B)

    def step():
        pred = net.forward_packed_train(batch)
        loss = torch.stack([net.loss(x[None], s[2][None]) for x, s in zip(batch.unpack_src(pred), samples)]).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []  # per step, each ended by a synchronise: the median is what two legs of a comparison are compared by
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t1)
    dt = (time.perf_counter() - t0) / steps
    return dict(B=B, points=points, train_backend=backend, step_s=dt, step_median_s=float(np.median(times)), samples_per_s=B / dt, mean_coarse_points=sum(s[1].shape[0] for s in samples) / B,
                rows_src=batch.rows_src, rows_total=batch.rows_total, loss=float(loss.detach()),
                peak_mem_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def bench_wgrad(reps=20):
    out = []
    for rows in (65536, 330 * 1024):
        for N, K in ((256, 256), (1024, 256), (256, 1024), (768, 256)):
            dY = torch.randn(rows, N, device=DEV)
            X = torch.randn(rows, K, device=DEV)
            dW = torch.empty(N, K, device=DEV)
            for kernel, fn, peak in (("f32", train.wgrad, PEAK_TF), ("split", train.wgrad_split, PEAK_TF_BF3)):
                fn(dY, X, dW)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn(dY, X, dW)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / reps / 1e3
                tf = 2.0 * rows * N * K / t / 1e12
                out.append(dict(kernel=kernel, rows=rows, N=N, K=K, us=t * 1e6, tflops=tf, frac_of_peak=tf / peak))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("point", "dem"), default="point")
    ap.add_argument("--batches", default=None, help="default 4,32 (point) or 1,8 (dem)")
    ap.add_argument("--points", default="4000,16000", help="DSM points per sample (dem)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--train-backend", choices=PointTransformer.TRAIN_BACKENDS, default="f32", help="net.train_backend of the training legs")
    ap.add_argument("--wgrad-only", action="store_true")
    ap.add_argument("--no-wgrad", action="store_true", help="training legs only (the legs of a backend comparison)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.model == "dem":
        res = dict(model="dem", train=[])
        for pts in (int(p) for p in a.points.split(",")):
            for B in (int(b) for b in (a.batches or "1,8").split(",")):
                r = bench_dem_training(B, pts, a.steps, a.warmup, a.train_backend)
                res["train"].append(r)
                print("dem train %s points %5d B %2d: %.3f s/step (median %.3f)  %.1f samples/s  (%.0f coarse points, %d rows, peak %.1f GB)"
                      % (a.train_backend, pts, B, r["step_s"], r["step_median_s"], r["samples_per_s"], r["mean_coarse_points"], r["rows_total"], r["peak_mem_gb"]))
        if a.json:
            os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
            json.dump(res, open(a.json, "w"), indent=1)
        return
    res = dict(wgrad=[] if a.no_wgrad else bench_wgrad())
    for r in res["wgrad"]:
        print("wgrad %-5s rows %7d N %4d K %4d: %8.1f us  %6.1f TFLOP/s  %.2f of its roof" % (r["kernel"], r["rows"], r["N"], r["K"], r["us"], r["tflops"], r["frac_of_peak"]))
    if not a.wgrad_only:
        res["train"] = []
        for B in (int(b) for b in (a.batches or "4,32").split(",")):
            r = bench_training(B, a.steps, a.warmup, a.train_backend)
            res["train"].append(r)
            print("train %s B %2d: %.3f s/step (median %.3f)  %.1f pairs/s  (%.0f points/pair, peak %.1f GB)" % (a.train_backend, B, r["step_s"], r["step_median_s"], r["pairs_per_s"],
                                                                                                   r["mean_points_per_pair"], r["peak_mem_gb"]))
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
