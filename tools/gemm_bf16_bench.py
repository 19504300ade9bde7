#!/usr/bin/env python3
"""The three matrix products of train_backend "bf16" (csrc/gemm_bf16.hip) beside the "split" products they stand in for, and
beside the HBM roof.

    python tools/gemm_bf16_bench.py [--rows 65536,330240] [--reps 20] [--json OUT]

Per row count and (N, K) of the training step -- (256,256) merge / q, (768,256) q|k|v, (1024,256) mlp.0, (256,1024) mlp.2 -- the
forward C = A W^T, the data gradient dX = dY W and the weight gradient dW = dY^T X are timed through train.gemms(backend), i.e. with
everything a training step launches for them: "split" packs W (and transposes it for the data gradient, which runs in K = 256
chunks plus adds where the summed dimension is 768 or 1024), "bf16" is one launch (two for the weight gradient).  Legs
alternate split / bf16 / split / bf16; each figure is the median over --reps calls of device-event times after a warm-up
call, and the two equal legs show the noise.  The roof of a call is its operand and result bytes (fp32: A, W, C once each) over
the 6.29 TB/s measured copy rate; `of_roof` is roof time / measured time for the bf16 leg."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd import train  # noqa: E402
from scream_amd.model import PointTransformer  # noqa: E402

DEV = "cuda:0"
HBM_COPY_BYTES_PER_S = 6.29e12
SHAPES = [(256, 256), (768, 256), (1024, 256), (256, 1024)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="65536,330240")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_bf16_bench.py measures on the MI355X; no GPU found")
    mms = {backend: train.gemms(backend) for backend in PointTransformer.TRAIN_BACKENDS}
    out = []
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    for rows in (int(r) for r in a.rows.split(",")):
        for N, K in SHAPES:
            A, W, dY = rnd(rows, K), rnd(N, K) / 16, rnd(rows, N)
            C, dX, dW = torch.empty(rows, N, device=DEV), torch.empty(rows, K, device=DEV), torch.empty(N, K, device=DEV)
            calls = {"forward": lambda mm: mm.fwd(A, W), "dgrad": lambda mm: mm.dgrad(dY, W, out=dX), "wgrad": lambda mm: mm.wgrad(dY, A, dW)}
            for name, call in calls.items():
                legs = [timed(lambda: call(mms[b]), a.reps) for b in ("split", "bf16", "split", "bf16")]
                nbytes = 4 * (rows * K + rows * N + N * K)  # each of the three matrices once, whichever is the result
                roof = nbytes / HBM_COPY_BYTES_PER_S
                split_s, bf16_s = min(legs[0], legs[2]), min(legs[1], legs[3])
                rec = dict(rows=rows, N=N, K=K, product=name, split_s=[legs[0], legs[2]], bf16_s=[legs[1], legs[3]],
                           speedup=split_s / bf16_s, hbm_roof_s=roof, of_roof=roof / bf16_s, tflops_bf16=2.0 * rows * N * K / bf16_s / 1e12)
                out.append(rec)
                print("rows %6d N %4d K %4d %-7s split %8.1f %8.1f us  bf16 %8.1f %8.1f us  x%.2f  roof %7.1f us (%.0f %% of it)  %.0f TFLOP/s"
                      % (rows, N, K, name, legs[0] * 1e6, legs[2] * 1e6, legs[1] * 1e6, legs[3] * 1e6, rec["speedup"], roof * 1e6,
                         100 * rec["of_roof"], rec["tflops_bf16"]), flush=True)
            del A, W, dY, C, dX, dW
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S, results=out), f, indent=1)


if __name__ == "__main__":
    main()
