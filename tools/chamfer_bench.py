#!/usr/bin/env python3
"""What the HIP Chamfer distance costs on the MI355X, against the two ways there were to compute it, in one process.

    python tools/chamfer_bench.py [--runs 20] [--steps 8] [--no-step] [--json profiles/chamfer_bench.json]

Shapes: "dem" B = 8 samples of 16 000 points against 16 000 (the DEM training shape), "3dmatch" B = 32 pairs of 5 135 against
5 100 rows.  Legs, alternating run by run, each timed with device events around the calls of one run:
  packed_fwd / packed_fwd_bwd   chamfer_packed over the whole batch (csrc/chamfer.hip), and with its backward into a
  search_fwd                    B calls of geometry.chamfer_distance, two scream_nn_search each: forward only, it has no gradient
  dense_fwd / dense_fwd_bwd     the reference's formulation in torch on the same GPU: square_distance [B,N,M], two min, autograd
The scan's rate is given as point-pair evaluations per second, 2 B N M per forward (either direction evaluates every pair),
beside the bound that applies: nine vector instructions per evaluation (three subtractions, three products, two additions, one
minimum; none may fuse) at the fp32 vector rate of 157.3 TFLOP/s / 2 = 78.6 T lane-operations/s.  The 12 bytes per POINT make the
memory bound four orders of magnitude lower.
Last, one training step of DEMTransformer (6 + 6, fp32) at B = 8 x 16 000 with chamfer_weight = 1 against 0, alternating."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd.chamfer import chamfer_packed  # noqa: E402
from scream_amd.geometry import chamfer_distance  # noqa: E402

DEV = "cuda:0"
VECTOR_LANE_OPS_PER_S = 157.3e12 / 2  # the fp32 vector peak counts a fused multiply-add as two
OPS_PER_EVALUATION = 9


def alternate(fns, runs, warmup=3):
    """The callables in turn, run by run, device events around each; one timing dict each."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, f in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ts[k].append(t0.elapsed_time(t1))
    return [dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), runs=runs) for t in ts]


def dense(f, f_):
    """evaluate_open_gf.py:25-41 with utils.square_distance written out."""
    dist = -2 * torch.matmul(f, f_.permute(0, 2, 1))
    dist = dist + torch.sum(f ** 2, -1)[:, :, None]
    dist = dist + torch.sum(f_ ** 2, -1)[:, None, :]
    return torch.mean(torch.min(dist, dim=2)[0], dim=1).mean() + torch.mean(torch.min(dist, dim=1)[0], dim=1).mean()


def shape_case(name, B, N, M, runs):
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.uniform(0, 10, size=(B, N, 3)).astype(np.float32)).to(DEV)
    assert M <= N  # b: the first M points of a, moved by about a neighbour distance (a DEM under its DSM)
    b = a[:, :M] + torch.from_numpy(rng.normal(0, 0.02, size=(B, M, 3)).astype(np.float32)).to(DEV)
    pair = torch.arange(B, device=DEV, dtype=torch.int32)
    rows = (pair * N, torch.full_like(pair, N), pair * M, torch.full_like(pair, M))
    pa, pb = a.reshape(B * N, 3), b.reshape(B * M, 3)

    def packed_fwd():
        return chamfer_packed(pa, rows[0], rows[1], pb, rows[2], rows[3], N, M)

    def packed_fwd_bwd():
        x = pa.detach().requires_grad_()
        chamfer_packed(x, rows[0], rows[1], pb, rows[2], rows[3], N, M).backward()
        return x.grad

    def search_fwd():
        return torch.stack([chamfer_distance(a[i:i + 1], b[i:i + 1]) for i in range(B)]).mean()

    def dense_fwd():
        with torch.no_grad():
            return dense(a, b)

    def dense_fwd_bwd():
        x = a.detach().requires_grad_()
        dense(x, b).backward()
        return x.grad

    res = dict(B=B, N=N, M=M, value_packed=float(packed_fwd()), value_search=float(search_fwd()), value_dense=float(dense_fwd()))
    res["grad_max_abs_diff_packed_dense"] = float((packed_fwd_bwd().reshape(B, N, 3) - dense_fwd_bwd()).abs().max())
    legs = ("packed_fwd", "packed_fwd_bwd", "search_fwd", "dense_fwd", "dense_fwd_bwd")
    for k, t in zip(legs, alternate([packed_fwd, packed_fwd_bwd, search_fwd, dense_fwd, dense_fwd_bwd], runs)):
        res[k] = t
        print("%-8s %-16s median %8.3f ms  (min %.3f, max %.3f, %d runs)" % (name, k, t["median_ms"], t["min_ms"], t["max_ms"], runs))
    evaluations = 2.0 * B * N * M
    res["pair_evaluations_per_forward"] = evaluations
    # (the whole forward: four launches, the scan among them; the scan alone is not timed here)
    res["packed_fwd_pair_evaluations_per_s"] = evaluations / (res["packed_fwd"]["median_ms"] / 1e3)
    res["vector_bound_pair_evaluations_per_s"] = VECTOR_LANE_OPS_PER_S / OPS_PER_EVALUATION
    res["packed_fwd_share_of_vector_bound"] = res["packed_fwd_pair_evaluations_per_s"] / res["vector_bound_pair_evaluations_per_s"]
    res["bound"] = "vector issue (9 instructions per evaluation); the memory bound is (N + M) x 12 bytes per pair"
    res["search_over_packed_fwd"] = res["search_fwd"]["median_ms"] / res["packed_fwd"]["median_ms"]
    res["dense_over_packed_fwd"] = res["dense_fwd"]["median_ms"] / res["packed_fwd"]["median_ms"]
    res["dense_over_packed_fwd_bwd"] = res["dense_fwd_bwd"]["median_ms"] / res["packed_fwd_bwd"]["median_ms"]
    print("%-8s %.3g evaluations/s = %.1f %% of the vector bound; search / packed %.2f, dense / packed %.2f (fwd) %.2f (fwd + bwd)" % (
        name, res["packed_fwd_pair_evaluations_per_s"], 100 * res["packed_fwd_share_of_vector_bound"], res["search_over_packed_fwd"],
        res["dense_over_packed_fwd"], res["dense_over_packed_fwd_bwd"]))
    return res


def step_case(steps, B=8, points=16000):
    from scream_amd.evaluate_open_gf import SyntheticDEM
    from scream_amd.fit import dem_preparer, dem_real_rows, _point_loss
    from scream_amd.model import DEMTransformer
    from scream_amd.optim import FusedAdam
    from scream_amd.synthetic import make_state_dict
    net = DEMTransformer(256, 6, 6)
    net.load_state_dict(make_state_dict(0, 256, 6, 6, dem=True))
    net = net.to(DEV).train()
    opt = FusedAdam(net.parameters(), lr=0.0)  # (the same weights in every step: the two legs do the same work throughout)
    ds = SyntheticDEM(B, 0, points=points)
    prepared = dem_preparer(DEV)([ds[i] for i in range(B)])

    def step(weight):
        def run():
            loss = _point_loss(net, net.forward_packed_train(prepared[0]), prepared, weight, dem_real_rows)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return run

    res = dict(B=B, points=points, layers=(6, 6), train_backend=net.train_backend)
    res["step_weight_0"], res["step_weight_1"] = alternate([step(0.0), step(1.0)], steps, warmup=2)
    res["chamfer_share_of_step"] = 1.0 - res["step_weight_0"]["median_ms"] / res["step_weight_1"]["median_ms"]
    for k in ("step_weight_0", "step_weight_1"):
        print("%-16s median %8.3f ms  (min %.3f, max %.3f, %d steps)" % (k, res[k]["median_ms"], res[k]["min_ms"], res[k]["max_ms"], steps))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step leg")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_bench.py measures on the MI355X; no GPU found")
    res = dict(device=torch.cuda.get_device_name(0), timing="device events, medians after 3 warm-up rounds, legs alternating")
    res["dem"] = shape_case("dem", 8, 16000, 16000, a.runs)
    res["3dmatch"] = shape_case("3dmatch", 32, 5135, 5100, a.runs)
    res["training_step"] = "not measured" if a.no_step else step_case(a.steps)
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
