#!/usr/bin/env python3
"""What batch preparation and the packed loss cost on the MI355X, each against the path it replaces, in one process.

    python tools/prep_bench.py [--pairs 32] [--runs 20] [--steps 8] [--train-backend split] [--json profiles/prep_bench.json]

Case 1, preparation of B synthetic 3DMatch-like pairs (scream_amd.synthetic.make_3dmatch_pair: float64, ~5 k points per cloud):
  device        prepare_3dmatch_train on clouds that are on the GPU already (where voxel_down_sample_batch leaves them): the host
                draws B perturbations, four small uploads, five launches, augmentation and noise included
  device+upload the same with the B float64 clouds starting on the host
  host          what the repository offered before: normalize_pair (float64 numpy) per pair and PackedBatch.from_host -- no
                augmentation at all, so the host path does LESS work
  Without augmentation (prepare_3dmatch_val) the two paths are compared first: largest |difference| of the packed coordinates.
Case 2, one training step of PointTransformer (6 + 6) at B pairs, forward + loss + backward + Adam:
  packed        net.loss_packed(pred, prepared)
  stacked       torch.stack([net.loss(...) per pair on batch.unpack_src(pred)]).mean(), tools/train_bench.py's step
  the two alternate step by step on the same model and batch; the loss alone (forward + backward from a detached prediction) is
  timed the same way.
Times are host clocks around work that ends in torch.cuda.synchronize(); medians after warm-up, with minimum and maximum."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd.data import normalize_pair  # noqa: E402
from scream_amd.model import PointTransformer  # noqa: E402
from scream_amd.packing import PackedBatch, StagingBuffers  # noqa: E402
from scream_amd.prep import prepare_3dmatch_train, prepare_3dmatch_val  # noqa: E402
from scream_amd.synthetic import make_3dmatch_pair, make_state_dict  # noqa: E402

DEV = "cuda:0"


def alternate(fns, runs, warmup=2):
    """The callables in turn, run by run; one timing dict each."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return [dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), runs=runs) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--train-backend", choices=("f32", "split"), default="split")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prep_bench.py measures on the MI355X; no GPU found")
    B = a.pairs
    raws = [make_3dmatch_pair(100 + i)[:3] for i in range(B)]
    Ts = np.stack([r[2] for r in raws])
    host_src, host_tgt = [torch.from_numpy(r[0]) for r in raws], [torch.from_numpy(r[1]) for r in raws]
    dev_src, dev_tgt = [t.to(DEV) for t in host_src], [t.to(DEV) for t in host_tgt]
    res = dict(device=torch.cuda.get_device_name(0), pairs=B, mean_points_per_pair=sum(r[0].shape[0] + r[1].shape[0] for r in raws) / B)

    # ---- case 1
    staging = StagingBuffers()

    def host_path():
        items = [normalize_pair(r[0], r[1], r[2]) for r in raws]
        batch, _ = PackedBatch.from_host([i[0] for i in items], [i[1] for i in items], [i[3].reshape(3) for i in items], torch.device(DEV),
                                         staging=staging)
        staging.uploaded()
        return batch

    rng = np.random.default_rng(0)
    ids = list(range(B))
    device_path = lambda: prepare_3dmatch_train(dev_src, dev_tgt, Ts, rng=rng, seed=1, sample_ids=ids)
    upload_path = lambda: prepare_3dmatch_train([t.to(DEV) for t in host_src], [t.to(DEV) for t in host_tgt], Ts, rng=rng, seed=1, sample_ids=ids)
    want, got = host_path(), prepare_3dmatch_val(dev_src, dev_tgt, Ts)
    res["val_against_host_max_abs_diff"] = float((want.xyz - got.batch.xyz).abs().max())
    res["val_against_host_center_max_abs_diff"] = float((want.center - got.batch.center).abs().max())
    res["rows_total"] = got.batch.rows_total
    res["prepare_device"], res["prepare_device_with_upload"], res["prepare_host"] = alternate([device_path, upload_path, host_path], a.runs)
    res["prepare_host_over_device"] = res["prepare_host"]["median_ms"] / res["prepare_device"]["median_ms"]
    res["prepare_host_over_device_with_upload"] = res["prepare_host"]["median_ms"] / res["prepare_device_with_upload"]["median_ms"]
    for k in ("prepare_device", "prepare_device_with_upload", "prepare_host"):
        print("%-28s median %8.3f ms  (min %.3f, max %.3f, %d runs)" % (k, res[k]["median_ms"], res[k]["min_ms"], res[k]["max_ms"], a.runs))

    # ---- case 2
    net = PointTransformer(256, 6, 6)
    net.load_state_dict(make_state_dict(0, 256, 6, 6))
    net.train_backend = a.train_backend
    net = net.to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=2e-4)
    prep = device_path()
    batch = prep.batch
    srcs = [x.clone() for x in batch.unpack_src(batch.xyz[:batch.rows_src])]

    def stacked_loss(pred):
        return torch.stack([net.loss(x[None], s[None], prep.rot[p][None], prep.trans[p][None])
                            for p, (x, s) in enumerate(zip(batch.unpack_src(pred), srcs))]).mean()

    def step(loss_fn):
        def run():
            loss = loss_fn(net.forward_packed_train(batch))
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        return run

    pred0 = net.forward_packed_train(batch).detach()
    a_loss, b_loss = net.loss_packed(pred0, prep), stacked_loss(pred0)
    res["loss_packed"], res["loss_stacked"] = float(a_loss), float(b_loss)

    def loss_only(loss_fn):
        def run():
            p = pred0.clone().requires_grad_(True)
            loss_fn(p).backward()
            return p.grad
        return run

    ga, gb = loss_only(lambda p: net.loss_packed(p, prep))(), loss_only(stacked_loss)()
    res["loss_grad_max_abs_diff"] = float((ga - gb).abs().max())
    res["loss_only_packed"], res["loss_only_stacked"] = alternate([loss_only(lambda p: net.loss_packed(p, prep)), loss_only(stacked_loss)], a.runs)
    res["step_packed"], res["step_stacked"] = alternate([step(lambda p: net.loss_packed(p, prep)), step(stacked_loss)], a.steps)
    res["train_backend"] = a.train_backend
    for k in ("step_packed", "step_stacked"):
        res[k]["pairs_per_s"] = B / (res[k]["median_ms"] / 1e3)
    res["step_stacked_over_packed"] = res["step_stacked"]["median_ms"] / res["step_packed"]["median_ms"]
    for k in ("loss_only_packed", "loss_only_stacked", "step_packed", "step_stacked"):
        print("%-28s median %8.3f ms  (min %.3f, max %.3f, %d runs)" % (k, res[k]["median_ms"], res[k]["min_ms"], res[k]["max_ms"], res[k]["runs"]))
    print("loss packed %.9g stacked %.9g; largest |gradient difference| %.3g" % (res["loss_packed"], res["loss_stacked"], res["loss_grad_max_abs_diff"]))
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
