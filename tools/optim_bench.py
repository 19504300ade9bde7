#!/usr/bin/env python3
"""What the optimiser costs on the MI355X: FusedAdam (scream_amd/optim.py) against torch.optim.Adam, in one process.

    python tools/optim_bench.py [--runs 20] [--batches 1,4,32] [--train-backend split] [--json profiles/optim_bench.json]

Case 1, the step alone on the parameters of the 6 + 6 PointTransformer with fixed gradients: FusedAdam, torch.optim.Adam() as
  tools/train_bench.py and the loop tests use it, and torch.optim.Adam(fused=True); the three alternate run by run.
Case 2, one whole training step (forward_packed_train, packed L1 loss, backward, optimiser) at B pairs, with FusedAdam and with
  torch.optim.Adam() on two models of the same weights and the same prepared batch; the two alternate run by run.
Case 3, GradScaler.step + update on the fixed gradients with each of the two.
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
from scream_amd import FusedAdam  # noqa: E402
from scream_amd.model import PointTransformer  # noqa: E402
from scream_amd.prep import prepare_3dmatch_train  # noqa: E402
from scream_amd.synthetic import make_3dmatch_pair, make_state_dict  # noqa: E402

DEV = "cuda:0"


def alternate(fns, runs, warmup=3):
    """The callables in turn, run by run; one timing dict each."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return [dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), runs=runs) for t in ts]


def show(name, r):
    print("%-34s median %8.3f ms  (min %.3f, max %.3f, %d runs)" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["runs"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batches", default="1,4,32")
    ap.add_argument("--train-backend", choices=("f32", "split"), default="split")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py measures on the MI355X; no GPU found")
    sd = make_state_dict(0, 256, 6, 6)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=a.runs, train_backend=a.train_backend)

    # ---- case 1 and 3: the step alone
    gen = torch.Generator(device=DEV).manual_seed(0)
    base = [v.to(DEV) for v in sd.values()]
    grads = [1e-3 * torch.randn(p.shape, device=DEV, generator=gen) for p in base]
    res["tensors"], res["parameters"] = len(base), sum(p.numel() for p in base)

    def fixed(make):
        params = [p.clone().requires_grad_(True) for p in base]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        return make(params)

    opts = dict(fused_adam=fixed(lambda ps: FusedAdam(ps, lr=2e-4)), torch_adam=fixed(lambda ps: torch.optim.Adam(ps, lr=2e-4)),
                torch_adam_fused=fixed(lambda ps: torch.optim.Adam(ps, lr=2e-4, fused=True)))
    names = list(opts)
    for n, r in zip(names, alternate([opts[n].step for n in names], a.runs)):
        res["step_alone_" + n] = r
        show("step alone: " + n, r)
    res["fused_adam_step_not_slower_than_torch_adam"] = res["step_alone_fused_adam"]["median_ms"] <= res["step_alone_torch_adam"]["median_ms"]

    def scaled(opt):
        scaler = torch.amp.GradScaler("cuda")
        one = torch.ones((), device=DEV)

        def run():
            scaler.scale(one)
            scaler.step(opt)
            scaler.update()
        return run

    pair = ("fused_adam", "torch_adam")
    for n, r in zip(pair, alternate([scaled(fixed(lambda ps: FusedAdam(ps, lr=2e-4))), scaled(fixed(lambda ps: torch.optim.Adam(ps, lr=2e-4)))], a.runs)):
        res["grad_scaler_step_" + n] = r
        show("GradScaler step + update: " + n, r)

    # ---- case 2: the whole training step
    for B in [int(b) for b in a.batches.split(",")]:
        raws = [make_3dmatch_pair(100 + i)[:3] for i in range(B)]
        srcs, tgts = [torch.from_numpy(r[0]).to(DEV) for r in raws], [torch.from_numpy(r[1]).to(DEV) for r in raws]
        prep = prepare_3dmatch_train(srcs, tgts, np.stack([r[2] for r in raws]), rng=0, seed=1, sample_ids=list(range(B)))

        def leg(make):
            net = PointTransformer(256, 6, 6)
            net.load_state_dict(sd)
            net.train_backend = a.train_backend
            net = net.to(DEV).train()
            opt = make(net.parameters())

            def run():
                loss = net.loss_packed(net.forward_packed_train(prep.batch), prep)
                opt.zero_grad()
                loss.backward()
                opt.step()
            return run

        legs = [leg(lambda ps: FusedAdam(ps, lr=2e-4)), leg(lambda ps: torch.optim.Adam(ps, lr=2e-4))]
        for n, r in zip(pair, alternate(legs, a.runs)):
            r["pairs_per_s"] = B / (r["median_ms"] / 1e3)
            res["train_step_B%d_%s" % (B, n)] = r
            show("training step B=%d: %s" % (B, n), r)
        res["train_step_B%d_rows_total" % B] = prep.batch.rows_total
        del legs
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
