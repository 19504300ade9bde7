#!/usr/bin/env python3
"""What the adversarial loss costs on the MI355X: the HIP discriminator (scream_amd/gan.py) against the same network as torch
modules (nn.Conv2d / nn.BatchNorm2d / nn.LeakyReLU: how a GAN step ran before the HIP discriminator), in one process.

    python tools/gan_bench.py [--runs 20] [--images 6,192] [--batches 1,32] [--json profiles/gan_bench.json]

Case 1, the discriminator's three passes of one training step at n images of 2 x 64 x 64: the generator branch (a pass on fake, the
  gradient back to the images) and the discriminator branch (passes on real and on fake, one backward).  Legs: hip, hip again (two
  equal legs: their difference is the spread of the run) and torch; they alternate run by run.
Case 2, one whole training step of the 6 + 6 PointTransformer at B pairs (6 B images per discriminator call): train_epoch without
  the adversarial loss, train_epoch_gan with the torch discriminator, train_epoch_gan with the HIP one (twice).
Times are host clocks around work that ends in torch.cuda.synchronize(); medians after warm-up, with minimum and maximum."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd import FusedAdam  # noqa: E402
from scream_amd.fit import pair_preparer, pair_real_rows, train_epoch, train_epoch_gan  # noqa: E402
from scream_amd.gan import AdversarialLoss, weights_init  # noqa: E402
from scream_amd.model import PointTransformer  # noqa: E402
from scream_amd.synthetic import make_3dmatch_pair, make_state_dict  # noqa: E402

DEV = "cuda:0"


class TorchDiscriminator(nn.Module):
    def __init__(self, input_nc=2, ndf=64):
        super().__init__()
        seq = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(0.2, True)]
        for cin, cout, stride in ((ndf, 2 * ndf, 2), (2 * ndf, 4 * ndf, 2), (4 * ndf, 8 * ndf, 1)):
            seq += [nn.Conv2d(cin, cout, 4, stride, 1, bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.2, True)]
        seq += [nn.Conv2d(8 * ndf, 1, 4, 1, 1)]
        self.main = nn.Sequential(*seq)

    def forward(self, x):
        return self.main(x)


class TorchAdversarialLoss(nn.Module):
    """The same network and losses from torch's own modules; branch 0 differentiates the weights too, as a plain module does."""

    def __init__(self, input_nc=2, ndf=64):
        super().__init__()
        self.discriminator = TorchDiscriminator(input_nc, ndf).apply(weights_init)

    def forward(self, fake, real, optimizer_idx):
        if optimizer_idx == 0:
            return -torch.mean(self.discriminator(fake))
        lr, lf = self.discriminator(real.detach()), self.discriminator(fake.contiguous().detach())
        return 0.5 * (torch.mean(F.relu(1.0 - lr)) + torch.mean(F.relu(1.0 + lf)))


def alternate(fns, runs, warmup=3):
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
    print("%-44s median %9.3f ms  (min %.3f, max %.3f, %d runs)" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["runs"]), flush=True)


def verdict(res, key):
    hip, again, other = (res["%s_%s" % (key, n)]["median_ms"] for n in ("hip", "hip_again", "torch"))
    spread = abs(hip - again)
    res[key + "_spread_ms"] = spread
    res[key + "_hip_no_slower_than_torch_within_spread"] = bool(hip <= other + spread)
    print("%s: hip %.3f ms, torch %.3f ms, spread of two equal legs %.3f ms -> %s" % (
        key, hip, other, spread, "no slower" if hip <= other + spread else "SLOWER by %.3f ms" % (hip - other)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--images", default="6,192")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--json", default=os.path.join("profiles", "gan_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gan_bench.py measures on the MI355X; no GPU found")
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=a.runs)
    names = ("hip", "hip_again", "torch")

    def losses():
        torch.manual_seed(0)
        hip = AdversarialLoss().to(DEV)
        other = TorchAdversarialLoss().to(DEV)
        other.load_state_dict(hip.state_dict())
        again = AdversarialLoss().to(DEV)
        again.load_state_dict(hip.state_dict())
        return hip, again, other

    # ---- case 1: the three passes
    for n in [int(v) for v in a.images.split(",")]:
        gen = torch.Generator(device=DEV).manual_seed(n)
        fake, real = torch.rand(n, 2, 64, 64, device=DEV, generator=gen), torch.rand(n, 2, 64, 64, device=DEV, generator=gen)

        def leg(loss):
            def run():
                x = fake.detach().requires_grad_(True)
                loss(x, None, 0).backward()
                loss.zero_grad()
                loss(fake, real, 1).backward()
            return run

        for name, r in zip(names, alternate([leg(m) for m in losses()], a.runs)):
            res["passes_n%d_%s" % (n, name)] = r
            show("three passes, %d images: %s" % (n, name), r)
        verdict(res, "passes_n%d" % n)

    # ---- case 2: the whole training step
    sd = make_state_dict(0, 256, 6, 6)
    for B in [int(b) for b in a.batches.split(",")]:
        raws = [make_3dmatch_pair(100 + i)[:3] for i in range(B)]
        batch = [[(torch.from_numpy(r[0]), torch.from_numpy(r[1]), torch.from_numpy(r[2])) for r in raws]]

        def leg(loss):
            net = PointTransformer(256, 6, 6)
            net.load_state_dict(sd)
            net = net.to(DEV)
            opt_g = FusedAdam(net.parameters(), lr=2e-4)
            prepare = pair_preparer("3dmatch", True, DEV, seed=1)
            if loss is None:
                return lambda: train_epoch(net, opt_g, batch, prepare)
            opt_d = FusedAdam(loss.parameters(), lr=1e-4, betas=(0.5, 0.999))
            return lambda: train_epoch_gan(net, loss, opt_g, opt_d, batch, prepare, pair_real_rows)

        legs = [leg(m) for m in losses()] + [leg(None)]
        for name, r in zip(names + ("no_gan",), alternate(legs, a.runs)):
            r["pairs_per_s"] = B / (r["median_ms"] / 1e3)
            res["train_step_B%d_%s" % (B, name)] = r
            show("training step B=%d (%d images): %s" % (B, 6 * B, name), r)
        verdict(res, "train_step_B%d" % B)
        del legs
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
