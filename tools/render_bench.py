#!/usr/bin/env python3
"""Depth renderer (csrc/render.hip) timing against the model's own time for the same input.

    python tools/render_bench.py [--runs 20] [--warmup 3] [--json OUT]

Cases: B = 1 and B = 32 synthetic 3DMatch-like pairs (scream_amd.synthetic.make_3dmatch_pair, normalised as the dataset does)
and one KITTI-size pair (make_kitti_pair), six views at w = 64, rho = 24 (the models' renderer).  Forward (scream_render_depth)
and backward (scream_render_depth_bwd) are timed with HIP events, median of --runs after --warmup.  Reported per case: us per
pair, evaluations per second counting (n + m) w^2 V point-pixel evaluations, and the ratio to the model's time for that input:
the 6 + 6 training step (forward + loss + backward) at B = 1, forward_packed at B = 32.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/render_bench.py` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd import ops  # noqa: E402
from scream_amd.model import PointTransformer  # noqa: E402
from scream_amd.packing import PackedBatch  # noqa: E402
from scream_amd.render import rotation_matrix, view_eulers  # noqa: E402
from scream_amd.synthetic import make_3dmatch_pair, make_kitti_pair, make_state_dict  # noqa: E402

DEV = "cuda:0"
W, RHO = 64, 24


def normalise(src, tgt, T):
    """datasets/three_d_match.py:228-242: the unit ball around the registered union."""
    rot, t = T[:3, :3], T[:3, 3:]
    reg = np.concatenate([(rot @ src.T + t).T, tgt])
    c = reg.mean(0)
    s = 1.0 / np.linalg.norm(reg - c, axis=1).max()
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return f(s * (src - c)), f(s * (tgt - c)), f(rot), f(s * (t - c.reshape(3, 1) + rot @ c.reshape(3, 1)))


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def bench_case(name, pairs, net, runs, warmup, model_kind):
    B = len(pairs)
    batch = PackedBatch.from_pairs([p[0] for p in pairs], [p[1] for p in pairs], [p[3].reshape(3) for p in pairs])
    with torch.no_grad():
        pred = net.eval().forward_packed(batch)  # the renderer's source: the predicted source, as the model renders it
    # the source rows of the batch (src_pred) and the target rows (the second half of xyz), each with its own row offsets
    tgt_rows = batch.xyz[batch.rows_src:]
    t_row0 = (batch.tgt_row0 - batch.rows_src).to(torch.int32).contiguous()
    rot = torch.stack([rotation_matrix(e) for e in view_eulers("muti")]).to(DEV)
    V = rot.shape[0]
    max_s, max_t = max(batch.src_len), max(batch.tgt_len)
    ws = ops.render_workspace(B, V, W, pred.shape[0], DEV)
    s_row0, s_len, t_len = batch.src_row0.contiguous(), batch.src_len_dev.contiguous(), batch.tgt_len_dev.contiguous()
    fwd = lambda: ops.render_depth(pred, s_row0, s_len, tgt_rows, t_row0, t_len, max_s, max_t, rot, W, RHO, ws)
    imgs, amax = fwd()
    up = torch.randn_like(imgs)
    bwd = lambda: ops.render_depth_bwd(up, amax, pred, s_row0, s_len, max_s, rot, W, RHO, ws)
    t_fwd = timed(fwd, runs, warmup)
    fwd()
    t_bwd = timed(bwd, runs, warmup)
    evals = sum(n + m for n, m in zip(batch.src_len, batch.tgt_len)) * W * W * V
    if model_kind == "train":
        net.train()
        opt_free = [p for p in net.parameters()]

        def step():
            p_ = net.forward_packed_train(batch)
            loss = torch.stack([net.loss(x[None], p[0][None], p[2][None], p[3][None])
                                for x, p in zip(batch.unpack_src(p_), pairs)]).mean()
            for q in opt_free:
                q.grad = None
            loss.backward()
        t_model = timed(step, max(3, runs // 4), 1)
        net.eval()
    else:
        def inf():
            with torch.no_grad():
                net.forward_packed(batch)
        t_model = timed(inf, runs, warmup)
    r = dict(case=name, B=B, n=int(np.mean(batch.src_len)), m=int(np.mean(batch.tgt_len)), views=V, w=W,
             fwd_us_per_pair=t_fwd / B, bwd_us_per_pair=t_bwd / B, fwd_evals_per_s=evals / (t_fwd * 1e-6),
             model=("training step" if model_kind == "train" else "forward_packed"), model_us_per_pair=t_model / B,
             fwd_over_model=t_fwd / t_model, fwd_bwd_over_model=(t_fwd + t_bwd) / t_model)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    net = PointTransformer(256, 6, 6)
    net.load_state_dict(make_state_dict(0, 256, 6, 6))
    net = net.to(DEV)
    m3 = lambda seed: normalise(*make_3dmatch_pair(seed)[:3])
    out = [bench_case("3dmatch_b1", [m3(100)], net, a.runs, a.warmup, "train"),
           bench_case("3dmatch_b32", [m3(200 + i) for i in range(32)], net, a.runs, a.warmup, "infer")]
    ks, kt, kT = make_kitti_pair(300)[:3]
    out.append(bench_case("kitti_b1", [normalise(ks, kt, kT)], net, a.runs, a.warmup, "infer"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
