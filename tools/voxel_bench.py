#!/usr/bin/env python3
"""voxel_down_sample (csrc/voxel.hip) timing against the host restatement on the same data.

    python tools/voxel_bench.py [--runs 20] [--warmup 3] [--json profiles/voxel_down_sample.json]

Legs: "3dmatch" 32 + 32 seeded clouds of 200 k points at 0.0625 m (raw fragments of a batch of pairs), "kitti" 8 + 8 clouds of
120 k points at 0.3 m.  Per leg, on the GPU: the kernels alone (ops.voxel_down_sample_packed on packed rows: no packing, no
copy of the lengths) and the public call (voxel_down_sample_batch: packing, launches, the one device-to-host copy, slicing),
HIP events, median of --runs after --warmup; on the host: scream_amd.evaluate_open_gf.voxel_down_sample on the same clouds over
16 worker processes.  The GPU result of the first cloud is compared bit for bit with the host restatement of its fp32 points
before anything is timed.  Each GPU leg runs in a child process of its own under a time limit; a leg that fails ends the run.
Bytes per pass: see docs/design/small_kernels.md; kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats -- python tools/voxel_bench.py --leg kitti --no-host`."""
import argparse
import json
import os
import subprocess
import sys
import time
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"3dmatch": dict(clouds=64, points=200000, voxel=0.0625), "kitti": dict(clouds=16, points=120000, voxel=0.3)}
LEG_TIMEOUT_S = 300
HOST_WORKERS = 16


def make_cloud(leg, seed):
    n = LEGS[leg]["points"]
    rng = np.random.default_rng(seed)
    if leg == "3dmatch":  # a 3 m room: most points on its faces, the rest clutter inside
        p = rng.uniform(-1.5, 1.5, size=(n, 3))
        face = rng.random(n) < 0.8
        axis = rng.integers(0, 3, size=n)
        wall = np.where(rng.random(n) < 0.5, -1.5, 1.5) + rng.normal(0, 0.004, size=n)
        p[np.arange(n)[face], axis[face]] = wall[face]
    else:  # a LiDAR sweep: 120 m across, ground and objects within 4 m of height
        r = rng.uniform(2.0, 60.0, size=n)
        a = rng.uniform(0, 2 * np.pi, size=n)
        p = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 2.0, size=n)], axis=1)
    return np.ascontiguousarray(p, dtype=np.float32)


def _host_one(args):
    from scream_amd.evaluate_open_gf import voxel_down_sample
    cloud, voxel = args
    return voxel_down_sample(cloud.astype(np.float64), voxel).shape[0]


def host_leg(leg):
    """Wall time of the host restatement on the leg's clouds over HOST_WORKERS processes (the fp32 clouds are handed to the
    workers inside the timed window: 2.4 MB each)."""
    jobs = [(make_cloud(leg, 1000 + i), LEGS[leg]["voxel"]) for i in range(LEGS[leg]["clouds"])]
    with Pool(HOST_WORKERS) as pool:
        pool.map(_host_one, [(j[0][:1000], j[1]) for j in jobs[:HOST_WORKERS]])  # start the workers, import the package
        t0 = time.perf_counter()
        voxels = pool.map(_host_one, jobs, chunksize=1)
        t1 = time.perf_counter()
    return dict(host_ms=(t1 - t0) * 1e3, host_workers=HOST_WORKERS, voxels_total=int(sum(voxels)))


def gpu_leg(leg, runs, warmup):
    import torch
    from scream_amd import ops
    from scream_amd.evaluate_open_gf import voxel_down_sample as host_voxel_down_sample
    from scream_amd.voxel import voxel_down_sample_batch
    assert torch.cuda.is_available(), "voxel_bench needs the MI355X"
    cfg = LEGS[leg]
    B, n, voxel = cfg["clouds"], cfg["points"], cfg["voxel"]
    host_clouds = [make_cloud(leg, 1000 + i) for i in range(B)]
    clouds = [torch.from_numpy(c).to("cuda:0") for c in host_clouds]
    xyz = torch.cat(clouds).contiguous()
    row0 = (torch.arange(B, dtype=torch.int32) * n).to("cuda:0")
    length = torch.full((B,), n, dtype=torch.int32).to("cuda:0")
    vox = torch.full((B,), voxel, dtype=torch.float64).to("cuda:0")
    first = voxel_down_sample_batch(clouds, voxel)[0].cpu().numpy()
    want = host_voxel_down_sample(host_clouds[0].astype(np.float64), voxel).astype(np.float32)
    assert first.shape == want.shape and np.array_equal(first.view(np.uint32), want.view(np.uint32)), "GPU result differs from the host's"

    def timed(fn):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    k = timed(lambda: ops.voxel_down_sample_packed(xyz, row0, length, n, vox))
    c = timed(lambda: voxel_down_sample_batch(clouds, voxel))
    return dict(leg=leg, clouds=B, points_per_cloud=n, voxel=voxel, runs=runs, voxels_first_cloud=int(first.shape[0]),
                kernels_ms=k[0], kernels_ms_min=k[1], kernels_ms_max=k[2], call_ms=c[0], call_ms_min=c[1], call_ms_max=c[2],
                points_per_s_kernels=B * n / (k[0] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run this GPU leg in this process and print its JSON line")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.leg:
        print("RESULT " + json.dumps(gpu_leg(a.leg, a.runs, a.warmup)), flush=True)
        return 0
    out = []
    for leg in ("3dmatch", "kitti"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--runs", str(a.runs), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print("leg %s ran into its time limit: stopping" % leg, file=sys.stderr)
            return 1
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print("leg %s failed (exit %d): stopping\n%s" % (leg, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        row = json.loads(lines[-1][len("RESULT "):])
        if not a.no_host:
            row.update(host_leg(leg))
            row["host_over_gpu_call"] = row["host_ms"] / row["call_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
