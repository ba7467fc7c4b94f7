#!/usr/bin/env python3
"""What mixed batches cost: ms per frame step (ingvio_frame_run(restore_prior), bench.py's timed step) of the default workload
(512 filters, 150 features x 11 clones, nominal state) staged with
  uniform_k10 / uniform_k11   every filter at k = 10 / 11 (k and the noise scalar kernel arguments)
  mixed_k9_11                 k drawn from {9, 10, 11} per filter
  mixed_k1_20                 k drawn from 1 .. 20 per filter
  per_filter_noise            k = 10, sigma / sigma_cb / sigma_rw scaled per filter (ingvio_frame_set_imu_noise)
The steps beyond a filter's 10 measured IMU samples repeat its last one (timing only).  Prints one JSON line.
usage: python tools/mixed_batch_bench.py [--batch 512] [--steps 50] [--warmup 5] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def with_k(step, k):
    idx = [min(s, len(step["dt"]) - 1) for s in range(k)]
    return dict(step, Phi=[step["Phi"][s] for s in idx], G=[step["G"][s] for s in idx], dt=[step["dt"][s] for s in idx])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="timed blocks per batch kind, interleaved over the kinds")
    args = ap.parse_args()
    import bench
    from ingvio_amd import capi, synth
    B, F, C, n_gnss, n_lm = args.batch, 150, 11, 6, 52
    N = 21 + n_gnss + 3 * n_lm + 6 * C
    ctx = capi.Context(batch=B, n_max=((N + 15) // 16) * 16, c_max=C, f_max=F, m_max=64)
    filters, steps, frames, _ = bench.build_batch(ctx, B, 0, F, C, n_gnss, n_lm)
    ctx.snapshot()
    pr = synth.PARAMS
    sigma, scb, srw = filters[0].sigma(), pr["sigma_cb"], pr["sigma_rw"]
    rng = np.random.default_rng(5)
    kinds = {
        "uniform_k10": ([10] * B, None),
        "uniform_k11": ([11] * B, None),
        "mixed_k9_11": (rng.integers(9, 12, B).tolist(), None),
        "mixed_k1_20": (rng.integers(1, 21, B).tolist(), None),
        "per_filter_noise": ([10] * B, [list(np.asarray(sigma) * f) + [scb * f, srw * f] for f in rng.uniform(0.5, 2.0, B)]),
    }
    # the staged inputs of each kind, built once (the host packing is not what is measured)
    stagers = {}
    for name, (ks, noise) in kinds.items():
        stagers[name] = (ctx.frame_stage_prepare(0, [with_k(steps[b], ks[b]) for b in range(B)], frames, sigma, filters[0].enable_gnss,
                                                 scb, srw, max_accept=0, compress_rule=1), noise)
    times = {name: [] for name in kinds}
    for rep in range(args.repeats):
        for name, (stage, noise) in stagers.items():
            stage()
            if noise is not None:
                ctx.frame_set_imu_noise(0, noise)
            for _ in range(args.warmup):
                ctx.frame_run(restore_prior=True)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.frame_run(restore_prior=True)
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    ctx.close()
    out = dict(batch=B, feats=F, clones=C, steps=args.steps, repeats=args.repeats,
               ms_per_step={n: round(float(np.median(v)), 4) for n, v in times.items()},
               ms_per_step_all={n: [round(x, 4) for x in v] for n, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
