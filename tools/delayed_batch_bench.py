#!/usr/bin/env python3
"""Delayed initialisation of a batch, two forms on the same build and the same inputs:
  batch    one ingvio_add_variable_delayed_batch call for B filters x K candidates
  single   a loop of B x K ingvio_add_variable_delayed calls (four to five stream synchronisations each)
Shape: stereo rows on 11 clones (m = 44, 66 columns), s = 3, N = 249.  The prior is restored from a snapshot before every
repetition; a repetition is timed from its first call to the return of its last (both forms end synchronised); medians over
--reps repetitions after --warmup.  Prints one JSON line.  Both forms are called through ctypes with arguments built ahead of
the timed region.  Only figures of one run are compared with each other.
usage: python tools/delayed_batch_bench.py [--batch 512] [--cands 1,4] [--reps 20] [--warmup 3]
The two GPU steps of a measurement, each under its own time limit, the second only after the first has ended well (the kernel
times of both forms come from the SEPARATE traced run; its wall times are not used):
  timeout -k 10 400 python tools/delayed_batch_bench.py > delayed_bench.json &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d delayed_trace -o dl -- python tools/delayed_batch_bench.py --reps 2 --warmup 1
then read delayed_trace/**/dl_kernel_stats.csv: k_delayed_front / k_ekf_core / k_downdate per round of the batch form against
k_delayed_qr + k_gamma + k_delayed_add (+ k_ekf_core + k_downdate) per call of the single form."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ingvio_amd import capi  # noqa: E402

CLONES, M, S, N, NOISE = 11, 44, 3, 249, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--cands", default="1,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ks = [int(x) for x in a.cands.split(",")]
    B, kmax = a.batch, max(ks)
    rng = np.random.default_rng(1)
    A = rng.standard_normal((N, N))
    P0 = 1e-2 * (A @ A.T / N + 0.1 * np.eye(N))
    ctx = capi.Context(batch=B, n_max=((N + S * kmax + 15) // 16) * 16, c_max=CLONES, f_max=32, m_max=64)
    for b in range(B):
        ctx.cov_set(b, P0)
    ctx.snapshot()
    vidx = [21 + 6 * i for i in range(CLONES)]; vsize = [6] * CLONES
    from scipy.stats import chi2
    chk = float(chi2.ppf(0.95, M))
    cands = [(vidx, vsize, rng.standard_normal((M, 6 * CLONES)), rng.standard_normal((M, S)), 0.05 * rng.standard_normal(M), chk)
             for _ in range(kmax)]
    L, h = ctx.L, ctx.h
    out = {"tool": "delayed_batch_bench", "batch": B, "m": M, "s": S, "n": N, "reps": a.reps, "forms": {}}
    for K in ks:
        arr, cap, keep = capi.make_delayed_blocks([cands[:K]] * B)
        added = np.zeros((B, cap), dtype=np.int32); idx = np.zeros((B, cap), dtype=np.int32); g = np.zeros((B, cap))
        dx = np.zeros((B, cap, ctx.ldp)); st = np.zeros(B, dtype=np.int32)
        pa, pi, pg, pd, ps = capi._i(added), capi._i(idx), capi._d(g), capi._d(dx), capi._i(st)
        noise, one = C.c_double(NOISE), C.c_double(1.0)

        def batch():
            rc = L.ingvio_add_variable_delayed_batch(h, 0, B, arr, noise, one, 1, cap, pa, pi, pg, pd, ps)
            assert rc == 0, rc

        q = arr[0].cand
        dx1 = np.zeros(ctx.ldp); a1 = C.c_int(0); i1 = C.c_int(0); g1 = C.c_double(0.0)
        pd1, chk_c = capi._d(dx1), C.c_double(chk)

        def single():
            for b in range(B):
                for j in range(K):
                    c = q[j]
                    rc = L.ingvio_add_variable_delayed(h, b, c.vidx, c.vsize, c.k, c.H_old, c.ldh, c.H_new, c.ldn, c.m, c.s, c.res, noise, one, 1,
                                                       chk_c, pd1, C.byref(a1), C.byref(i1), C.byref(g1))
                    assert rc == 0 and a1.value == 1, (rc, a1.value)

        res = {}
        for name, fn in (("batch", batch), ("single", single)):
            ts = []
            for r in range(a.warmup + a.reps):
                ctx.restore(); ctx.sync()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = np.array(ts[a.warmup:])
            res[name] = {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}
            if name == "batch":
                assert added.all() and (idx[:, K - 1] == N + S * (K - 1)).all()
        res["ratio_single_over_batch"] = res["single"]["median_ms"] / res["batch"]["median_ms"]
        out["forms"]["%dx%d" % (B, K)] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
