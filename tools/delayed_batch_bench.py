#!/usr/bin/env python3
"""Delayed initialisation of a batch, two forms on the same build and the same inputs:
  batch    one ingvio_add_variable_delayed_batch call for B filters x K candidates
  single   a loop of B x K ingvio_add_variable_delayed calls (four to five stream synchronisations each)
Shape: stereo rows on 11 clones (m = 44, 66 columns), s = 3, N = 249.  The prior is restored from a snapshot before every
repetition; a repetition is timed from its first call to the return of its last (both forms end synchronised); medians over
--reps repetitions after --warmup.  Prints one JSON line.  Both forms are called through ctypes with arguments built ahead of
the timed region.  Only figures of one run are compared with each other.
usage: python tools/delayed_batch_bench.py [--batch 512] [--cands 1,4] [--reps 20] [--warmup 3] [--mode delayed|init]
                                          [--clones C] [--mono] [--form 0|1|2[,..]] [--no-single]
--clones C (--mode delayed): every clone of a window of C observing, m = 4 C (--mono: 2 C) rows on 6 C columns, N = 21 + 6 C + 3 x 54
  beyond 11 clones (the default shape keeps N = 249).  --form: ingvio_set_delayed_form for the batch form; several values (0,2) time the
  batch form once per value on the same context, "batch_form<k>" each.  The loop of single-filter calls runs under mode 0 and is left
  out where the single-filter call cannot take the shape (beyond 22 clones stereo) or with --no-single.
--mode init: landmark initialisation from the track store and the nominal table, two forms on the same build and inputs:
  call        one ingvio_landmark_init_nominal call for B filters x K candidates (rows formed on the device, 40 bytes per candidate)
  round_trip  per candidate: nominal_get -> host rows (numpy, vectorised over the batch) -> ingvio_add_variable_delayed_batch ->
              nominal_set -> nominal_box_plus
Stereo, 11 clones 0.3 m apart, every clone observing; prior and table restored from a snapshot before every repetition.  The call's
arguments are built ahead of the timed region; the round trip's host work (reading the table, the rows, building the blocks, writing
the table back) is what that form consists of and is timed with it.
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


def init_rows(cR, cp, pf, uv, Rlr, tlr):
    """stereo rows of calcResJacobianSingleFeatAllStereoObs for a batch: cR [B,C,3,3], cp [B,C,3], anchor = window position 0"""
    B, Cw = cR.shape[:2]
    RT = cR.transpose(0, 1, 3, 2)
    pc = np.einsum("bcij,bcj->bci", RT, pf - cp)
    sk = np.array([[0.0, -pf[2], pf[1]], [pf[2], 0.0, -pf[0]], [-pf[1], pf[0], 0.0]])
    A = RT @ sk

    def proj(p):
        J = np.zeros((B, Cw, 2, 3))
        J[..., 0, 0] = 1.0 / p[..., 2]; J[..., 1, 1] = 1.0 / p[..., 2]
        J[..., 0, 2] = -p[..., 0] / p[..., 2] ** 2; J[..., 1, 2] = -p[..., 1] / p[..., 2] ** 2
        return J, p[..., :2] / p[..., 2:3]
    pr = pc @ Rlr.T + tlr
    Jl, ul = proj(pc); Jr, ur = proj(pr)
    Jr = Jr @ Rlr
    J = np.concatenate([Jl, Jr], axis=2)                                  # [B,C,4,3]
    Ht, Hf = J @ A, J @ RT
    H_old = np.zeros((B, 4 * Cw, 6 * Cw)); H_new = Hf.reshape(B, 4 * Cw, 3)
    for c in range(Cw):
        H_old[:, 4 * c:4 * c + 4, 6 * c + 3:6 * c + 6] = -Hf[:, c]
        if c:
            H_old[:, 4 * c:4 * c + 4, 6 * c:6 * c + 3] = Ht[:, c]; H_old[:, 4 * c:4 * c + 4, 0:3] = -Ht[:, c]
    res = (uv[None] - np.concatenate([ul, ur], axis=2)).reshape(B, 4 * Cw)
    return H_old, H_new, res


def run_init(a, ks):
    from ingvio_amd import synth
    B, kmax = a.batch, max(ks)
    rng = np.random.default_rng(1)
    A = rng.standard_normal((N, N))
    P0 = 1e-4 * (A @ A.T / N + 0.1 * np.eye(N))
    Rlr, tlr = synth.t_cl2cr()
    ctx = capi.Context(batch=B, n_max=((N + S * kmax + 15) // 16) * 16, c_max=CLONES, f_max=32, m_max=64)
    for b in range(B):
        ctx.cov_set(b, P0)
    ctx.tracks_create(32)
    ctx.nominal_create(32)
    val = np.zeros((4 + CLONES, 15)); val[:, 0] = val[:, 4] = val[:, 8] = 1.0
    for c in range(CLONES):
        val[4 + c, 9] = 0.3 * c
    table = dict(kind=[0, 2, 2, 1] + [1] * CLONES, idx=[0, 9, 12, 15] + [21 + 6 * c for c in range(CLONES)], anchor=[-1] * (4 + CLONES), val=val,
                 clone_var=list(range(4, 4 + CLONES)), v_ext=3, v_pose=0, v_bg=1, v_ba=2, gravity=np.array([0.0, 0.0, -9.8]))
    ctx.nominal_set(0, [table] * B)
    pts = np.stack([np.array([rng.uniform(0.5, 2.5), rng.uniform(-1.0, 1.0), rng.uniform(6.0, 10.0)]) for _ in range(kmax)])
    uv = np.zeros((kmax, CLONES, 4))
    for j in range(kmax):
        for c in range(CLONES):
            pc = pts[j] - val[4 + c, 9:12]; pr = Rlr @ pc + tlr
            uv[j, c] = np.array([pc[0] / pc[2], pc[1] / pc[2], pr[0] / pr[2], pr[1] / pr[2]]) + rng.normal(0.0, 0.02, 4)
    of = dict(stereo=1, R_cl2cr=Rlr, t_cl2cr=tlr, noise=0.08, chi2_table=synth.chi2_table())
    raw = dict(imu=np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 9.8, 0.005]]), R=np.eye(3), p=np.zeros(3), v=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3),
               gravity=np.array([0.0, 0.0, -9.8]))
    for c in range(CLONES):                                               # the store, column by column through its delta
        fr = dict(append=c, obs_track=list(range(kmax)), obs_uv=uv[:, c], clone_idx=[], clone_R=np.zeros((0, 9)), clone_p=np.zeros((0, 3)),
                  feat_track=[], feat_anchor=[], feat_dof=[])
        ctx.frame_stage_tracks_prepare(0, [dict(raw=raw)] * B, [fr] * B, of, [1e-3] * 4)()
    ctx.sync()
    ctx.snapshot()
    tab = synth.chi2_table()
    out = {"tool": "delayed_batch_bench", "mode": "init", "batch": B, "m": M, "s": S, "n": N, "reps": a.reps, "forms": {}}
    for K in ks:
        blocks = [dict(cands=[(j, 0, pts[j]) for j in range(K)], drop=[])] * B

        arr, cap, keep = capi.make_lm_init_blocks(blocks)                  # the call's arguments, built ahead of the timed region
        o, keep_tab = capi.make_opts(of)
        added = np.zeros((B, cap), dtype=np.int32); idx = np.zeros((B, cap), dtype=np.int32); slot = np.zeros((B, cap), dtype=np.int32)
        g = np.zeros((B, cap)); dx = np.zeros((B, cap, ctx.ldp)); st = np.zeros(B, dtype=np.int32)
        pa, pi, psl, pg, pd, ps = capi._i(added), capi._i(idx), capi._i(slot), capi._d(g), capi._d(dx), capi._i(st)
        one = C.c_double(1.0)

        def call():
            rc = ctx.L.ingvio_landmark_init_nominal(ctx.h, 0, B, arr, C.byref(o), one, 1, cap, pa, pi, psl, pg, pd, ps)
            assert rc == 0 and added.all(), rc

        def round_trip():
            for j in range(K):
                dev = ctx.nominal_get()
                cR = np.stack([np.stack([d["val"][s][:9].reshape(3, 3) for s in d["clone_var"]]) for d in dev])
                cp = np.stack([np.stack([d["val"][s][9:12] for s in d["clone_var"]]) for d in dev])
                H_old, H_new, res = init_rows(cR, cp, pts[j], uv[j], Rlr, tlr)
                bl = [[([int(d["idx"][s]) for s in d["clone_var"]], [6] * CLONES, H_old[b], H_new[b], res[b], tab[M])] for b, d in enumerate(dev)]
                got = ctx.add_variable_delayed_batch(0, bl, 0.08)
                dxp = np.zeros((B, ctx.ldp))
                row = np.zeros(15); row[0] = row[4] = row[8] = 1.0; row[9:12] = pts[j]
                for b, d in enumerate(dev):
                    assert got[b][0][0]
                    d["kind"] = np.append(d["kind"], capi.NOM_LANDMARK); d["idx"] = np.append(d["idx"], got[b][1][0])
                    d["anchor"] = np.append(d["anchor"], d["clone_var"][0]); d["val"] = np.vstack([d["val"], row])
                    dxp[b, :len(got[b][3][0])] = got[b][3][0]
                ctx.nominal_set(0, dev)
                ctx.nominal_box_plus(0, dxp)
            ctx.sync()

        res = {}
        for name, fn in (("call", call), ("round_trip", round_trip)):
            ts = []
            for r in range(a.warmup + a.reps):
                ctx.restore(); ctx.sync()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = np.array(ts[a.warmup:])
            res[name] = {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}
        res["ratio_round_trip_over_call"] = res["round_trip"]["median_ms"] / res["call"]["median_ms"]
        out["forms"]["%dx%d" % (B, K)] = res
    ctx.close()
    print(json.dumps(out))


def main():
    global CLONES, M, N
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--cands", default="1,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="delayed", choices=["delayed", "init"])
    ap.add_argument("--clones", type=int, default=CLONES)
    ap.add_argument("--mono", action="store_true")
    ap.add_argument("--form", default="0")
    ap.add_argument("--no-single", action="store_true")
    a = ap.parse_args()
    ks = [int(x) for x in a.cands.split(",")]
    if a.mode == "init":
        return run_init(a, ks)
    B, kmax = a.batch, max(ks)
    forms = [int(x) for x in a.form.split(",")]
    CLONES, M = a.clones, (2 if a.mono else 4) * a.clones
    N = 249 if CLONES <= 11 else 21 + 6 * CLONES + 162
    mu = M - S
    single_fits = 8 * (6 * CLONES * mu + (mu + 1) ** 2) <= 150 * 1024 and not a.no_single
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
    out = {"tool": "delayed_batch_bench", "batch": B, "clones": CLONES, "m": M, "s": S, "n": N, "reps": a.reps, "forms": {}}
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
        runs = [("batch" if forms == [0] else "batch_form%d" % f, batch, f) for f in forms] + ([("single", single, 0)] if single_fits else [])
        for name, fn, form in runs:
            ctx.set_delayed_form(form)
            ts = []
            for r in range(a.warmup + a.reps):
                ctx.restore(); ctx.sync()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = np.array(ts[a.warmup:])
            res[name] = {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}
            if name != "single":
                assert added.all() and (idx[:, K - 1] == N + S * (K - 1)).all()
        if single_fits:
            res["ratio_single_over_batch"] = res["single"]["median_ms"] / res[runs[0][0]]["median_ms"]
        out["forms"]["%dx%d" % (B, K)] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
