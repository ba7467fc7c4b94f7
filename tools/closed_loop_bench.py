#!/usr/bin/env python3
"""What closing the filter loop costs: a batch of filters (default 512, 150 features x 11 clones, k = 10) runs the same
closed loop of frames twice,
  host loop    per frame: ingvio_frame_stage_tracks with the host's nominal values, ingvio_frame_run, ingvio_frame_fetch, then boxPlus,
               the marginalisation's index shift and the IMU nominal integration on the host (ingvio_amd/closed_loop.py: the C oracle's
               functions, one call per variable - the Python reference, not an optimised host)
  device loop  the nominal state on the device (ingvio_frame_stage_tracks_nominal), pipelined:
               run(i); stage_async(i+1); fetch_begin(i); run(i+1); fetch_end(i)
and reports ms per frame (the host loop split into its phases), the bytes one filter's frame hand-over takes in each mode, and whether
the two loops agree.  --device-only runs the device loop alone (the rocprofv3 --kernel-trace --stats run for the kernels' times).
--gnss: every filter also takes a raw GNSS epoch (the 11 usable satellites of tests/golden/gnss_front.npz) per frame, and two forms of the
device loop are timed on the same build,
  device form      run(i); fetch_begin(i); gnss_front_stage_nominal(i); gnss_run(i); stage_async(i+1); run(i+1); fetch_end(i)
  round-trip form  the epoch through the host: ingvio_nominal_get, ingvio_gnss_front_stage with the table's values, ingvio_gnss_run,
                   ingvio_gnss_fetch, ingvio_nominal_box_plus (three synchronisations per epoch)
Both forms run the same way - a context synchronisation at the end of every frame, so that a frame's time is its own - and both are
reported twice: *_abi_ms_per_frame, the time spent INSIDE the library's calls (what a compiled host would pay), and
*_wall_ms_per_frame with this harness' Python between the calls (for the round-trip form mostly the conversion of 512 fetched tables
into epoch structures).  device_loop_ms_per_frame is the device form free-running, without the per-frame synchronisation.  The GNSS
modes write $RESULTS/closed_loop_bench_gnss.json.
--register-only: the loop without epochs but with the GNSS scalars registered, i.e. the clock recursion of k_imu_steps<true> switched on
(against the plain run: that kernel's time with and without registered clocks).
--landmarks L: every filter carries L in-state landmarks that are observed in every frame (ingvio_amd/closed_loop_lm.py), two forms on
the same build,
  device form      run(i); stage_async(i+1); landmark_stage_nominal(i+1, in_frame); fetch_begin(i); run(i+1); fetch_end(i) - the
                   landmark update inside ingvio_frame_run, its inputs from the table
  round-trip form  the plain frame, then ingvio_nominal_get, ingvio_landmark_stage with the table's values, ingvio_landmark_run,
                   ingvio_landmark_fetch, ingvio_nominal_box_plus
measured and reported as the GNSS forms are; writes $RESULTS/closed_loop_bench_lm.json.
Writes $RESULTS/closed_loop_bench.json (RESULTS defaults to results/) and prints one JSON line.
usage: python tools/closed_loop_bench.py [--batch 512] [--features 150] [--window 11] [--k 10] [--frames 30] [--warmup 5] [--device-only]
                                         [--gnss | --register-only | --landmarks L]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stage_bytes(cases, f, k, host):
    """bytes of frame f's upload slab, by the layout frame_stage_tracks_impl (capi.hip) gives it: the [B][32]-int headers, then the int,
    mask and double pools, each padded to 64 bytes.  Per filter: drop / free / obs / pf tracks, the clone table (host values only: the
    window with the new clone), the features and 5 clock indices as ints; obs uv (4), points (3), clone poses (12, host values only), IMU
    samples (7 k) and the start state (24, host values only) as doubles, rounded up to 4"""
    def pad(b):
        return (b + 63) & ~63
    ni = nd = 0
    for c in cases:
        d = c["frames"][f]["delta"]
        nct = c["C"] if host else 0
        n_obs, n_pf = len(d.get("obs_track", [])), len(d.get("pf_track", []))
        ni += len(d.get("drop", [])) + len(d.get("free", [])) + n_obs + n_pf + nct + len(d["feat_track"]) + 5
        od = 4 * n_obs + 3 * n_pf + 12 * nct + 7 * k + (24 if host else 0)
        nd += (od + 3) & ~3
    return pad(4 * len(cases) * 32) + pad(4 * ni) + pad(8 * nd)


class TimedLib:
    """the loaded library with the time spent inside its calls summed up (the round-trip form's figure: ABI calls only)"""

    def __init__(self, lib):
        self._lib, self.t = lib, 0.0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            t0 = time.perf_counter()
            r = fn(*args)
            self.t += time.perf_counter() - t0
            return r
        return call


def main_gnss(a):
    from ingvio_amd import synth
    from ingvio_amd import closed_loop as cl
    from ingvio_amd import closed_loop_gnss as cg
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    z = np.load(os.path.join(ROOT, "tests", "golden", "gnss_front.npz"))
    t0 = time.perf_counter()
    cases = cg.make_gnss_loop(z, B, NF, F=F, every=0, ks=(a.k,), windows=(a.window,))
    table = synth.chi2_table()
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, gnss=bool(a.gnss), setup_s=round(time.perf_counter() - t0, 1))

    def fresh():
        ctx = cl.loop_ctx(cases, F, c_max=a.window + 1)
        ctx.nominal_create(64)
        ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
        ctx.nominal_set_gnss(0, [c["gnss_slots"] for c in cases])
        return ctx

    # device form
    ctx = fresh()
    stages = [cg.nominal_stage(ctx, cases, f, use_async=True) for f in range(NF)]
    gst = [cg.gnss_stage_call(ctx, cases, f, table) for f in range(NF)] if a.gnss else None
    stages[0]()
    ctx.frame_run()
    for f in range(NF):
        if f == W:
            ctx.sync()
            t0 = time.perf_counter()
        ctx.frame_fetch_begin()
        if a.gnss:
            gst[f]()
            ctx.gnss_run()
        if f + 1 < NF:
            stages[f + 1]()
            ctx.frame_run()
        ctx.frame_fetch_end()
    ctx.sync()
    out["device_loop_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NF - W), 4)
    if a.gnss:
        g = ctx.gnss_fetch()
        out["last_epoch_rows_mean"] = float(g[1].mean()); out["last_epoch_ok"] = int((g[4] == 0).sum())
    dev_nom = ctx.nominal_get()
    ctx.close()
    if a.gnss and not a.device_only:
        # device form once more, measured exactly as the round-trip form below: synchronised per frame, time inside the calls and wall
        ctx = fresh()
        stages = [cg.nominal_stage(ctx, cases, f, use_async=True) for f in range(NF)]
        gst = [cg.gnss_stage_call(ctx, cases, f, table) for f in range(NF)]
        stages[0]()
        ctx.frame_run()
        ctx.L = TimedLib(ctx.L)
        wall = 0.0
        for f in range(NF):
            ctx.sync()
            if f == W:
                ctx.L.t = 0.0
            t1 = time.perf_counter()
            ctx.frame_fetch_begin()
            gst[f]()
            ctx.gnss_run()
            if f + 1 < NF:
                stages[f + 1]()
                ctx.frame_run()
            ctx.frame_fetch_end()
            ctx.sync()
            if f >= W:
                wall += time.perf_counter() - t1
        out["device_abi_ms_per_frame"] = round(1e3 * ctx.L.t / (NF - W), 4)
        out["device_wall_ms_per_frame"] = round(1e3 * wall / (NF - W), 4)
        ctx.L = ctx.L._lib
        ctx.close()
        # round-trip form
        ctx = fresh()
        stages = [cg.nominal_stage(ctx, cases, f, use_async=True) for f in range(NF)]
        stages[0]()
        ctx.frame_run()
        ctx.L = TimedLib(ctx.L)
        wall = 0.0
        for f in range(NF):
            ctx.sync()
            if f == W:
                ctx.L.t = 0.0
            t1 = time.perf_counter()
            ctx.frame_fetch_begin()
            nom = ctx.nominal_get()                                      # synchronises both streams
            ctx.gnss_front_stage_prepare(0, cg.table_epochs(nom, cases, f), table, gate_rows=True, strong_reject=True)()
            ctx.gnss_run()
            g = ctx.gnss_fetch()                                         # synchronises
            ctx.nominal_box_plus(0, g[0])
            if f + 1 < NF:
                stages[f + 1]()
                ctx.frame_run()
            ctx.frame_fetch_end()
            ctx.sync()
            if f >= W:
                wall += time.perf_counter() - t1
        abi = ctx.L.t
        ctx.L = ctx.L._lib
        out["roundtrip_abi_ms_per_frame"] = round(1e3 * abi / (NF - W), 4)
        out["roundtrip_wall_ms_per_frame"] = round(1e3 * wall / (NF - W), 4)
        rt_nom = ctx.nominal_get()
        ctx.close()
        out["max_abs_pose_device_vs_roundtrip"] = max(float(np.max(np.abs(dev_nom[b]["val"][0] - rt_nom[b]["val"][0]))) for b in range(B))
    res_dir = os.environ.get("RESULTS", os.path.join(ROOT, "results"))
    os.makedirs(res_dir, exist_ok=True)
    with open(os.path.join(res_dir, "closed_loop_bench_gnss.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main_landmarks(a):
    from ingvio_amd import closed_loop as cl
    from ingvio_amd import closed_loop_lm as clm
    B, F, NF, W, L = a.batch, a.features, a.frames, a.warmup, a.landmarks
    t0 = time.perf_counter()
    cases = clm.make_lm_loop(B, NF, L=L, F=F, ks=(a.k,), windows=(a.window,))
    opts = clm.lm_opts()
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, landmarks=L, setup_s=round(time.perf_counter() - t0, 1))

    def fresh():
        ctx = cl.loop_ctx(cases, F, c_max=a.window + 1)
        ctx.nominal_create(max(64, 32 + L))
        ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
        return ctx

    def device_form(ctx, timed_lib):
        stages = [cl.nominal_stage(ctx, cases, f, use_async=True) for f in range(NF)]
        lms = [clm.lm_stage_call(ctx, cases, f, opts) for f in range(NF)]
        stages[0](); lms[0]()
        ctx.frame_run()
        if timed_lib:
            ctx.L = TimedLib(ctx.L)
        wall, t0 = 0.0, 0.0
        for f in range(NF):
            if timed_lib or f == W:
                ctx.sync()
            if f == W:
                t0 = time.perf_counter()
                if timed_lib:
                    ctx.L.t = 0.0
            t1 = time.perf_counter()
            if f + 1 < NF:
                stages[f + 1](); lms[f + 1]()
                ctx.frame_fetch_begin()
                ctx.frame_run()
                ctx.frame_fetch_end()
            else:
                ctx.frame_fetch()
            if timed_lib:
                ctx.sync()
                if f >= W:
                    wall += time.perf_counter() - t1
        ctx.sync()
        free = time.perf_counter() - t0
        abi = ctx.L.t if timed_lib else 0.0
        if timed_lib:
            ctx.L = ctx.L._lib
        return free, abi, wall

    ctx = fresh()
    free, _, _ = device_form(ctx, False)
    out["device_loop_ms_per_frame"] = round(1e3 * free / (NF - W), 4)
    lm = ctx.landmark_fetch()
    out["last_frame_lm_rows_mean"] = float(lm[1].mean()); out["last_frame_lm_ok"] = int((lm[4] == 0).sum())
    dev_nom = ctx.nominal_get()
    ctx.close()
    if not a.device_only:
        ctx = fresh()
        _, abi, wall = device_form(ctx, True)
        out["device_abi_ms_per_frame"] = round(1e3 * abi / (NF - W), 4)
        out["device_wall_ms_per_frame"] = round(1e3 * wall / (NF - W), 4)
        ctx.close()
        # round-trip form
        ctx = fresh()
        stages = [cl.nominal_stage(ctx, cases, f, use_async=True) for f in range(NF)]
        stages[0]()
        ctx.frame_run()
        ctx.L = TimedLib(ctx.L)
        wall = 0.0
        for f in range(NF):
            ctx.sync()
            if f == W:
                ctx.L.t = 0.0
            t1 = time.perf_counter()
            ctx.frame_fetch_begin()
            nom = ctx.nominal_get()                                      # synchronises both streams
            ctx.landmark_stage(0, clm.table_frames(nom, cases, f), opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"], opts["t_cl2cr"])
            ctx.landmark_run()
            lm = ctx.landmark_fetch()                                    # synchronises
            ctx.nominal_box_plus(0, lm[0])
            if f + 1 < NF:
                stages[f + 1]()
                ctx.frame_run()
            ctx.frame_fetch_end()
            ctx.sync()
            if f >= W:
                wall += time.perf_counter() - t1
        abi = ctx.L.t
        ctx.L = ctx.L._lib
        out["roundtrip_abi_ms_per_frame"] = round(1e3 * abi / (NF - W), 4)
        out["roundtrip_wall_ms_per_frame"] = round(1e3 * wall / (NF - W), 4)
        rt_nom = ctx.nominal_get()
        ctx.close()
        # (the two forms differ by design: the round trip updates the landmarks after the frame's marginalisation, with rows at the
        # values the frame left; the device form inside the frame, in the reference's order)
        out["max_abs_pose_device_vs_roundtrip"] = max(float(np.max(np.abs(dev_nom[b]["val"][0] - rt_nom[b]["val"][0]))) for b in range(B))
    res_dir = os.environ.get("RESULTS", os.path.join(ROOT, "results"))
    os.makedirs(res_dir, exist_ok=True)
    with open(os.path.join(res_dir, "closed_loop_bench_lm.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--features", type=int, default=150)
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--gnss", action="store_true")
    ap.add_argument("--register-only", action="store_true", help="the loop without epochs, the GNSS scalars registered (clock recursion on)")
    ap.add_argument("--landmarks", type=int, default=0, help="L in-state landmarks per filter, updated in every frame")
    a = ap.parse_args()
    if a.landmarks > 0:
        return main_landmarks(a)
    if a.gnss or a.register_only:
        return main_gnss(a)
    from oracle import oracle as orc
    from ingvio_amd import closed_loop as cl
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    t0 = time.perf_counter()
    cases = cl.make_loop(B, NF, F=F, ks=(a.k,), windows=(a.window,))
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, setup_s=round(time.perf_counter() - t0, 1))

    # device loop, pipelined
    ctx = cl.loop_ctx(cases, F, c_max=a.window + 1)
    ctx.nominal_create(64)
    ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    calls = [cl.nominal_stage(ctx, cases, f, use_async=True) for f in range(NF)]
    calls[0]()
    ctx.frame_run()
    dev_res = []
    for f in range(NF):
        if f == W:
            ctx.sync()
            t0 = time.perf_counter()
        if f + 1 < NF:
            calls[f + 1]()
            ctx.frame_fetch_begin()
            ctx.frame_run()
            dev_res.append(ctx.frame_fetch_end())
        else:
            dev_res.append(ctx.frame_fetch())
    out["device_loop_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NF - W), 4)
    dev_nom = ctx.nominal_get()
    ctx.close()
    timed = range(W, NF)
    out["bytes_per_filter_host"] = round(sum(stage_bytes(cases, f, a.k, True) for f in timed) / (len(timed) * B), 1)
    out["bytes_per_filter_device"] = round(sum(stage_bytes(cases, f, a.k, False) for f in timed) / (len(timed) * B), 1)
    if a.device_only:
        print(json.dumps(out))
        return

    # host loop, phase by phase
    ctx = cl.loop_ctx(cases, F, c_max=a.window + 1)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    opts_frame, sigma, eg, scb, srw = cl.stage_args(cases)
    ph = dict(host_imu=0.0, stage=0.0, run_fetch=0.0, host_box_plus=0.0)
    worst = 0.0
    for f in range(NF):
        timed = f >= W
        t = time.perf_counter()
        steps, tfs = [], []
        for c, tb in zip(cases, tabs):
            fr = c["frames"][f]
            e, bg, ba = tb.slots[tb.v_pose], tb.slots[tb.v_bg], tb.slots[tb.v_ba]
            raw = dict(imu=fr["imu"], R=e["R"], p=e["p"], v=e["v"], bg=bg["p"], ba=ba["p"], gravity=tb.gravity)
            R, p, v = e["R"], e["p"], e["v"]
            for q in range(fr["imu"].shape[0]):
                R, p, v, _, _ = orc.imu_transition(R, p, v, bg["p"], ba["p"], fr["imu"][q, :3], fr["imu"][q, 3:6], tb.gravity, fr["imu"][q, 6])
            e["R"], e["p"], e["v"] = R, p, v
            tb.append_clone(fr["new_idx"])
            steps.append(dict(raw=raw, gnss_idx=c["step"]["gnss_idx"], marg_idx=fr["marg"]))
            clo = [tb.slots[s] for s in tb.clones]
            tfs.append(dict(fr["delta"], clone_idx=[s["idx"] for s in clo], clone_R=np.stack([s["R"] for s in clo]),
                            clone_p=np.stack([s["p"] for s in clo])))
        t1 = time.perf_counter()
        ctx.frame_stage_tracks_prepare(0, steps, tfs, opts_frame, sigma, eg, scb, srw)()
        t2 = time.perf_counter()
        ctx.frame_run()
        dx, acc, rows = ctx.frame_fetch()
        t3 = time.perf_counter()
        for b, (c, tb) in enumerate(zip(cases, tabs)):
            tb.box_plus(dx[b])
            tb.marginalize(c["frames"][f]["marg"])
        t4 = time.perf_counter()
        if timed:
            ph["host_imu"] += t1 - t; ph["stage"] += t2 - t1; ph["run_fetch"] += t3 - t2; ph["host_box_plus"] += t4 - t3
        d = dev_res[f][0]
        worst = max(worst, float(np.max(np.abs(d - dx)) / max(np.max(np.abs(dx)), 1e-300)))
    ctx.close()
    for key in ph:
        out["host_loop_ms_" + key] = round(1e3 * ph[key] / (NF - W), 3)
    out["host_loop_ms_per_frame"] = round(sum(out["host_loop_ms_" + key] for key in ph), 3)
    out["max_rel_dx_device_vs_host"] = worst
    out["max_rel_pose_device_vs_host"] = max(float(np.max(np.abs(dev_nom[b]["val"][tabs[b].v_pose] - tabs[b].as_dict()["val"][tabs[b].v_pose])))
                                             for b in range(B))
    res_dir = os.environ.get("RESULTS", os.path.join(ROOT, "results"))
    os.makedirs(res_dir, exist_ok=True)
    with open(os.path.join(res_dir, "closed_loop_bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
