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
--gnss-in-frame: the epoch staged WITH its frame (ingvio_gnss_frame_stage_nominal) next to the two-call device form above, on the same
build in one run; 8 satellites per filter (--sats) and the GNSS scalars in front of the clones, so that the in-frame update rides on the
MSCKF write-back,
  in-frame form    run(i); stage_async(i+1); gnss_frame_stage_nominal(i+1); fetch_begin(i); run(i+1); fetch_end(i)
Each form free-running (<form>_loop_ms_per_frame) and synchronised per frame (<form>_abi / _wall_ms_per_frame), the two-call form
first, then the in-frame form, then the two-call form again (its spread); writes $RESULTS/closed_loop_bench_gnss_in_frame.json.
--gnss-acquire: no loop - every filter lacks the frequency shift and the four clock biases, and the SPP fix reports all five
(ingvio_amd/closed_loop_gnss_init.py): ONE ingvio_gnss_init_nominal for the batch against the round trip of today's entry points
(host_acquire), --repeats timed rounds of each from the same snapshot; device_ms / roundtrip_ms are the best of them, wall time of
this harness included (for the round trip mostly numpy rows and one ctypes call per candidate).  Writes
$RESULTS/closed_loop_bench_gnss_acquire.json.
--register-only: the loop without epochs but with the GNSS scalars registered, i.e. the clock recursion of k_imu_steps<true> switched on
(against the plain run: that kernel's time with and without registered clocks).
--landmarks L: every filter carries L in-state landmarks that are observed in every frame (ingvio_amd/closed_loop_lm.py), two forms on
the same build,
  device form      run(i); stage_async(i+1); landmark_stage_nominal(i+1, in_frame); fetch_begin(i); run(i+1); fetch_end(i) - the
                   landmark update inside ingvio_frame_run, its inputs from the table
  round-trip form  the plain frame, then ingvio_nominal_get, ingvio_landmark_stage with the table's values, ingvio_landmark_run,
                   ingvio_landmark_fetch, ingvio_nominal_box_plus
measured and reported as the GNSS forms are; writes $RESULTS/closed_loop_bench_lm.json.
--tail: the loop with a real window policy (ingvio_amd/closed_loop_tail.py): the frame is staged without a marginalisation, every filter
carries --landmarks L in-state landmarks (default 20) that are updated in every frame, and behind the frame the OLDEST clone leaves and
ALL landmarks change their anchor to the newest clone, two forms on the same build,
  device form      ... run(i); fetch_begin(i); nominal_tail(i); stage_async(i+1); landmark_stage_nominal(i+1, in_frame); run(i+1) ...
  round-trip form  the tail through the host: ingvio_nominal_get, one ingvio_replace_var_linear per landmark and one ingvio_marginalize
                   per variable and filter, ingvio_nominal_set
measured and reported as the GNSS forms are; writes $RESULTS/closed_loop_bench_tail.json.
--two-updates [--second 40]: both MSCKF updates of the camera callback per camera frame (ingvio_amd/closed_loop_update.py): the first
with --features - --second tracks, the second with --second tracks over three or four selected stamps, triangulated first, marginalising
the frame's clone; two forms on the same build,
  device form      run(i); ustage(i, async); fetch_begin(i); run_u(i); fetch_end(i); stage(i+1, async); ... - the second update an
                   update-only frame from the table and the track store (ingvio_update_stage_tracks_nominal)
  round-trip form  the plain frame, then ingvio_nominal_get, ingvio_msckf_update_tri with tri_masks, ingvio_marginalize, boxPlus / drop /
                   shift on the host, ingvio_nominal_set
the device form free-running (device_loop_ms_per_frame) and both synchronised per camera frame; writes
$RESULTS/closed_loop_bench_two_updates.json.
--two-updates --tri-first: the first update's points found on the device (ingvio_frame_stage_tracks_nominal_tri), both placements of its
triangulation, against the form with host-sent points and the stalling form (main_tri_first); $RESULTS/closed_loop_bench_tri_first.json.
--odom: what the odometry record costs (ingvio_odom_begin / _end, ingvio_amd/closed_loop_odom.py), on one build in one run; the forms
free-running and alternated A B C A B C,
  A  the plain pipelined loop
  B  the loop with the record of every frame, values only:   run(i); odom_begin(i); stage_async(i+1); fetch_begin(i); run(i+1);
  C  the loop with the full record                            odom_end(i); odom_begin(i+1); fetch_end(i)
then C with the record collected in front of run(i+1) (the order of a loop that hands every record out before it launches the next
frame), then the stalling form the record replaces: ingvio_nominal_get plus one ingvio_cov_get_marginal of the pose block per filter
behind every run, timed over --stall-frames frames.  Writes $RESULTS/closed_loop_bench_odom.json.
Writes $RESULTS/closed_loop_bench.json (RESULTS defaults to results/) and prints one JSON line.
usage: python tools/closed_loop_bench.py [--batch 512] [--features 150] [--window 11] [--k 10] [--frames 30] [--warmup 5] [--device-only]
                                         [--gnss | --gnss-in-frame [--sats 8] | --register-only | --landmarks L | --tail [--landmarks L] |
                                          --odom [--repeats 2] [--stall-frames 3]]"""
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


def free_run(out, ctx, cases, form, NF, W):
    """the pipelined device loop free-running, every stage prepared beforehand -> device_loop_ms_per_frame"""
    from ingvio_amd.closed_loop import DeviceLoop
    loop = DeviceLoop(ctx, cases, range(NF), form, collect=False).prepare()
    loop.start()
    for f in range(NF):
        if f == W:
            ctx.sync()
            t0 = time.perf_counter()
        loop.frame(f)
    ctx.sync()
    out["device_loop_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NF - W), 4)


def synced_run(out, name, ctx, cases, form, NF, W):
    """the same loop with a context synchronisation at the end of every frame -> <name>_abi_ms_per_frame, the time inside the
    library's calls, and <name>_wall_ms_per_frame"""
    from ingvio_amd.closed_loop import DeviceLoop
    loop = DeviceLoop(ctx, cases, range(NF), form, collect=False).prepare()
    loop.start()
    ctx.L = TimedLib(ctx.L)
    wall = 0.0
    for f in range(NF):
        ctx.sync()
        if f == W:
            ctx.L.t = 0.0
        t1 = time.perf_counter()
        loop.frame(f)
        ctx.sync()
        if f >= W:
            wall += time.perf_counter() - t1
    out[name + "_abi_ms_per_frame"] = round(1e3 * ctx.L.t / (NF - W), 4)
    out[name + "_wall_ms_per_frame"] = round(1e3 * wall / (NF - W), 4)
    ctx.L = ctx.L._lib


def synced_forms(out, fresh, cases, device_form, roundtrip_form, NF, W, dev_nom):
    """the device and the round-trip form, measured the same way, and how far apart they leave the pose"""
    ctx = fresh()
    synced_run(out, "device", ctx, cases, device_form, NF, W)
    ctx.close()
    ctx = fresh()
    synced_run(out, "roundtrip", ctx, cases, roundtrip_form, NF, W)
    rt_nom = ctx.nominal_get()
    ctx.close()
    out["max_abs_pose_device_vs_roundtrip"] = max(float(np.max(np.abs(d["val"][0] - r["val"][0]))) for d, r in zip(dev_nom, rt_nom))


def finish(out, name=None):
    if name:
        res_dir = os.environ.get("RESULTS", os.path.join(ROOT, "results"))
        os.makedirs(res_dir, exist_ok=True)
        with open(os.path.join(res_dir, name), "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


def fresh_ctx(a, cases, v_max=64, gnss=False, table=True):
    from ingvio_amd import closed_loop as cl
    ctx = cl.loop_ctx(cases, a.features, c_max=a.window + 1)
    if table:
        ctx.nominal_create(v_max)
        ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    if gnss:
        ctx.nominal_set_gnss(0, [c["gnss_slots"] for c in cases])
    return ctx


def main_gnss(a):
    from ingvio_amd import synth
    from ingvio_amd import closed_loop_gnss as cg
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    z = np.load(os.path.join(ROOT, "tests", "golden", "gnss_front.npz"))
    t0 = time.perf_counter()
    cases = cg.make_gnss_loop(z, B, NF, F=F, every=0, ks=(a.k,), windows=(a.window,))
    table = synth.chi2_table()
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, gnss=bool(a.gnss), setup_s=round(time.perf_counter() - t0, 1))
    fresh = lambda: fresh_ctx(a, cases, gnss=True)
    ctx = fresh()
    free_run(out, ctx, cases, cg.GnssForm(table, epochs=a.gnss), NF, W)
    if a.gnss:
        g = ctx.gnss_fetch()
        out["last_epoch_rows_mean"] = float(g[1].mean()); out["last_epoch_ok"] = int((g[4] == 0).sum())
    dev_nom = ctx.nominal_get()
    ctx.close()
    if a.gnss and not a.device_only:
        synced_forms(out, fresh, cases, cg.GnssForm(table), cg.GnssRoundTrip(table), NF, W, dev_nom)
    finish(out, "closed_loop_bench_gnss.json")


def main_gnss_in_frame(a):
    from ingvio_amd import synth
    from ingvio_amd import closed_loop_gnss as cg
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    z = np.load(os.path.join(ROOT, "tests", "golden", "gnss_front.npz"))
    t0 = time.perf_counter()
    cases = cg.make_gnss_loop(z, B, NF, F=F, every=0, ks=(a.k,), windows=(a.window,), scalars_in_front=True, n_sat=a.sats)
    table = synth.chi2_table()
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, sats=a.sats, setup_s=round(time.perf_counter() - t0, 1))
    fresh = lambda: fresh_ctx(a, cases, gnss=True)
    noms = {}
    for name, form in (("two_call", cg.GnssForm), ("in_frame", cg.GnssInFrameForm), ("two_call_again", cg.GnssForm)):
        o = {}
        ctx = fresh()
        free_run(o, ctx, cases, form(table), NF, W)
        out[name + "_loop_ms_per_frame"] = o["device_loop_ms_per_frame"]
        g = ctx.gnss_fetch()
        out[name + "_last_epoch_rows_mean"] = float(g[1].mean()); out[name + "_last_epoch_ok"] = int((g[4] == 0).sum())
        if name == "in_frame":
            out["in_frame_folded"] = ctx.debug_gnss_fused_last() == 2
        noms[name] = ctx.nominal_get()
        ctx.close()
        if not a.device_only:
            ctx = fresh()
            synced_run(out, name, ctx, cases, form(table), NF, W)
            ctx.close()
    out["max_abs_pose_in_frame_vs_two_call"] = max(float(np.max(np.abs(d["val"][0] - r["val"][0]))) for d, r in zip(noms["in_frame"], noms["two_call"]))
    finish(out, "closed_loop_bench_gnss_in_frame.json")


def main_gnss_acquire(a):
    """GnssUpdate::addNewTrackedSys for the whole batch, every filter lacking FS and the four clock biases: ONE ingvio_gnss_init_nominal
    (device form) against closed_loop_gnss_init.host_acquire (ingvio_nominal_get, ingvio_gnss_sat_eval, numpy rows, one
    ingvio_add_variable_delayed per candidate, host boxPlus, ingvio_nominal_set + _set_gnss), on the same build in one process.  Both
    start from the same snapshot; the first call of either form (buffers, code objects) is not timed.  No threshold is set."""
    from ingvio_amd import synth
    from ingvio_amd import closed_loop_gnss_init as ci
    B, F = a.batch, a.features
    z = np.load(os.path.join(ROOT, "tests", "golden", "gnss_front.npz"))
    t0 = time.perf_counter()
    cases = ci.make_init_loop(z, B, 1, [ci.ALL5], F=F, ks=(a.k,), windows=(a.window,))
    table = synth.chi2_table()
    out = dict(batch=B, window=a.window, candidates_per_filter=ci.CAND, satellites=int(len(z["eph"])), repeats=a.repeats, setup_s=round(time.perf_counter() - t0, 1))
    ctx = fresh_ctx(a, cases, gnss=True)
    ctx.snapshot()
    blocks = ci.init_blocks(cases, 0)
    dev, host = [], []
    for it in range(a.repeats + 1):
        call = ctx.gnss_init_nominal_prepare(0, blocks, table, ci.CHI2_MULT, True, False)
        ctx.sync()
        t = time.perf_counter()
        raw = call()                                                     # synchronises once, at its end
        dev.append(time.perf_counter() - t)
        dev_state = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(min(B, 8))])
        ctx.restore()
        cs = ci.fresh(cases)
        ctx.sync()
        t = time.perf_counter()
        ver = ci.host_acquire(ctx, cs, 0, table)
        ctx.sync()
        host.append(time.perf_counter() - t)
        host_state = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(min(B, 8))])
        ctx.restore()
    out["device_ms"] = round(1e3 * min(dev[1:]), 3); out["roundtrip_ms"] = round(1e3 * min(host[1:]), 3)
    out["device_ms_all"] = [round(1e3 * x, 3) for x in dev[1:]]; out["roundtrip_ms_all"] = [round(1e3 * x, 3) for x in host[1:]]
    out["added_device"] = int(raw["added"].sum()); out["added_roundtrip"] = int(sum(v[g]["added"] for v in ver for g in range(ci.CAND)))
    out["max_rel_P_device_vs_roundtrip"] = max(float(np.linalg.norm(d - h) / np.linalg.norm(h)) for d, h in zip(dev_state[1], host_state[1]))
    ctx.close()
    finish(out, "closed_loop_bench_gnss_acquire.json")


def main_landmarks(a):
    from ingvio_amd import closed_loop_lm as clm
    B, F, NF, W, L = a.batch, a.features, a.frames, a.warmup, a.landmarks
    t0 = time.perf_counter()
    cases = clm.make_lm_loop(B, NF, L=L, F=F, ks=(a.k,), windows=(a.window,))
    opts = clm.lm_opts()
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, landmarks=L, setup_s=round(time.perf_counter() - t0, 1))
    fresh = lambda: fresh_ctx(a, cases, v_max=max(64, 32 + L))
    ctx = fresh()
    free_run(out, ctx, cases, clm.LmForm(opts), NF, W)
    lm = ctx.landmark_fetch()
    out["last_frame_lm_rows_mean"] = float(lm[1].mean()); out["last_frame_lm_ok"] = int((lm[4] == 0).sum())
    dev_nom = ctx.nominal_get()
    ctx.close()
    if not a.device_only:
        # (the two forms differ by design: the round trip updates the landmarks after the frame's marginalisation, with rows at the
        # values the frame left; the device form inside the frame, in the reference's order)
        synced_forms(out, fresh, cases, clm.LmForm(opts), clm.LmRoundTrip(opts), NF, W, dev_nom)
    finish(out, "closed_loop_bench_lm.json")


def main_tail(a):
    from ingvio_amd import closed_loop_lm as clm
    from ingvio_amd import closed_loop_tail as clt
    B, F, NF, W, L = a.batch, a.features, a.frames, a.warmup, a.landmarks or 20
    t0 = time.perf_counter()
    cases = clt.make_tail_loop(B, NF, L=L, F=F, mode="sw", behind=False, erase=False, reanchor_all=True, ks=(a.k,), windows=(a.window,))
    opts = clm.lm_opts()
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, landmarks=L, tail=True, setup_s=round(time.perf_counter() - t0, 1))
    fresh = lambda: fresh_ctx(a, cases, v_max=max(64, 32 + L))
    ctx = fresh()
    form = clt.TailForm(opts, cases, fetch_lm=False)
    free_run(out, ctx, cases, form, NF, W)
    out["last_frame_anchor_changes_mean"] = float(np.mean([sum(v) for v in form.out[1]]))
    dev_nom = ctx.nominal_get()
    ctx.close()
    if not a.device_only:
        synced_forms(out, fresh, cases, clt.TailForm(opts, cases, fetch_lm=False), clt.TailRoundTrip(opts, cases), NF, W, dev_nom)
    finish(out, "closed_loop_bench_tail.json")


def main_two_updates(a):
    """both MSCKF updates of the camera callback per camera frame (ingvio_amd/closed_loop_update.py): the first lists
    --features - --second tracks, the second --second tracks over selected stamps with their points triangulated in the run"""
    from ingvio_amd import closed_loop as cl
    from ingvio_amd import closed_loop_update as cu
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    t0 = time.perf_counter()
    cases = cu.make_update_loop(B, NF, F=F, n_lost=F - a.second, carry_point=False, ks=(a.k,), windows=(a.window,))
    out = dict(batch=B, features=F, second=a.second, window=a.window, k=a.k, frames_timed=NF - W, two_updates=True, setup_s=round(time.perf_counter() - t0, 1))
    fresh = lambda: fresh_ctx(a, cases)
    entries = cu.two_update_entries(range(NF))

    def device_run(name, synced):
        ctx = fresh()
        loop = cl.DeviceLoop(ctx, cases, entries, None, collect=False, update_stage=cu.update_stage).prepare()
        loop.start()
        if synced:
            ctx.L = TimedLib(ctx.L)
        wall = 0.0
        for f in range(NF):
            if synced or f == W:
                ctx.sync()
            if f == W:
                t0 = time.perf_counter()
                if synced:
                    ctx.L.t = 0.0
            t1 = time.perf_counter()
            r1, r2 = loop.frame(2 * f), loop.frame(2 * f + 1)
            if synced:
                ctx.sync()
                wall += time.perf_counter() - t1 if f >= W else 0.0
        ctx.sync()
        if synced:
            out[name + "_abi_ms_per_frame"] = round(1e3 * ctx.L.t / (NF - W), 4)
            out[name + "_wall_ms_per_frame"] = round(1e3 * wall / (NF - W), 4)
            ctx.L = ctx.L._lib
        else:
            out[name + "_loop_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NF - W), 4)
            out["last_second_update_rows_mean"] = float(r2[2].mean()); out["last_second_update_tri_ok_mean"] = float((r2[4][:, :a.second] == 1).sum(axis=1).mean())
        nom = ctx.nominal_get()
        ctx.close()
        return nom
    dev_nom = device_run("device", False)
    if not a.device_only:
        device_run("device", True)
        ctx = fresh()
        synced_run(out, "roundtrip", ctx, cases, cu.UpdateRoundTrip(cases, range(NF), a.window + 1), NF, W)
        rt_nom = ctx.nominal_get()
        ctx.close()
        out["max_abs_pose_device_vs_roundtrip"] = max(float(np.max(np.abs(d["val"][0] - r["val"][0]))) for d, r in zip(dev_nom, rt_nom))
    finish(out, "closed_loop_bench_two_updates.json")


def main_tri_first(a):
    """--two-updates --tri-first: what it costs to find the first update's points on the device (ingvio_frame_stage_tracks_nominal_tri), on
    one build in one process, the forms free-running and alternated T0 T1 P T0 T1 P,
      T0 / T1  no point ever handed over, both updates triangulate in their runs; the first update's k_triangulate in front of the gate
               (ingvio_set_first_tri_placement 0) / at the stage behind the gather (1)
      P        the two-update loop with the first update's points sent by the host once (--two-updates as it was)
    then the stalling form a caller without the export is left with: the first update staged without tri, ingvio_nominal_get (both
    streams drained) and ingvio_triangulate on the staged frames (drained again) in front of every first update's run, over
    --stall-frames camera frames - a lower bound for a host-fed triangulation from the values of ingvio_nominal_get, which would also
    upload its frames.  Writes $RESULTS/closed_loop_bench_tri_first.json."""
    from ingvio_amd import closed_loop as cl
    from ingvio_amd import closed_loop_update as cu
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    t0 = time.perf_counter()
    base = cl.make_loop(B, NF, F=F, ks=(a.k,), windows=(a.window,))                      # (one set of inputs, split both ways)
    sent = cu.split_updates(copy.deepcopy(base), F, True, F - a.second, False)
    tri = cu.split_updates(base, F, True, F - a.second, False, first_tri=True)
    out = dict(batch=B, features=F, second=a.second, window=a.window, k=a.k, frames_timed=NF - W, tri_first=True, setup_s=round(time.perf_counter() - t0, 1))
    entries = cu.two_update_entries(range(NF))

    def run(cases, placement, nf=NF, w=W, stall=False):
        ctx = fresh_ctx(a, cases)
        ctx.set_first_tri_placement(placement)

        class Stall(cl.Form):
            def staged(self, loop, i):
                loop.ctx.nominal_get()
                loop.ctx.triangulate(0, None, stereo=True, mask_failed=True)
        loop = cl.DeviceLoop(ctx, cases, entries[:2 * nf], Stall() if stall else None, collect=False, update_stage=cu.update_stage).prepare()
        loop.start()
        for f in range(nf):
            if f == w:
                ctx.sync()
                t1 = time.perf_counter()
            r1, r2 = loop.frame(2 * f), loop.frame(2 * f + 1)
        ctx.sync()
        ms = round(1e3 * (time.perf_counter() - t1) / (nf - w), 4)
        ctx.close()
        return ms, r1
    forms = dict(T0=(tri, 0), T1=(tri, 1), P=(sent, 0))
    if a.device_only:                                                    # the kernel-trace run: the default form alone
        out["T0_ms_per_frame"] = run(tri, 0)[0]
        return finish(out)
    times = {k: [] for k in forms}
    for rep in range(a.repeats):
        for name, (cases, placement) in forms.items():
            ms, r1 = run(cases, placement)
            times[name].append(ms)
            if name == "T0":
                n1 = len(tri[0]["frames"][NF - 1]["delta"]["feat_track"])
                out["last_first_update_listed"] = n1
                out["last_first_update_tri_ok_mean"] = float((r1[4][:, :n1] == 1).sum(axis=1).mean())
                out["last_first_update_rows_mean"] = float(r1[2].mean())
    for name, t in times.items():
        out[name + "_ms_per_frame"] = t
        out[name + "_ms_per_frame_min"] = min(t)
    out["stalling_ms_per_frame"] = run(sent, 0, a.stall_frames + 1, 1, stall=True)[0]
    finish(out, "closed_loop_bench_tri_first.json")


def main_maintain(a):
    """--maintain: the MSCKF anchor change / invalid-feature erase behind every camera frame of the two-update loop with triangulating first
    updates and three decoy tracks per filter (ingvio_amd/closed_loop_maintain.py), on one build in one process, the forms alternated
    N Fc Sc F S R, --repeats times over, every stage prepared beforehand, free-running between two synchronisations:
      N  the loop without maintenance
      F  ingvio_tracks_maintain_begin behind the second update's run, _end behind the next first update's run
      S  the synchronous ingvio_tracks_maintain as a late form
      R  the round trip: ingvio_nominal_get (a synchronisation and every filter's table), the host model on the host's own points; its
         erasures are not sent on (the prepared stages' free_tracks are fixed), so the figure is the download and the model
      Fc / Sc  F and S with the calls' arguments prebuilt, as the stages are: the lists of a first, untimed F run are replayed through
         the C exports with the ctypes blocks and the result buffers made beforehand and no bookkeeping - what the calls themselves
         cost a host that has its lists ready (the loop is deterministic, so the lists are the ones F builds)
    --device-only: form Fc alone (the kernel-trace run).  Writes $RESULTS/closed_loop_bench_maintain.json."""
    from ingvio_amd import closed_loop as cl
    from ingvio_amd import closed_loop_maintain as cm
    from ingvio_amd import closed_loop_update as cu
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    t0 = time.perf_counter()
    cases = cm.add_decoys(cu.make_update_loop(B, NF, F=F, n_lost=F - a.second, carry_point=False, first_tri=True, ks=(a.k,), windows=(a.window,)), F, "sw")
    out = dict(batch=B, features=F, second=a.second, window=a.window, k=a.k, frames_timed=NF - W, maintain=True, setup_s=round(time.perf_counter() - t0, 1))
    entries = cu.two_update_entries(range(NF))

    class RoundTrip(cl.Form):
        late = True

        def __init__(self):
            self.books, self.stores = [cm.Book(c) for c in cases], [cu.HostStore(F + cm.DECOYS, a.window + 1) for _ in cases]

        def staged(self, loop, i):
            for bk in self.books:
                bk.staged()

        def after(self, loop, i):
            e = loop.frames[i]
            if not isinstance(e, cl.UpdateEntry):
                return
            noms = loop.ctx.nominal_get()
            for c, bk, st, nm in zip(cases, self.books, self.stores, noms):
                fr = c["frames"][e.f]
                cm.decoy_points(st, fr)
                cm.host_maintain(cu.host_table_of(nm), st, bk.an, bk.leave(fr), cm.MOVE_MIN_DEPTH["sw"])

    recorded = []                                                        # the blocks of every call, in order (filled by the first F run)

    class Replay(cl.Form):
        def __init__(self, ctx, free):
            import ctypes as C
            self.free, self.late, self.open, self.k = free, not free, False, 0
            self.args = [ctx._maintain_args(blocks, cm.MOVE_MIN_DEPTH["sw"], cm.MIN_DEPTH, None, None) for blocks in recorded]
            cap = max(o.list_cap for _, _, o, _ in self.args)
            self.ver, self.dep, self.lmv = np.zeros((B, cap), dtype=np.uint8), np.zeros((B, cap)), np.zeros((B, 1), dtype=np.uint8)
            ub = C.POINTER(C.c_ubyte)
            self.out = (self.ver.ctypes.data_as(ub), self.dep.ctypes.data_as(C.POINTER(C.c_double)), self.lmv.ctypes.data_as(ub))
            self.byref = C.byref

        def end(self, ctx):
            if self.open:
                ctx._chk(ctx.L.ingvio_tracks_maintain_end(ctx.h, *self.out))
                self.open = False

        def ran(self, loop, i):
            if not self.free:
                return
            ctx = loop.ctx
            self.end(ctx)
            if isinstance(loop.frames[i], cl.UpdateEntry):
                nb, arr, o, _ = self.args[self.k]
                self.k += 1
                ctx._chk(ctx.L.ingvio_tracks_maintain_begin(ctx.h, 0, nb, arr, self.byref(o)))
                self.open = True
                if i + 1 == len(loop.frames):
                    self.end(ctx)

        def after(self, loop, i):
            if self.free or not isinstance(loop.frames[i], cl.UpdateEntry):
                return
            ctx = loop.ctx
            nb, arr, o, _ = self.args[self.k]
            self.k += 1
            ctx._chk(ctx.L.ingvio_tracks_maintain(ctx.h, 0, nb, arr, self.byref(o), *self.out))

    def run(name, record=False):
        ctx = fresh_ctx(a, cases)
        ctx.tracks_create(F + cm.DECOYS)
        verdicts = {}
        if record:
            begin = ctx.tracks_maintain_begin
            ctx.tracks_maintain_begin = lambda b0, blocks, *args, **kw: (recorded.append(blocks), begin(b0, blocks, *args, **kw))[1]
        form = {"N": lambda: None, "R": RoundTrip, "Fc": lambda: Replay(ctx, True), "Sc": lambda: Replay(ctx, False),
                "F": lambda: cm.decoy_form(cases, [cm.Book(c) for c in cases], verdicts, True),
                "S": lambda: cm.decoy_form(cases, [cm.Book(c) for c in cases], verdicts, False)}[name]()
        loop = cl.DeviceLoop(ctx, cases, entries, form, collect=False, update_stage=cu.update_stage).prepare()
        loop.start()
        for f in range(NF):
            if f == W:
                ctx.sync()
                t1 = time.perf_counter()
            loop.frame(2 * f), loop.frame(2 * f + 1)
        ctx.sync()
        ms = round(1e3 * (time.perf_counter() - t1) / (NF - W), 4)
        ctx.close()
        if verdicts:
            v = np.concatenate([np.asarray(x[1]) for per in verdicts.values() for x in per])
            out[name + "_verdict_counts"] = [int(n) for n in np.bincount(v, minlength=5)]
        return ms
    run("F", record=True)                                                # untimed: the lists
    if a.device_only:
        out["Fc_ms_per_frame"] = run("Fc")
        return finish(out)
    names = ("N", "Fc", "Sc", "F", "S", "R")
    times = {k: [] for k in names}
    for rep in range(a.repeats):
        for name in names:
            times[name].append(run(name))
    for name, t in times.items():
        out[name + "_ms_per_frame"] = t
    finish(out, "closed_loop_bench_maintain.json")


def main_odom(a):
    import ctypes
    from ingvio_amd import capi
    from ingvio_amd import closed_loop as cl
    from ingvio_amd.closed_loop_odom import OdomForm
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    t0 = time.perf_counter()
    cases = cl.make_loop(B, NF, F=F, ks=(a.k,), windows=(a.window,))
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, odom=True, setup_s=round(time.perf_counter() - t0, 1))
    forms = dict(A=lambda: None, B=lambda: OdomForm(what=0, dicts=False), C=lambda: OdomForm(what=capi.ODOM_ALL, dicts=False))
    if a.device_only:                                                    # the kernel-trace run: form C alone
        ctx = fresh_ctx(a, cases)
        free_run(out, ctx, cases, forms["C"](), NF, W)
        ctx.close()
        return finish(out)
    times = {k: [] for k in forms}
    last = {}
    for rep in range(a.repeats):
        for name, make in forms.items():
            o, form = {}, make()
            ctx = fresh_ctx(a, cases)
            free_run(o, ctx, cases, form, NF, W)
            times[name].append(o["device_loop_ms_per_frame"])
            if form is not None:
                last[name] = form.finish(ctx)
            ctx.close()
    for name, t in times.items():
        out[name + "_ms_per_frame"] = t
        out[name + "_ms_per_frame_min"] = min(t)
    out["A_spread_ms"] = round(max(times["A"]) - min(times["A"]), 4)
    out["record_bytes"] = ctypes.sizeof(capi.Odom)
    out["last_record_status_or"] = int(np.bitwise_or.reduce(last["C"]["status"]))
    out["values_equal_B_C"] = bool(np.array_equal(last["B"]["p"], last["C"]["p"]) and np.array_equal(last["B"]["R_i2w"], last["C"]["R_i2w"]))

    # C with every record handed out in front of the next run
    ctx = fresh_ctx(a, cases)
    loop = cl.DeviceLoop(ctx, cases, range(NF), OdomForm(what=capi.ODOM_ALL, dicts=False)).prepare()
    loop.start()
    for f in range(NF):
        if f == W:
            ctx.sync()
            t0 = time.perf_counter()
        loop.frame(f)
    ctx.sync()
    out["C_collected_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NF - W), 4)
    ctx.close()

    # the stalling form
    class Stall(cl.Form):
        def ran(self, loop, i):
            nom = loop.ctx.nominal_get()
            self.out = [loop.ctx.marginal(b, [int(q["idx"][q["v_pose"]])], [9]) for b, q in enumerate(nom)]
    NS, WS = a.stall_frames + 1, 1
    ctx = fresh_ctx(a, cases)
    loop = cl.DeviceLoop(ctx, cases, range(NS), Stall()).prepare()
    loop.start()
    for f in range(NS):
        if f == WS:
            ctx.sync()
            t0 = time.perf_counter()
        loop.frame(f)
    ctx.sync()
    out["stalling_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NS - WS), 3)
    ctx.close()
    finish(out, "closed_loop_bench_odom.json")


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
    ap.add_argument("--gnss-in-frame", action="store_true", help="the epoch staged with its frame next to the two-call device form")
    ap.add_argument("--sats", type=int, default=8, help="--gnss-in-frame: satellites per epoch (at most 8 for the fold)")
    ap.add_argument("--gnss-acquire", action="store_true", help="ingvio_gnss_init_nominal for the batch against the round trip through the host (--repeats timed rounds)")
    ap.add_argument("--register-only", action="store_true", help="the loop without epochs, the GNSS scalars registered (clock recursion on)")
    ap.add_argument("--landmarks", type=int, default=0, help="L in-state landmarks per filter, updated in every frame")
    ap.add_argument("--tail", action="store_true", help="the oldest clone leaves and every landmark changes its anchor behind every frame")
    ap.add_argument("--two-updates", action="store_true", help="both MSCKF updates of the camera callback: the second as an update-only frame from the table")
    ap.add_argument("--second", type=int, default=40, help="--two-updates: features of the second update")
    ap.add_argument("--tri-first", action="store_true", help="--two-updates: the first update's points triangulated on the device, against host-sent points and the stalling form")
    ap.add_argument("--maintain", action="store_true", help="the two-update loop with the MSCKF anchor change / invalid-feature erase: free-running, synchronous, round trip, none")
    ap.add_argument("--odom", action="store_true", help="the plain loop against the loop with the odometry record, and the stalling form")
    ap.add_argument("--repeats", type=int, default=2, help="--odom: rounds of A B C")
    ap.add_argument("--stall-frames", type=int, default=3, help="--odom: timed frames of the stalling form")
    a = ap.parse_args()
    if a.gnss_acquire:
        return main_gnss_acquire(a)
    if a.odom:
        return main_odom(a)
    if a.maintain:
        return main_maintain(a)
    if a.two_updates:
        return main_tri_first(a) if a.tri_first else main_two_updates(a)
    if a.tail:
        return main_tail(a)
    if a.landmarks > 0:
        return main_landmarks(a)
    if a.gnss_in_frame:
        return main_gnss_in_frame(a)
    if a.gnss or a.register_only:
        return main_gnss(a)
    from ingvio_amd import closed_loop as cl
    B, F, NF, W = a.batch, a.features, a.frames, a.warmup
    t0 = time.perf_counter()
    cases = cl.make_loop(B, NF, F=F, ks=(a.k,), windows=(a.window,))
    out = dict(batch=B, features=F, window=a.window, k=a.k, frames_timed=NF - W, setup_s=round(time.perf_counter() - t0, 1))

    # device loop, pipelined
    ctx = fresh_ctx(a, cases)
    loop = cl.DeviceLoop(ctx, cases, range(NF)).prepare()
    loop.start()
    dev_res = []
    for f in range(NF):
        if f == W:
            ctx.sync()
            t0 = time.perf_counter()
        dev_res.append(loop.frame(f))
    out["device_loop_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / (NF - W), 4)
    dev_nom = ctx.nominal_get()
    ctx.close()
    timed = range(W, NF)
    out["bytes_per_filter_host"] = round(sum(stage_bytes(cases, f, a.k, True) for f in timed) / (len(timed) * B), 1)
    out["bytes_per_filter_device"] = round(sum(stage_bytes(cases, f, a.k, False) for f in timed) / (len(timed) * B), 1)
    if a.device_only:
        return finish(out)

    # host loop, phase by phase
    ctx = fresh_ctx(a, cases, table=False)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    ph = dict(host_imu=0.0, stage=0.0, run_fetch=0.0, host_box_plus=0.0)
    worst = 0.0
    for f in range(NF):
        t = time.perf_counter()
        steps, tfs = cl.host_propagate(cases, tabs, f)
        t1 = time.perf_counter()
        cl.host_stage(ctx, cases, steps, tfs)
        t2 = time.perf_counter()
        ctx.frame_run()
        dx, acc, rows = ctx.frame_fetch()
        t3 = time.perf_counter()
        cl.host_tail(cases, tabs, f, dx)
        t4 = time.perf_counter()
        if f >= W:
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
    finish(out, "closed_loop_bench.json")


if __name__ == "__main__":
    main()
