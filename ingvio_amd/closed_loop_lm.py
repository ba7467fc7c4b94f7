"""In-state SLAM landmarks in the closed loop of the device-resident nominal state (ingvio_landmark_stage_nominal) -
harness code beside ingvio_amd/closed_loop.py, shared by tests/test_gpu_nominal_landmarks.py and tools/closed_loop_bench.py --landmarks:
the loop inputs of closed_loop.make_loop with L real landmarks per filter that stay in view over all frames, the host reference loop in
the reference's order (IngvioFilter.cpp:277-324) built from the host-fed entry points, and the device loop.

The landmarks are points seen from the TRUE camera poses of every frame (synth.make_features over the loop's frame times), anchored to
the window's first clone (make_loop never marginalises it); the table holds their positions with a small error, the prior their 3 x 3
blocks.  Every `outlier_every`-th landmark is grossly off in every third frame (so that both gate verdicts occur), one or two lose track
in some frames."""
import numpy as np

from ingvio_amd.closed_loop import LM, make_loop, nominal_stage, stage_args

CHI2_4, CHI2_2 = 9.487729036781154, 5.991464547107979      # quantile(chi_squared(4 | 2), 0.95), Update.cpp:98-100
LM_NOISE = 0.02


def make_lm_loop(B, n_frames, L=6, F=24, seed=5, outlier_every=4, lm_sigma=0.05, pf_sigma=0.02, noise_px=1e-3, **kw):
    """closed_loop.make_loop with L landmarks per filter plus, per case: "lm_slots" (their table slots, in the order of the observations)
    and per frame "lm_uv" [L][4], "lm_tracked" [L]"""
    from ingvio_amd import synth
    cases = make_loop(B, n_frames, F=F, seed=seed, n_landmarks=L, lm_sigma=lm_sigma, **kw)
    for b, c in enumerate(cases):
        rng = np.random.default_rng(7000 + 13 * seed + b)
        t = c["table"]
        sl = [i for i, s in enumerate(t.slots) if s is not None and s["kind"] == LM]
        assert len(sl) == L
        c["lm_slots"] = sl
        k = c["frames"][0]["imu"].shape[0]
        t0 = 0.1 * (seed + b) + (c["C"] - 1) * synth.IMU_PER_FRAME * synth.IMU_DT      # the time of the table's start state (build_case)
        times = [t0 + (f + 1) * k * synth.IMU_DT for f in range(n_frames)]
        pf, uv, _ = synth.make_features(rng, times, L, noise_px=noise_px, outlier_every=0, pf_sigma=pf_sigma)
        for l, s in enumerate(sl):
            t.slots[s]["p"] = pf[l].copy()
        for f, fr in enumerate(c["frames"]):
            u = uv[:, f, :].copy()
            tr = np.ones(L, dtype=np.uint8)
            if outlier_every and f % 3 == 1:
                for l in range(outlier_every - 1, L, outlier_every):
                    u[l, 0] += 1.0; u[l, 3] -= 0.7
            if f % 5 == 2:
                tr[1 % L] = 0
            if b % 2 and f % 7 == 3:
                tr[4 % L] = 0
            fr["lm_uv"], fr["lm_tracked"] = u, tr
    return cases


def lm_opts(stereo=True, noise=LM_NOISE):
    from ingvio_amd import synth
    Rlr, tlr = synth.t_cl2cr()
    return dict(stereo=stereo, noise=noise, chi2_thr=CHI2_4 if stereo else CHI2_2, R_cl2cr=Rlr, t_cl2cr=tlr)


def host_frames(tabs, cases, f):
    """what ingvio_landmark_stage takes, from the host tables' present values"""
    out = []
    for c, t in zip(cases, tabs):
        e, x = t.slots[t.v_pose], t.slots[t.v_ext]
        lm = [t.slots[s] for s in c["lm_slots"]]
        out.append(dict(R_i2w=e["R"], p_i2w=e["p"], R_cl2i=x["R"], p_c2i=x["p"], idx_epose=e["idx"], idx_ext=x["idx"],
                        lm_idx=[s["idx"] for s in lm], anchor_idx=[t.slots[s["anchor"]]["idx"] for s in lm],
                        pf=np.stack([s["p"] for s in lm]) if lm else np.zeros((0, 3)), uv=c["frames"][f]["lm_uv"],
                        tracked=c["frames"][f]["lm_tracked"]))
    return out


def table_frames(nominal, cases, f, slots=None, uv=None, tracked=None):
    """the same from what ingvio_nominal_get returned (the round-trip form)"""
    out = []
    for b, (nm, c) in enumerate(zip(nominal, cases)):
        sl = c["lm_slots"] if slots is None else slots[b]
        vp, vx = nm["v_pose"], nm["v_ext"]
        out.append(dict(R_i2w=nm["val"][vp, 0:9].reshape(3, 3), p_i2w=nm["val"][vp, 9:12], R_cl2i=nm["val"][vx, 0:9].reshape(3, 3),
                        p_c2i=nm["val"][vx, 9:12], idx_epose=int(nm["idx"][vp]), idx_ext=int(nm["idx"][vx]),
                        lm_idx=[int(nm["idx"][s]) for s in sl], anchor_idx=[int(nm["idx"][nm["anchor"][s]]) for s in sl],
                        pf=nm["val"][sl, 9:12].reshape(-1, 3), uv=c["frames"][f]["lm_uv"] if uv is None else uv[b],
                        tracked=c["frames"][f]["lm_tracked"] if tracked is None else tracked[b]))
    return out


def nominal_frames(cases, f):
    """what ingvio_landmark_stage_nominal takes: slots, observations, tracked flags"""
    return [dict(lm_var=c["lm_slots"], uv=c["frames"][f]["lm_uv"], tracked=c["frames"][f]["lm_tracked"]) for c in cases]


def host_propagate(cases, tabs, f, marg):
    """IMU nominal integration and the new clone on the host tables; -> (steps, track frames) of ingvio_frame_stage_tracks"""
    from oracle import oracle as orc
    steps, tfs = [], []
    for c, t in zip(cases, tabs):
        fr = c["frames"][f]
        e, bg, ba = t.slots[t.v_pose], t.slots[t.v_bg], t.slots[t.v_ba]
        raw = dict(imu=fr["imu"], R=e["R"], p=e["p"], v=e["v"], bg=bg["p"], ba=ba["p"], gravity=t.gravity)
        R, p, v = e["R"], e["p"], e["v"]
        for q in range(fr["imu"].shape[0]):
            R, p, v, _, _ = orc.imu_transition(R, p, v, bg["p"], ba["p"], fr["imu"][q, :3], fr["imu"][q, 3:6], t.gravity, fr["imu"][q, 6])
        e["R"], e["p"], e["v"] = R, p, v
        t.append_clone(fr["new_idx"])
        steps.append(dict(raw=raw, gnss_idx=c["step"]["gnss_idx"], marg_idx=fr["marg"] if marg else -1))
        cl = [t.slots[s] for s in t.clones]
        tfs.append(dict(fr["delta"], clone_idx=[s["idx"] for s in cl], clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl])))
    return steps, tfs


def host_step_lm(ctx, cases, tabs, f, opts):
    """the reference loop from the host-fed entry points, in the reference's order: IMU nominal integration and the new clone on the
    host, ingvio_frame_stage_tracks with host values and NO marginalisation -> run -> fetch -> host boxPlus -> ingvio_landmark_stage with
    the updated values -> run -> fetch -> host boxPlus -> ingvio_marginalize of the frame's clone -> the host table's drop and shift.
    -> ((dx, accept, rows) of the MSCKF update, (dx, rows, accept, gamma, status) of the landmark update)"""
    opts_frame, sigma, eg, scb, srw = stage_args(cases)
    steps, tfs = host_propagate(cases, tabs, f, marg=False)
    ctx.frame_stage_tracks_prepare(0, steps, tfs, opts_frame, sigma, eg, scb, srw)()
    ctx.frame_run()
    frame = ctx.frame_fetch()
    for b, t in enumerate(tabs):
        t.box_plus(frame[0][b])
    ctx.landmark_stage(0, host_frames(tabs, cases, f), opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"], opts["t_cl2cr"])
    ctx.landmark_run()
    lm = ctx.landmark_fetch()
    for b, (c, t) in enumerate(zip(cases, tabs)):
        t.box_plus(lm[0][b])
        ctx.marginalize(b, c["frames"][f]["marg"], 6)
        t.marginalize(c["frames"][f]["marg"])
    return frame, lm


def host_step_lm_prestaged(ctx, cases, tabs, f, opts):
    """the host-fed IN-FRAME landmark stage: the rows are staged before ingvio_frame_run, i.e. linearised at the values the host has
    BEFORE the frame's MSCKF update (not the reference's order).  The host tables are left propagated, not updated."""
    opts_frame, sigma, eg, scb, srw = stage_args(cases)
    steps, tfs = host_propagate(cases, tabs, f, marg=True)
    ctx.frame_stage_tracks_prepare(0, steps, tfs, opts_frame, sigma, eg, scb, srw)()
    ctx.landmark_stage(0, host_frames(tabs, cases, f), opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"], opts["t_cl2cr"],
                       in_frame=True)
    ctx.frame_run()
    return ctx.frame_fetch(), ctx.landmark_fetch()


def lm_stage_call(ctx, cases, f, opts, in_frame=True):
    return ctx.landmark_stage_nominal_prepare(0, nominal_frames(cases, f), opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"],
                                              opts["t_cl2cr"], in_frame=in_frame)


def device_loop_lm(ctx, cases, frames, opts, pipelined):
    """the device loop with the in-frame landmark stage; -> [(frame results, landmark results)] per frame.  pipelined:
    run(i); stage_tracks_nominal(i + 1, async); landmark_stage_nominal(i + 1); fetch_begin(i); run(i + 1); fetch_end(i)
    The landmark results of frame i are fetched between fetch_begin(i) and run(i + 1) (optional for the loop; it synchronises)."""
    out = []
    if not pipelined:
        for f in frames:
            nominal_stage(ctx, cases, f)()
            lm_stage_call(ctx, cases, f, opts)()
            ctx.frame_run()
            out.append((ctx.frame_fetch(), ctx.landmark_fetch()))
        return out
    nominal_stage(ctx, cases, frames[0], use_async=True)()
    lm_stage_call(ctx, cases, frames[0], opts)()
    ctx.frame_run()
    for i, f in enumerate(frames):
        if i + 1 < len(frames):
            nominal_stage(ctx, cases, frames[i + 1], use_async=True)()
            lm_stage_call(ctx, cases, frames[i + 1], opts)()
            ctx.frame_fetch_begin()
            lm = ctx.landmark_fetch()                                    # after stage i + 1: its upload leaves frame i's results alone
            ctx.frame_run()
            out.append((ctx.frame_fetch_end(), lm))
        else:
            out.append((ctx.frame_fetch(), ctx.landmark_fetch()))
    return out
