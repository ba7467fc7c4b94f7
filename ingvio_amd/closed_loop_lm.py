"""In-state SLAM landmarks in the closed loop of the device-resident nominal state (ingvio_landmark_stage_nominal) -
harness code beside ingvio_amd/closed_loop.py, shared by tests/test_gpu_nominal_landmarks.py and tools/closed_loop_bench.py --landmarks:
the loop inputs of closed_loop.make_loop with L real landmarks per filter that stay in view over all frames, the host reference loop in
the reference's order (IngvioFilter.cpp:277-324) built from the host-fed entry points, and the loop's two forms for
closed_loop.DeviceLoop (the in-frame stage from the table, the update through the host).

The landmarks are points seen from the TRUE camera poses of every frame (synth.make_features over the loop's frame times), anchored to
the window's first clone (make_loop never marginalises it); the table holds their positions with a small error, the prior their 3 x 3
blocks.  Every `outlier_every`-th landmark is grossly off in every third frame (so that both gate verdicts occur), one or two lose track
in some frames."""
import numpy as np

from ingvio_amd.closed_loop import LM, Form, device_loop, host_propagate, host_stage, host_tail, make_loop

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


def nominal_frames(cases, f):
    """what ingvio_landmark_stage_nominal takes: slots, observations, tracked flags"""
    return [dict(lm_var=c["lm_slots"], uv=c["frames"][f]["lm_uv"], tracked=c["frames"][f]["lm_tracked"]) for c in cases]


def staged_frames(nominal, staged):
    """what ingvio_landmark_stage takes, from tables in the layout of ingvio_nominal_get / HostTable.as_dict() and what
    ingvio_landmark_stage_nominal takes (nominal_frames; None: a filter that stages nothing)"""
    out = []
    for nm, s in zip(nominal, staged):
        sl = [] if s is None else list(s["lm_var"])
        vp, vx = nm["v_pose"], nm["v_ext"]
        out.append(dict(R_i2w=nm["val"][vp, 0:9].reshape(3, 3), p_i2w=nm["val"][vp, 9:12], R_cl2i=nm["val"][vx, 0:9].reshape(3, 3),
                        p_c2i=nm["val"][vx, 9:12], idx_epose=int(nm["idx"][vp]), idx_ext=int(nm["idx"][vx]),
                        lm_idx=[int(nm["idx"][v]) for v in sl], anchor_idx=[int(nm["idx"][nm["anchor"][v]]) for v in sl],
                        pf=nm["val"][sl, 9:12].reshape(-1, 3), uv=np.zeros((0, 4)) if s is None else s["uv"],
                        tracked=np.zeros(0, dtype=np.uint8) if s is None else s["tracked"]))
    return out


def table_frames(nominal, cases, f, slots=None, uv=None, tracked=None):
    """staged_frames for frame f of the loop; slots / uv / tracked [B]: other landmarks or observations than the loop's"""
    staged = nominal_frames(cases, f)
    for b, s in enumerate(staged):
        s.update({k: v[b] for k, v in (("lm_var", slots), ("uv", uv), ("tracked", tracked)) if v is not None})
    return staged_frames(nominal, staged)


def host_frames(tabs, cases, f):
    return table_frames([t.as_dict() for t in tabs], cases, f)


def host_lm_stage(ctx, frames, opts, in_frame=False):
    ctx.landmark_stage(0, frames, opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"], opts["t_cl2cr"], in_frame=in_frame)


def host_step_lm(ctx, cases, tabs, f, opts):
    """the reference loop from the host-fed entry points, in the reference's order: IMU nominal integration and the new clone on the
    host, ingvio_frame_stage_tracks with host values and NO marginalisation -> run -> fetch -> host boxPlus -> ingvio_landmark_stage with
    the updated values -> run -> fetch -> host boxPlus -> ingvio_marginalize of the frame's clone -> the host table's drop and shift.
    -> ((dx, accept, rows) of the MSCKF update, (dx, rows, accept, gamma, status) of the landmark update)"""
    host_stage(ctx, cases, *host_propagate(cases, tabs, f, marg=False))
    ctx.frame_run()
    frame = ctx.frame_fetch()
    host_tail(cases, tabs, f, frame[0], drop=False)
    host_lm_stage(ctx, host_frames(tabs, cases, f), opts)
    ctx.landmark_run()
    lm = ctx.landmark_fetch()
    for b, c in enumerate(cases):
        ctx.marginalize(b, c["frames"][f]["marg"], 6)
    host_tail(cases, tabs, f, lm[0])
    return frame, lm


def host_step_lm_prestaged(ctx, cases, tabs, f, opts):
    """the host-fed IN-FRAME landmark stage: the rows are staged before ingvio_frame_run, i.e. linearised at the values the host has
    BEFORE the frame's MSCKF update (not the reference's order).  The host tables are left propagated, not updated."""
    host_stage(ctx, cases, *host_propagate(cases, tabs, f))
    host_lm_stage(ctx, host_frames(tabs, cases, f), opts, in_frame=True)
    ctx.frame_run()
    return ctx.frame_fetch(), ctx.landmark_fetch()


def lm_stage_call(ctx, cases, f, opts, in_frame=True):
    return ctx.landmark_stage_nominal_prepare(0, nominal_frames(cases, f), opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"],
                                              opts["t_cl2cr"], in_frame=in_frame)


class LmForm(Form):
    """the in-frame landmark stage from the table, right behind the frame stage it belongs to; the frame's run applies it.  The
    landmark results of frame i are fetched between fetch_begin(i) and run(i + 1) (optional for the loop; it synchronises)."""

    def __init__(self, opts):
        self.opts = opts

    def prepare(self, ctx, cases, f):
        return lm_stage_call(ctx, cases, f, self.opts)

    def staged(self, loop, i):
        loop.form_call(i)()

    def collect(self, ctx):
        return ctx.landmark_fetch()


class LmRoundTrip(Form):
    """the plain frame, then the update through the host: ingvio_nominal_get, ingvio_landmark_stage with the table's values,
    ingvio_landmark_run, ingvio_landmark_fetch, ingvio_nominal_box_plus"""
    late = True

    def __init__(self, opts):
        self.opts = opts

    def after(self, loop, i):
        ctx = loop.ctx
        nom = ctx.nominal_get()                                          # synchronises both streams
        host_lm_stage(ctx, table_frames(nom, loop.cases, loop.frames[i]), self.opts)
        ctx.landmark_run()
        lm = ctx.landmark_fetch()                                        # synchronises
        ctx.nominal_box_plus(0, lm[0])


def device_loop_lm(ctx, cases, frames, opts, pipelined):
    """the device loop with the in-frame landmark stage; -> [(frame results, landmark results)] per frame"""
    return device_loop(ctx, cases, frames, pipelined, LmForm(opts))
