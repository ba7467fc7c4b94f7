"""Closed-loop batches of the device-resident nominal state (ingvio_nominal_*) - harness code shared by
tests/test_gpu_nominal_*.py and tools/closed_loop_bench.py: inputs of a loop of frames (raw IMU samples, track deltas, the
marginalised clone), the pieces of the host reference that keeps the nominal values with the C oracle's functions and the Var semantics
of oracle/stream_filter.py, and DeviceLoop, the one driver of the device loop.  closed_loop_gnss.py and closed_loop_lm.py add their
inputs, their host reference step and their Form of the driver; closed_loop_update.py the camera frame's second MSCKF update as a frame
entry of its own (UpdateEntry)."""
import numpy as np


SE23, SE3, VEC3, SCALAR, LM, NONE = 0, 1, 2, 3, 4, -1
SIZE = {SE23: 9, SE3: 6, VEC3: 3, SCALAR: 1, LM: 3}


class HostTable:
    """The table as the host keeps it: slots of {kind, idx, anchor slot, R, p, v}; free slots None (the next clone takes the lowest)."""

    def __init__(self, slots, clones, v_ext, v_pose, v_bg, v_ba, gravity):
        self.slots, self.clones = slots, clones
        self.v_ext, self.v_pose, self.v_bg, self.v_ba, self.gravity = v_ext, v_pose, v_bg, v_ba, np.asarray(gravity, dtype=float)

    def as_dict(self):
        n = len(self.slots)
        val = np.zeros((n, 15))
        for i, s in enumerate(self.slots):
            if s is not None:
                val[i, 0:9] = s["R"].reshape(9); val[i, 9:12] = s["p"]; val[i, 12:15] = s["v"]
        return dict(kind=[NONE if s is None else s["kind"] for s in self.slots], idx=[-1 if s is None else s["idx"] for s in self.slots],
                    anchor=[-1 if s is None else s["anchor"] for s in self.slots], val=val, clone_var=list(self.clones), v_ext=self.v_ext,
                    v_pose=self.v_pose, v_bg=self.v_bg, v_ba=self.v_ba, gravity=self.gravity)

    def box_plus(self, dx):                                              # StateManager.cpp:245-251 with the Var.update of each kind
        from oracle import oracle as orc
        for s in self.slots:
            if s is None:
                continue
            i = s["idx"]
            if s["kind"] == SE23:
                s["R"], s["p"], s["v"] = orc.se23_update(s["R"], s["p"], s["v"], dx[i:i + 9])
            elif s["kind"] == SE3:
                s["R"], s["p"] = orc.se3_update(s["R"], s["p"], dx[i:i + 6])
            elif s["kind"] == SCALAR:
                s["p"] = s["p"] + np.array([dx[i], 0.0, 0.0])
            elif s["kind"] == VEC3:
                s["p"] = s["p"] + dx[i:i + 3]
            else:
                a = self.slots[s["anchor"]]["idx"]
                dth = dx[a:a + 3]
                s["p"] = orc.gamma(dth, 0) @ s["p"] + orc.gamma(dth, 1) @ dx[i:i + 3]

    def marginalize(self, idx):                                          # StateManager.cpp:155-192
        drop = next(c for c in self.clones if self.slots[c]["idx"] == idx)
        self.clones = [c for c in self.clones if c != drop]
        self.slots[drop] = None
        for s in self.slots:
            if s is not None and s["idx"] > idx:
                s["idx"] -= 6

    def append_clone(self, idx):
        e, x = self.slots[self.v_pose], self.slots[self.v_ext]
        slot = next((i for i, s in enumerate(self.slots) if s is None), len(self.slots))
        new = dict(kind=SE3, idx=idx, anchor=-1, R=e["R"] @ x["R"], p=e["R"] @ x["p"] + e["p"], v=np.zeros(3))
        if slot == len(self.slots):
            self.slots.append(new)
        else:
            self.slots[slot] = new
        self.clones.append(slot)
        return slot




KS = (1, 9, 10, 33)


def make_loop(B, n_frames, F=24, seed=5, ks=KS, windows=None, n_landmarks=2, lm_sigma=1.0):
    """B filters of ragged windows; per frame and filter the raw IMU samples, the track delta and the marginalised clone (always the
    window's second clone: the first one anchors the landmarks).  Only integers of the state enter the inputs, so they are prepared
    in advance; the host reference keeps the values.  Per frame also "gnss_idx", the clock indices k_propagate takes: the scalars lie
    in front of the clones here, so they never shift."""
    from oracle import oracle as orc
    from ingvio_amd import synth
    cases = []
    for b in range(B):
        C = 5 + b % 7 if windows is None else windows[b % len(windows)]
        flt, step, frame, info = synth.build_case(lambda P, C=C: orc.Cov(P, ld=max(160, 48 + 6 * C)), orc.imu_transition, seed=seed + b, F=8, C=C, n_gnss=6, n_landmarks=n_landmarks,
                                                  lm_sigma=lm_sigma)
        P = flt.cov.P() if callable(flt.cov.P) else flt.cov.P
        raw = step["raw"]
        slots = []

        def add(kind, idx, R=None, p=None, v=None, anchor=-1):
            slots.append(dict(kind=kind, idx=idx, anchor=anchor, R=np.eye(3) if R is None else np.array(R, dtype=float),
                              p=np.zeros(3) if p is None else np.array(p, dtype=float), v=np.zeros(3) if v is None else np.array(v, dtype=float)))
            return len(slots) - 1
        v_pose = add(SE23, 0, raw["R"], raw["p"], raw["v"])
        v_bg, v_ba = add(VEC3, 9, p=raw["bg"]), add(VEC3, 12, p=raw["ba"])
        v_ext = add(SE3, 15, synth.R_CL2I, synth.T_CL2I)
        clone_names = [c["name"] for c in flt.clones]
        lm_vars = []
        for nm, idx, size in flt.vars[4:]:
            if nm.startswith("gnss") or nm == "yof":
                add(SCALAR, idx, p=[0.1 * idx, 0.0, 0.0])
            elif nm.startswith("lm"):
                lm_vars.append((nm, idx))
        clones = []
        for c in flt.clones:
            clones.append(add(SE3, flt.idx_of(c["name"]), c["R"], c["p"]))
        rng = np.random.default_rng(300 + b)
        for nm, idx in lm_vars:
            add(LM, idx, p=synth.true_pose(flt.t)[1] + rng.normal(size=3) * 3.0, anchor=clones[0])
        table = HostTable(slots, clones, v_ext, v_pose, v_bg, v_ba, raw["gravity"])
        k = ks[b % len(ks)]
        t0 = flt.t - len(step["dt"]) * synth.IMU_DT                     # the measured frame of build_case is not used
        times, t = [], t0
        for f in range(n_frames):
            t += k * synth.IMU_DT
            times.append(t)
        pf_true, uv, _ = synth.make_features(rng, times, F, outlier_every=0)
        imus, t = [], t0
        for f in range(n_frames):
            imu = np.zeros((k, 7))
            for q in range(k):
                gy, ac = synth.true_imu(t + synth.IMU_DT)
                imu[q, 0:3] = gy + rng.normal(0, synth.PARAMS["noise_g"], 3)
                imu[q, 3:6] = ac + rng.normal(0, synth.PARAMS["noise_a"], 3)
                imu[q, 6] = synth.IMU_DT
                t += synth.IMU_DT
            imus.append(imu)
        # integer bookkeeping of the window: clone idx list, slot observation flags, the marginalised idx per frame
        cidx = [s["idx"] for s in (slots[c] for c in clones)]
        n = P.shape[0]
        has_obs = [False] * len(cidx)
        frames = []
        for f in range(n_frames):
            drop = [1] if f > 0 else []
            if f > 0:
                del has_obs[1]
            app = len(has_obs)
            has_obs.append(True)
            cidx = cidx + [n]
            marg = cidx[1]
            nobs = sum(has_obs)
            d = dict(drop=drop, append=app, obs_track=list(range(F)), obs_uv=uv[:, f, :],
                     feat_track=list(range(F)) if nobs >= 3 else [], feat_anchor=[app] * F if nobs >= 3 else [],
                     feat_dof=[nobs - 1] * F if nobs >= 3 else [])
            if f == 0:
                d.update(pf_track=list(range(F)), pf=pf_true)
            frames.append(dict(delta=d, imu=imus[f], marg=marg, new_idx=n, gnss_idx=step["gnss_idx"], t=times[f]))
            cidx = [c - 6 if c > marg else c for c in cidx if c != marg]
        cases.append(dict(P=P, table=table, frames=frames, step=step, frame=frame, C=C))
    return cases



def loop_ctx(cases, F, c_max=12):
    from ingvio_amd import capi
    n_max = max(c["P"].shape[0] for c in cases) + 6
    ctx = capi.Context(batch=len(cases), n_max=((n_max + 15) // 16) * 16, c_max=c_max, f_max=F, m_max=64)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c["P"])
    ctx.tracks_create(F)
    return ctx


def stage_args(cases):
    c0 = cases[0]
    st = c0["step"]
    return c0["frame"], st["sigma"], st["enable_gnss"], st["sigma_cb"], st["sigma_rw"]


def first_tri(cases):
    """the cases' first updates triangulate on the device (closed_loop_update.make_update_loop(first_tri=True))"""
    return bool(cases[0].get("first_tri"))


def nominal_stage(ctx, cases, f, use_async=False, enable_gnss=None):
    opts_frame, sigma, eg, scb, srw = stage_args(cases)
    steps = [dict(imu=c["frames"][f]["imu"], gnss_idx=c["frames"][f]["gnss_idx"], marg_idx=c["frames"][f]["marg"]) for c in cases]
    if first_tri(cases):
        return ctx.frame_stage_tracks_nominal_tri_prepare(0, steps, [c["frames"][f]["delta"] for c in cases], opts_frame, sigma,
                                                          eg if enable_gnss is None else enable_gnss, scb, srw, tri={}, use_async=use_async)
    return ctx.frame_stage_tracks_nominal_prepare(0, steps, [c["frames"][f]["delta"] for c in cases], opts_frame, sigma,
                                                  eg if enable_gnss is None else enable_gnss, scb, srw, use_async=use_async)


# ---- the host reference: the pieces every host step is made of ---------------------------------------------------------------------
def host_propagate(cases, tabs, f, marg=True):
    """the host half of a frame: IMU nominal integration (oracle.imu_transition) and the new clone on the host tables; -> (steps, track
    frames) of ingvio_frame_stage_tracks.  marg=False: the frame does not marginalise (the caller does, after its own updates)"""
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
        steps.append(dict(raw=raw, gnss_idx=fr["gnss_idx"], marg_idx=fr["marg"] if marg else -1))
        cl = [t.slots[s] for s in t.clones]
        tfs.append(dict(fr["delta"], clone_idx=[s["idx"] for s in cl], clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl])))
    return steps, tfs


def host_stage(ctx, cases, steps, tfs):
    ctx.frame_stage_tracks_prepare(0, steps, tfs, *stage_args(cases))()


def host_tail(cases, tabs, f, dx, drop=True):
    """boxPlus with an update's dx, then (drop) the marginalised clone's drop and index shift"""
    for b, (c, t) in enumerate(zip(cases, tabs)):
        t.box_plus(dx[b])
        if drop:
            t.marginalize(c["frames"][f]["marg"])


def host_step(ctx, cases, tabs, f):
    """the reference loop: ingvio_frame_stage_tracks with host nominal values, run, fetch, then boxPlus / drop / shift"""
    host_stage(ctx, cases, *host_propagate(cases, tabs, f))
    ctx.frame_run()
    res = ctx.frame_fetch()
    host_tail(cases, tabs, f, res[0])
    return res


# ---- the device loop -----------------------------------------------------------------------------------------------------------------
class UpdateEntry:
    """a frame entry of DeviceLoop that is an update-only frame from the table: the second MSCKF update of camera frame f; tri: its run
    triangulates"""

    def __init__(self, f, tri=True):
        self.f, self.tri = f, tri

    def __repr__(self):
        return "UpdateEntry(%d)" % self.f


class Form:
    """What a form of the loop adds to the frame stage / run / fetch of DeviceLoop; this one, the plain loop, adds nothing.
    late: the form's work on frame i follows that frame's run (after), and the table must see it before frame i + 1 is staged."""
    late = False

    def prepare(self, ctx, cases, f):
        """the form's own stage of frame f as a callable, or None"""
        return None

    def staged(self, loop, i):
        """right after the frame stage of frames[i]"""

    def ran(self, loop, i):
        """right behind the frame_run of frames[i], in front of whatever is enqueued next"""

    def after(self, loop, i):
        """behind the run of frames[i]: serial after its fetch, pipelined right after its fetch_begin"""

    def collect(self, ctx):
        """the form's results of the frame, or None"""
        return None


class DeviceLoop:
    """The device loop of every form, driven frame by frame: start(), then frame(i) for i = 0 .. len(frames) - 1; run() does both.
    The nominal stages refuse when issued out of turn, so the order of the calls is this class and nowhere else:
      serial            stage(i) staged(i) run(i) fetch(i) after(i) collect(i)
      pipelined         start: stage(0) staged(0) run(0), then per frame
                        stage(i+1) staged(i+1) fetch_begin(i) collect(i) run(i+1) fetch_end(i)      (the last frame: fetch(i) collect(i))
      pipelined, late   fetch_begin(i) after(i) stage(i+1) staged(i+1) run(i+1) fetch_end(i) collect(i)
    Right behind every run(i) the form's ran(i) is called (closed_loop_odom.py takes the odometry record there).
    fetch_end(i) is issued after run(i + 1) and still returns frame i's results.  prepare() builds every stage callable ahead of
    the loop (otherwise each is built when it is due), collect=False leaves the form's results unfetched: what the bench tool times.
    sync_every_call (serial): a context synchronisation after every call that only enqueues.
    A frame entry may be an update-only frame from the table (closed_loop_update.py): an UpdateEntry(f) instead of the number f.  It is
    staged with update_stage(ctx, cases, f, use_async) and takes its place in the same sequences; where its run triangulated, its
    results are (dx, accept, rows, pf, tri_ok).  The form's prepare / staged belong to the numbered entries.  Cases whose first updates
    triangulate (first_tri) stage their numbered entries with ingvio_frame_stage_tracks_nominal_tri; those results carry (pf, tri_ok) too."""

    def __init__(self, ctx, cases, frames, form=None, pipelined=True, sync_every_call=False, collect=True, update_stage=None):
        self.ctx, self.cases, self.frames, self.form, self.pipelined = ctx, cases, list(frames), form or Form(), pipelined
        self.sync = ctx.sync if sync_every_call and not pipelined else (lambda: None)
        self.collect = self.form.collect if collect else (lambda ctx: None)
        self.stages, self.form_calls = {}, {}
        self.update_stage = update_stage
        self.staged_hook = None                                          # staged_hook(loop, i): right behind the stage of ANY entry i (tests read the staged frame there)

    def stage_of(self, f):
        if isinstance(f, UpdateEntry):
            return self.update_stage(self.ctx, self.cases, f.f, self.pipelined)
        return nominal_stage(self.ctx, self.cases, f, use_async=self.pipelined)

    def prepare(self):
        for i, f in enumerate(self.frames):
            self.stages[i] = self.stage_of(f)
            self.form_calls[i] = None if isinstance(f, UpdateEntry) else self.form.prepare(self.ctx, self.cases, f)
        return self

    def form_call(self, i):
        return self.form_calls[i] if i in self.form_calls else self.form.prepare(self.ctx, self.cases, self.frames[i])

    def stage(self, i):
        (self.stages.get(i) or self.stage_of(self.frames[i]))()
        self.sync()
        if self.staged_hook:
            self.staged_hook(self, i)
        if not isinstance(self.frames[i], UpdateEntry):
            self.form.staged(self, i)

    def run_entry(self, i):
        self.ctx.frame_run()
        self.form.ran(self, i)

    def start(self):
        if self.pipelined:
            self.stage(0)
            self.run_entry(0)

    def frame(self, i):
        """-> frame i's (dx, accept, rows), with a form that collects: (that, the form's results)"""
        out = self.plain_frame(i)
        e = self.frames[i]
        # (an ordinary entry of a loop whose first updates triangulate carries flags and points as the update-only entry does)
        if e.tri if isinstance(e, UpdateEntry) else first_tri(self.cases):      # (the last fetch_begin was entry i's: its flags and points came along)
            tri = self.ctx.frame_fetch_tri()
            out = (out[0] + tri, out[1]) if len(out) == 2 else out + tri
        return out

    def plain_frame(self, i):
        ctx, form, last = self.ctx, self.form, i + 1 == len(self.frames)
        if self.pipelined and not form.late and not last:
            self.stage(i + 1)
            ctx.frame_fetch_begin()
            res = self.collect(ctx)                                      # after stage i + 1: its upload leaves frame i's results alone
            self.run_entry(i + 1)
            fr = ctx.frame_fetch_end()
            return fr if res is None else (fr, res)
        if not self.pipelined:
            self.stage(i)
            self.run_entry(i)
            self.sync()
            fr = ctx.frame_fetch()
            form.after(self, i)
        elif form.late:
            ctx.frame_fetch_begin()
            form.after(self, i)
            if not last:
                self.stage(i + 1)
                self.run_entry(i + 1)
            fr = ctx.frame_fetch_end()                                   # issued after run(i + 1): still frame i's results
        else:
            fr = ctx.frame_fetch()
        res = self.collect(ctx)
        return fr if res is None else (fr, res)

    def run(self):
        self.start()
        return [self.frame(i) for i in range(len(self.frames))]


def device_loop(ctx, cases, frames, pipelined, form=None, sync_every_call=False):
    return DeviceLoop(ctx, cases, frames, form, pipelined, sync_every_call).run()
