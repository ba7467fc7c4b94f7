"""GNSS epochs in the closed loop of the device-resident nominal state (ingvio_nominal_set_gnss, ingvio_gnss_front_stage_nominal, DESIGN
4.11) - harness code beside ingvio_amd/closed_loop.py, shared by tests/test_gpu_nominal_gnss.py and tools/closed_loop_bench.py --gnss:
the loop inputs of closed_loop.make_loop with receiver clocks in the table and one raw GNSS epoch per filter and frame, the host
reference (clock recursion of ImuPropagator.cpp:139-148, host-fed front, host boxPlus) and the loop's forms for
closed_loop.DeviceLoop (epochs from the table behind the frame, epochs from the table inside the frame, epochs through the host).

The satellite data is one recorded instant (tests/golden/gnss_front.npz) while the synthetic trajectory moves, so every epoch is made
consistent with the filter's TRUE state of its frame: the anchor maps the true position onto the fixture's evaluation point (plus a few
metres), and pseudo-ranges / Dopplers are shifted by the difference between the oracle's residuals at that true state (position,
velocity, clocks that drift with the true frequency shift) and at the fixture's own true state - the fixture's measurement noise stays."""
import numpy as np

from ingvio_amd.closed_loop import SCALAR, Form, device_loop, host_step, make_loop
from ingvio_amd.closed_loop import nominal_stage  # noqa: F401  (the GNSS loop's stage is the plain one: it reads the frame's own clock indices)

C_LIGHT = 2.99792458e8
LAT, LON = np.deg2rad(31.0), np.deg2rad(121.4)
R_ENU = np.array([[-np.sin(LON), -np.sin(LAT) * np.cos(LON), np.cos(LAT) * np.cos(LON)],
                  [np.cos(LON), -np.sin(LAT) * np.sin(LON), np.cos(LAT) * np.sin(LON)], [0.0, np.cos(LAT), np.sin(LAT)]])
NO_EPH, NO_OBS = np.zeros((0, 25)), np.zeros((0, 6))


def rot_z(yaw):
    return np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])


def gnss_slots(case):
    """table slots of the clock biases GPS, GLO, GAL, BDS, FS, YOF (-1: none) of a make_loop case"""
    t, gi = case["table"], list(case["step"]["gnss_idx"])
    by_idx = {s["idx"]: i for i, s in enumerate(t.slots) if s is not None and s["kind"] == SCALAR}
    sl = [by_idx.get(i, -1) if i >= 0 else -1 for i in gi]
    rest = [i for i in by_idx.values() if i not in sl]
    return sl + [rest[0] if rest else -1]


def move_scalars_behind_clones(c):
    """make_loop appends the window's clones behind the GNSS scalars, so no marginalisation ever moves a scalar's idx.  Here the six
    scalars go to the END of the state (P permuted, every idx of the table and of the frames renumbered): the clones of the start window
    lie in front of them, and each of their marginalisations shifts the scalars by 6 - what a GNSS epoch must see in the table.
    Per frame: "marg", "new_idx" and "gnss_idx" (the clock indices k_propagate takes, valid at that frame's start)."""
    t, P = c["table"], c["P"]
    n = P.shape[0]
    sc = sorted(s["idx"] for s in t.slots if s is not None and s["kind"] == SCALAR)
    lo, ns = sc[0], len(sc)
    assert sc == list(range(lo, lo + ns))
    new_of = lambda i: i if i < lo else (n - ns + (i - lo) if i < lo + ns else i - ns)
    order = list(range(lo)) + list(range(lo + ns, n)) + list(range(lo, lo + ns))
    c["P"] = np.ascontiguousarray(P[np.ix_(order, order)])
    for s in t.slots:
        if s is not None:
            s["idx"] = new_of(s["idx"])
    c["step"] = dict(c["step"], gnss_idx=[new_of(i) if i >= 0 else -1 for i in c["step"]["gnss_idx"]])
    cidx = [t.slots[v]["idx"] for v in t.clones]
    g = list(c["step"]["gnss_idx"])
    for fr in c["frames"]:
        cidx = cidx + [n]
        marg = cidx[1]
        fr["marg"], fr["new_idx"], fr["gnss_idx"] = marg, n, list(g)
        cidx = [x - 6 if x > marg else x for x in cidx if x != marg]
        g = [x - 6 if x > marg else x for x in g]


def make_gnss_loop(z, B, n_frames, F=24, seed=5, every=3, scalars_in_front=False, n_sat=None, cases=None, **kw):
    """closed_loop.make_loop plus, per case: "gnss_slots", the table's clocks initialised from the fixture (xyzt[3:] plus noise, FS from
    velt[3], YOF = the epoch's yaw), and "epochs" [n_frames]: the host-owned part of a raw epoch (dict) or None; filter b has epochs
    unless b % every == every - 1 (every = 0: all filters).
    scalars_in_front: the GNSS scalars stay where make_loop puts them, in front of the clones - no marginalisation moves them, which is
    what lets an in-frame epoch ride on the MSCKF write-back (ingvio_gnss_frame_stage_nominal).  n_sat: every epoch keeps its first n_sat
    satellites only.  cases: the loop the epochs are added to (built with the same seed and F) instead of make_loop(B, n_frames, ...)."""
    from oracle import oracle as orc
    from ingvio_amd import synth
    if cases is None:
        cases = make_loop(B, n_frames, F=F, seed=seed, **kw)
    doy = float(z["doy"])
    base = orc.gnss_residuals(z["eph"], z["obs"], z["ion"], doy, np.r_[z["rcv_true"], z["cb_true"]], np.r_[z["vel_true"], z["fs_true"]])
    for b, c in enumerate(cases):
        rng = np.random.default_rng(900 + b)
        if not scalars_in_front:
            move_scalars_behind_clones(c)
        sl = gnss_slots(c)
        c["gnss_slots"] = sl
        yaw = 0.3 + 0.01 * b
        t = c["table"]
        for s in range(4):
            if sl[s] >= 0:
                t.slots[sl[s]]["p"] = np.array([z["xyzt"][3 + s] + rng.normal(0, 1.0), 0.0, 0.0])
        t.slots[sl[4]]["p"] = np.array([float(z["velt"][3]), 0.0, 0.0])
        t.slots[sl[5]]["p"] = np.array([yaw, 0.0, 0.0])
        k = c["frames"][0]["imu"].shape[0]
        t0 = 0.1 * (seed + b) + (c["C"] - 1) * synth.IMU_PER_FRAME * synth.IMU_DT      # the time of the table's start state (build_case)
        Rw = R_ENU @ rot_z(yaw)
        c["epochs"] = []
        for f in range(n_frames):
            if every and b % every == every - 1:
                c["epochs"].append(None)
                continue
            el = (f + 1) * k * synth.IMU_DT
            _, p_true, v_true = synth.true_pose(t0 + el)
            xyz = z["xyzt"][:3] + rng.normal(0, 2.0, 3)                                  # where the true position lands in ECEF
            anchor = xyz - Rw @ p_true
            truth = orc.gnss_residuals(z["eph"], z["obs"], z["ion"], doy, np.r_[xyz, z["cb_true"] + float(z["fs_true"]) * el],
                                       np.r_[Rw @ v_true, z["fs_true"]])
            obs = np.array(z["obs"], dtype=float)
            u = truth["usable"] == 1
            obs[u, 1] += truth["res_pos"][u] - base["res_pos"][u]
            obs[u, 2] -= (truth["res_vel"][u] - base["res_vel"][u]) * obs[u, 5] / C_LIGHT
            c["epochs"].append(dict(eph=np.array(z["eph"][:n_sat]), obs=obs[:n_sat], ion=z["ion"], doy=doy, R_enu2ecef=R_ENU, anchor_ecef=anchor,
                                    psr_amp=1.0, dopp_amp=1.0))
    return cases


def host_clocks(t, slots, imu, enable_gnss=1):
    """ImuPropagator.cpp:139-148 on the host table: cb_s += dt * fs at every IMU sample, for the clocks and FS in the state"""
    if not enable_gnss or slots[4] < 0:
        return
    fs = t.slots[slots[4]]["p"][0]
    for s in range(4):
        if slots[s] < 0:
            continue
        cb = t.slots[slots[s]]["p"][0]
        for q in range(imu.shape[0]):
            cb = cb + imu[q, 6] * fs
        t.slots[slots[s]]["p"] = np.array([cb, 0.0, 0.0])


NO_EPOCH = dict(eph=NO_EPH, obs=NO_OBS, ion=None, doy=0.0, p_w=np.zeros(3), v_w=np.zeros(3), cb=np.zeros(4), fs=0.0, yaw_offset=0.0,
                R_enu2ecef=np.eye(3), anchor_ecef=np.zeros(3), idx_se23=-1, idx_yof=-1, idx_fs=-1, idx_cb=[-1] * 4)


def table_epochs(nominal, cases, f):
    """the epochs ingvio_gnss_front_stage takes: the host-owned part plus the receiver state of the tables, given in the layout of
    ingvio_nominal_get / HostTable.as_dict()"""
    out = []
    for nm, c in zip(nominal, cases):
        ep, sl = c["epochs"][f], c["gnss_slots"]
        if ep is None:
            out.append(NO_EPOCH)
            continue
        vp = nm["v_pose"]
        val = lambda s: float(nm["val"][s, 9]) if s >= 0 else 0.0
        idx = lambda s: int(nm["idx"][s]) if s >= 0 else -1
        out.append(dict(ep, p_w=nm["val"][vp, 9:12], v_w=nm["val"][vp, 12:15], cb=[val(s) for s in sl[:4]], fs=val(sl[4]), yaw_offset=val(sl[5]),
                        idx_se23=int(nm["idx"][vp]), idx_yof=idx(sl[5]), idx_fs=idx(sl[4]), idx_cb=[idx(s) for s in sl[:4]]))
    return out


def host_epochs(tabs, cases, f):
    return table_epochs([t.as_dict() for t in tabs], cases, f)


def host_step_gnss(ctx, cases, tabs, f, chi2_table, enable_gnss=1):
    """the reference loop with today's entry points: host clock recursion, closed_loop.host_step (ingvio_frame_stage_tracks, host
    boxPlus / drop / shift), then ingvio_gnss_front_stage with host values, ingvio_gnss_run, ingvio_gnss_fetch, host boxPlus"""
    for c, t in zip(cases, tabs):
        host_clocks(t, c["gnss_slots"], c["frames"][f]["imu"], enable_gnss)
    frame = host_step(ctx, cases, tabs, f)
    ctx.gnss_front_stage(0, host_epochs(tabs, cases, f), chi2_table, gate_rows=True, strong_reject=True)
    ctx.gnss_run()
    g = ctx.gnss_fetch()
    for b, t in enumerate(tabs):
        if cases[b]["epochs"][f] is not None:
            t.box_plus(g[0][b])
    return frame, g


def gnss_stage_call(ctx, cases, f, chi2_table):
    return ctx.gnss_front_stage_nominal_prepare(0, [c["epochs"][f] for c in cases], chi2_table, gate_rows=True, strong_reject=True)


class GnssForm(Form):
    """the epoch of frame i from the table, behind that frame's run: gnss_front_stage_nominal(i); gnss_run(i).  Its boxPlus must
    reach the table before frame i + 1 is staged (late); the GNSS results are fetched last, which is optional for the loop.
    epochs=False: no epochs, the late order alone (the loop with registered clocks)"""
    late = True

    def __init__(self, chi2_table, epochs=True):
        self.chi2_table, self.epochs = chi2_table, epochs

    def prepare(self, ctx, cases, f):
        return gnss_stage_call(ctx, cases, f, self.chi2_table) if self.epochs else None

    def after(self, loop, i):
        if self.epochs:
            loop.form_call(i)()
            loop.sync()
            loop.ctx.gnss_run()
            loop.sync()

    def collect(self, ctx):
        return ctx.gnss_fetch() if self.epochs else None


def gnss_frame_stage_call(ctx, cases, f, chi2_table):
    return ctx.gnss_frame_stage_nominal_prepare(0, [c["epochs"][f] for c in cases], chi2_table, gate_rows=True, strong_reject=True)


class GnssInFrameForm(Form):
    """the epoch of frame i staged right behind that frame's stage (ingvio_gnss_frame_stage_nominal); the frame's run forms its rows at
    the state after the MSCKF update and applies them.  Not late: frame i + 1 is staged while frame i runs.  The GNSS results of frame
    i are fetched between fetch_begin(i) and run(i + 1) (optional for the loop; it synchronises)."""

    def __init__(self, chi2_table):
        self.chi2_table = chi2_table

    def prepare(self, ctx, cases, f):
        return gnss_frame_stage_call(ctx, cases, f, self.chi2_table)

    def staged(self, loop, i):
        loop.form_call(i)()
        loop.sync()

    def collect(self, ctx):
        return ctx.gnss_fetch()


class GnssRoundTrip(Form):
    """the epoch through the host: ingvio_nominal_get, ingvio_gnss_front_stage with the table's values, ingvio_gnss_run,
    ingvio_gnss_fetch, ingvio_nominal_box_plus (three synchronisations per epoch)"""
    late = True

    def __init__(self, chi2_table):
        self.chi2_table = chi2_table

    def after(self, loop, i):
        ctx = loop.ctx
        nom = ctx.nominal_get()                                          # synchronises both streams
        ctx.gnss_front_stage_prepare(0, table_epochs(nom, loop.cases, loop.frames[i]), self.chi2_table, gate_rows=True, strong_reject=True)()
        ctx.gnss_run()
        g = ctx.gnss_fetch()                                             # synchronises
        ctx.nominal_box_plus(0, g[0])


def device_loop_gnss(ctx, cases, frames, chi2_table, pipelined, sync_every_call=False, in_frame=False):
    """the device loop with GNSS epochs (in_frame: staged with the frame and applied by its run); -> [(frame results, GNSS results)] per frame"""
    return device_loop(ctx, cases, frames, pipelined, (GnssInFrameForm if in_frame else GnssForm)(chi2_table), sync_every_call)
