"""GNSS clock states acquired in the closed loop of the device-resident nominal state (ingvio_gnss_init_nominal) - harness
code beside closed_loop_gnss.py, shared by tests/test_gnss_init_model.py, tests/test_gpu_gnss_init.py and tools/closed_loop_bench.py
--gnss-acquire: loops of make_gnss_loop whose start state LACKS a chosen subset of {FS, clock GPS, GLO, GAL, BDS}, the SPP fix that
reports them, GnssUpdate::addNewTrackedSys (GnssUpdate.cpp:295-470, oracle/stream_filter.py::add_new_tracked_sys) on a HostTable with
the delayed initialisation of a backend of choice (the oracle's covariance: oracle_acquire; today's single-filter entry points of a
context: host_acquire, the round trip the new export replaces), the integer bookkeeping a host keeps while the state grows (Book), and
the loop's Form for closed_loop.DeviceLoop.

Candidate g: 0 = FS, 1..4 = clock bias GPS, GLO, GAL, BDS (INGVIO_GNSS_INIT_CAND); its entry of a case's "gnss_slots" is gpos(g)."""
import copy
import math

import numpy as np

from ingvio_amd.closed_loop import SCALAR, HostTable
from ingvio_amd.closed_loop_gnss import C_LIGHT, GnssForm, host_step_gnss, make_gnss_loop, rot_z

CAND = 5
NAMES = ("FS", "GPS", "GLO", "GAL", "BDS")
CHI2_MULT = 0.95                                                         # GnssUpdate.cpp:406 / :467


def gpos(g):
    return 4 if g == 0 else g - 1


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def remove_scalars(c, removed):
    """the case's start state without the scalars of the candidates in `removed`: their rows and columns cut from P, every idx of
    the table renumbered, their slots freed, their entries of gnss_slots -1.  c["removed"] keeps the list."""
    t, sl = c["table"], c["gnss_slots"]
    cut = sorted(t.slots[sl[gpos(g)]]["idx"] for g in removed)
    n = c["P"].shape[0]
    keep = [i for i in range(n) if i not in cut]
    c["P"] = np.ascontiguousarray(c["P"][np.ix_(keep, keep)])
    for g in removed:
        t.slots[sl[gpos(g)]] = None
        sl[gpos(g)] = -1
    for s in t.slots:
        if s is not None:
            s["idx"] -= sum(1 for x in cut if x < s["idx"])
    c["removed"] = sorted(removed)


def spp_of(z):
    """the SPP fix of the fixture: SppMeas::posSpp [7] / velSpp [4]"""
    return dict(pos_spp=np.array(z["xyzt"], dtype=float), vel_spp=np.array(z["velt"], dtype=float))


def make_init_loop(z, B, n_frames, removed, **kw):
    """make_gnss_loop(every=0) with filter b's start state lacking removed[b % len(removed)] (a list of candidates); per case also "spp"
    (the fixture's SPP fix) and "book" (the integers of the state as the host keeps them); the frames' marg / new_idx / gnss_idx are
    written by the book when a frame is due (Book.frame), because an acquisition changes them."""
    cases = make_gnss_loop(z, B, n_frames, every=0, **kw)
    for b, c in enumerate(cases):
        c["gnss_slots"] = list(c["gnss_slots"])
        remove_scalars(c, list(removed[b % len(removed)]))
        c["spp"] = spp_of(z)
        c["book"] = Book(c)
    return cases


ALL5 = (0, 1, 2, 3, 4)
# the mixed scenario of the tests: what each of ten filters lacks and what is done to its epochs
# (the "moved" filter is the one with 8 clones and 33 IMU samples per frame: there FS's update moves p_w most; the filter that lacks
# nothing is the one with the widest window, so that closed_loop.loop_ctx, which sizes n_max by the largest start state, leaves the
# others room to grow)
MIXED = [dict(removed=(0, 1, 4)), dict(removed=(2, 3)), dict(removed=ALL5), dict(removed=ALL5, moved=True), dict(removed=ALL5, no_epoch=True),
         dict(removed=(2, 3), one_glo=True), dict(removed=()), dict(removed=(0, 1, 4), bds_outlier=80.0),
         dict(removed=(1, 2, 3, 4)), dict(removed=ALL5, bds_outlier=80.0)]


def make_mixed(z, n_frames=1, **kw):
    """ten filters, ragged windows of 5-11 clones: MIXED.  no_epoch: the filter has no satellites (n_sat = 0); one_glo: its epochs keep
    one GLONASS satellite (m = 1: skipped); bds_outlier: metres added to the first BeiDou pseudo-range (refused); moved: the filter
    whose five candidates are checked round by round."""
    cases = make_init_loop(z, len(MIXED), n_frames, [m["removed"] for m in MIXED], **kw)
    for c, m in zip(cases, MIXED):
        c["mixed"] = m
        for f, ep in enumerate(c["epochs"]):
            if m.get("no_epoch"):
                c["epochs"][f] = None
                continue
            sys = ep["eph"][:, 0].astype(int)
            if m.get("one_glo"):
                keep = np.ones(len(sys), dtype=bool)
                keep[np.flatnonzero(sys == 1)[1:]] = False
                c["epochs"][f] = ep = dict(ep, eph=ep["eph"][keep], obs=ep["obs"][keep])
            if m.get("bds_outlier"):
                obs = np.array(ep["obs"])
                obs[np.flatnonzero(ep["eph"][:, 0].astype(int) == 3)[0], 1] += m["bds_outlier"]
                c["epochs"][f] = dict(ep, obs=obs)
    return cases


class Book:
    """The integers of a filter's state that the frame stage takes (marg, new_idx, gnss_idx), kept by the host while frames marginalise
    and acquisitions append: make_loop prepares them ahead, which an acquisition in the middle of the loop forbids."""

    def __init__(self, c):
        t = c["table"]
        self.cidx = [t.slots[v]["idx"] for v in t.clones]
        self.n = c["P"].shape[0]
        self.g = [t.slots[s]["idx"] if s >= 0 else -1 for s in c["gnss_slots"][:5]]

    def frame(self, fr):
        """frame fr is due: its integers, then the state behind its marginalisation"""
        self.cidx = self.cidx + [self.n]
        marg = self.cidx[1]
        fr["marg"], fr["new_idx"], fr["gnss_idx"] = marg, self.n, list(self.g)
        self.cidx = [x - 6 if x > marg else x for x in self.cidx if x != marg]
        self.g = [x - 6 if x > marg else x for x in self.g]

    def add(self, g, idx):
        assert idx == self.n
        self.g[gpos(g)] = idx
        self.n += 1


def book_frame(cases, f):
    for c in cases:
        c["book"].frame(c["frames"][f])


def follow(cases, verdicts):
    """books and gnss_slots of the cases follow an acquisition's verdicts: per filter {g: dict(added, new_idx, slot)}"""
    for c, v in zip(cases, verdicts):
        for g in range(CAND):
            if v[g]["added"]:
                c["book"].add(g, v[g]["new_idx"])
                c["gnss_slots"][gpos(g)] = v[g]["slot"]


def gated(cases, f):
    """views of the cases whose only epoch is frame f's, None where updateTrackedSys has nothing to do (checkGnssStates: YOF, FS and a
    clock in the state) - the stages of an epoch refuse a receiver without FS"""
    out = []
    for c in cases:
        sl = c["gnss_slots"]
        ok = sl[4] >= 0 and sl[5] >= 0 and any(s >= 0 for s in sl[:4])
        out.append(dict(c, epochs={f: c["epochs"][f] if ok else None}))
    return out


# ---- addNewTrackedSys on a HostTable ---------------------------------------------------------------------------------------------
def candidates(slots, spp):
    """the host's decision (getSysInSppMeas, calcSysToAdd): FS, then GPS, GLO, GAL, BDS"""
    out = [0] if abs(spp["vel_spp"][3]) > 1e-3 and slots[4] < 0 else []
    return out + [1 + s for s in range(4) if abs(spp["pos_spp"][3 + s]) > 1e-3 and slots[s] < 0]


def receiver(tab, slots, ep, spp):
    """the epoch ingvio_gnss_sat_eval takes, at the receiver of GnssUpdate.cpp:343-372: the table's state, the clocks and FS to add
    taken from the SPP fix, a scalar neither in the state nor to be added zero"""
    e, cands = tab.slots[tab.v_pose], candidates(slots, spp)
    val = lambda pos, g, fix: float(tab.slots[slots[pos]]["p"][0]) if slots[pos] >= 0 else (float(fix) if g in cands else 0.0)
    return dict(ep, p_w=e["p"], v_w=e["v"], cb=[val(s, 1 + s, spp["pos_spp"][3 + s]) for s in range(4)], fs=val(4, 0, spp["vel_spp"][3]),
                yaw_offset=float(tab.slots[slots[5]]["p"][0]))


def oracle_records(ep):
    """the satellite records [ns, 20] (INGVIO_GNSS_SAT_REC; the SatState left out) of a receiver() epoch, from the oracle"""
    from oracle import oracle as orc
    Rw = np.asarray(ep["R_enu2ecef"]) @ rot_z(ep["yaw_offset"])
    xyzt = np.r_[Rw @ ep["p_w"] + ep["anchor_ecef"], ep["cb"]]
    velt = np.r_[Rw @ ep["v_w"], ep["fs"]]
    o = orc.gnss_residuals(ep["eph"], ep["obs"], ep["ion"], ep["doy"], xyzt, velt)
    rec = np.zeros((len(ep["eph"]), 20))
    rec[:, 0], rec[:, 1], rec[:, 2:5], rec[:, 5:7], rec[:, 7:9], rec[:, 9] = o["res_pos"], o["res_vel"], o["los"], o["azel"], o["atmos"], o["usable"]
    return rec


def rows_of(g, ep, rec, Rw, x, yaw=None):
    """getResJacobianOfSys (:472-521) for candidate g from the satellite records: (Hx [m, 10], res [m], noise, satellites used).
    yaw: is_adjust_yof - the YOF value the round reads; column 9 is then the reference's as written (:401-404, :462-465), with
    getRecef2enu() = R_enu2ecef^T.  None (the default): column 9 stays zero"""
    fs = g == 0
    eph, obs = np.asarray(ep["eph"]), np.asarray(ep["obs"])
    sats = [i for i in range(len(eph)) if rec[i, 9] != 0 and (fs or int(eph[i, 0]) == g - 1)]
    m = len(sats)
    Hx, res, avg = np.zeros((m, 10)), np.zeros(m), 0.0
    RS = Rw @ np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])
    for r, i in enumerate(sats):
        u = rec[i, 2:5]
        Hx[r, 0:3] = u @ RS
        Hx[r, (6 if fs else 3):(9 if fs else 6)] = -(u @ Rw)
        if yaw is not None:
            cy, sy = math.cos(yaw), math.sin(yaw)
            Hx[r, 9] = -(u @ (np.asarray(ep["R_enu2ecef"]).T @ np.array([-sy * x[0] - cy * x[1], cy * x[0] - sy * x[1], 0.0])))
        res[r] = -(rec[i, 1] if fs else rec[i, 0])
        se = math.sin(rec[i, 6])
        se = 1e-6 if abs(se) < 1e-6 else se
        std = obs[i, 4] * C_LIGHT / obs[i, 5] if fs else obs[i, 3]
        avg += eph[i, 24] * std / (se * se)
    noise = (ep.get("dopp_amp", 1.0) if fs else ep.get("psr_amp", 1.0)) * math.sqrt(avg / m) if m else 0.0
    return Hx, res, noise, sats


def acquire(tab, slots, ep, spp, rec, add, chi2_table, read_once=False, adjust_yof=False):
    """addNewTrackedSys on a HostTable (moved in place, with `slots`).  rec: the satellite records at receiver(tab, slots, ep, spp);
    add(vidx, vsize, Hx, Hf, res, noise, chi2_check) -> (added, dx, chi2, new_idx): the backend's addVariableDelayed.
    read_once: p, v are read once before the loop instead of per round (what the reference does NOT do, :397 / :458).
    adjust_yof: is_adjust_yof - the rows carry the YOF column, from YOF as the table holds it in the round.
    -> {g: dict(added, new_idx, slot, chi2, noise, dx, m)} for the five candidates"""
    out = {g: dict(added=False, new_idx=-1, slot=-1, chi2=0.0, noise=0.0, dx=None, m=0) for g in range(CAND)}
    if ep is None or len(ep["eph"]) == 0 or slots[5] < 0:
        return out
    cands = candidates(slots, spp)
    e, yof = tab.slots[tab.v_pose], tab.slots[slots[5]]
    Rw = np.asarray(ep["R_enu2ecef"]) @ rot_z(yof["p"][0])                # once, from YOF at the start (:332)
    free = [i for i, s in enumerate(tab.slots) if s is None]
    free += list(range(len(tab.slots), len(tab.slots) + CAND))
    slot_of = {g: free[k] for k, g in enumerate(cands)}
    p0, v0 = np.array(e["p"]), np.array(e["v"])
    for g in cands:
        x = (v0 if g == 0 else p0) if read_once else (e["v"] if g == 0 else e["p"])
        Hx, res, noise, sats = rows_of(g, ep, rec, Rw, x, float(yof["p"][0]) if adjust_yof else None)
        m = out[g]["m"] = len(sats)
        if m <= 1:                                                       # StateManager.cpp:571-575
            continue
        added, dx, chi2, idx = add([e["idx"], yof["idx"]], [9, 1], Hx, np.ones((m, 1)), res, noise, float(chi2_table[m]))
        out[g].update(chi2=chi2, noise=noise, hnorm=math.sqrt(float(np.sum(Hx * Hx)) + m))      # |[Hx | H_new]|_F: the rotations keep it
        if not added:
            continue
        value = spp["vel_spp"][3] if g == 0 else spp["pos_spp"][2 + g]
        while len(tab.slots) <= slot_of[g]:
            tab.slots.append(None)
        tab.slots[slot_of[g]] = dict(kind=SCALAR, idx=idx, anchor=-1, R=np.eye(3), p=np.array([float(value), 0.0, 0.0]), v=np.zeros(3))
        tab.box_plus(dx)
        slots[gpos(g)] = slot_of[g]
        out[g].update(added=True, new_idx=idx, slot=slot_of[g], dx=np.array(dx))
    return out


def oracle_acquire(P, tab, slots, ep, spp, chi2_table, read_once=False, ld=None, rec=None, adjust_yof=False):
    """acquire() on orc.Cov.add_variable_delayed, no GPU; -> (verdicts, the posterior P); tab and slots are moved in place.
    rec: satellite records to take instead of the oracle's own (the device front's: the two agree to 1e-6 m in res_pos only)"""
    from oracle import oracle as orc
    cov = orc.Cov(P, ld=ld or P.shape[0] + 16)
    if ep is None or slots[5] < 0:
        return acquire(tab, slots, ep, spp, None, None, chi2_table), P

    def add(vidx, vsize, Hx, Hf, res, noise, chk):
        added, dx, chi2 = cov.add_variable_delayed(vidx, vsize, Hx, Hf, res, noise, chi2_mult=CHI2_MULT, do_chi2=True, chi2_check=chk)
        lam.append(float(np.linalg.eigvalsh(np.array(cov.P() if callable(cov.P) else cov.P)).max()))
        return added, dx, chi2, cov.n - 1
    lam = []                                                             # lambda_max of P behind every round that was tried, in order
    out = acquire(tab, slots, ep, spp, oracle_records(receiver(tab, slots, ep, spp)) if rec is None else rec, add, chi2_table, read_once, adjust_yof)
    for g, l in zip([g for g in range(CAND) if "hnorm" in out[g]], lam):
        out[g]["lam_post"] = l
    Pn = cov.P() if callable(cov.P) else cov.P
    return out, np.array(Pn)


def ctx_acquire(ctx, cases, tabs, f, chi2_table, read_once=False, adjust_yof=False):
    """acquire() for every filter on today's single-filter entry points of a context that holds the covariances: ingvio_gnss_sat_eval at
    the overridden receivers (one call), then ingvio_add_variable_delayed per candidate with its own noise, host boxPlus on tabs.
    The cases' gnss_slots move with the verdicts."""
    eps = [c["epochs"][f] for c in cases]
    live = [b for b, (c, ep) in enumerate(zip(cases, eps)) if ep is not None and c["gnss_slots"][5] >= 0 and candidates(c["gnss_slots"], c["spp"])]
    recs = {}
    if live:
        r = ctx.gnss_sat_eval([receiver(tabs[b], cases[b]["gnss_slots"], eps[b], cases[b]["spp"]) for b in live])
        recs = {b: r[i] for i, b in enumerate(live)}
    out = []
    for b, c in enumerate(cases):
        def add(vidx, vsize, Hx, Hf, res, noise, chk, b=b):
            return ctx.add_variable_delayed(b, vidx, vsize, Hx, Hf, res, noise, chi2_mult=CHI2_MULT, do_chi2=True, chi2_check=chk)
        out.append(acquire(tabs[b], c["gnss_slots"], eps[b] if b in recs else None, c["spp"], recs.get(b), add, chi2_table, read_once, adjust_yof))
    return out


def table_from(nm):
    """a HostTable from a filter's ingvio_nominal_get record"""
    slots = []
    for k, i, a, v in zip(nm["kind"], nm["idx"], nm["anchor"], nm["val"]):
        slots.append(None if k < 0 else dict(kind=int(k), idx=int(i), anchor=int(a), R=np.array(v[0:9]).reshape(3, 3), p=np.array(v[9:12]), v=np.array(v[12:15])))
    return HostTable(slots, [int(x) for x in nm["clone_var"]], nm["v_ext"], nm["v_pose"], nm["v_bg"], nm["v_ba"], nm["gravity"])


def host_acquire(ctx, cases, f, chi2_table, read_once=False):
    """the round trip through the host with today's entry points, on a context with the device table: ingvio_nominal_get,
    ingvio_gnss_sat_eval, numpy rows, ingvio_add_variable_delayed per candidate, host boxPlus, ingvio_nominal_set + _set_gnss"""
    tabs = [table_from(nm) for nm in ctx.nominal_get()]
    out = ctx_acquire(ctx, cases, tabs, f, chi2_table, read_once)
    ctx.nominal_set(0, [t.as_dict() for t in tabs])
    ctx.nominal_set_gnss(0, [c["gnss_slots"] for c in cases])
    return out


def init_blocks(cases, f):
    """the blocks ingvio_gnss_init_nominal takes (capi.make_gnss_init_blocks) for frame f's epochs"""
    return [dict(epoch=c["epochs"][f], pos_spp=c["spp"]["pos_spp"], vel_spp=c["spp"]["vel_spp"]) for c in cases]


def verdicts_of(res, ns=None):
    """the export's arrays as acquire() returns its verdicts"""
    out = []
    for b in range(res["added"].shape[0]):
        out.append({g: dict(added=bool(res["added"][b, g]), new_idx=int(res["new_idx"][b, g]), slot=int(res["slot"][b, g]), chi2=float(res["chi2"][b, g]),
                            noise=float(res["noise"][b, g]), dx=None if res["dx"] is None or not res["added"][b, g] else res["dx"][b, g]) for g in range(CAND)})
    return out


# ---- the loops -------------------------------------------------------------------------------------------------------------------
def host_loop(ctx, cases, tabs, frames, chi2_table, acquire_at):
    """the reference loop: closed_loop_gnss.host_step_gnss per frame (the epoch only where the receiver has FS and a clock), and behind
    frame acquire_at's epoch ctx_acquire on the host tables.  -> [(frame results, GNSS results)], the acquisition's verdicts"""
    out, ver = [], None
    for f in frames:
        book_frame(cases, f)
        out.append(host_step_gnss(ctx, gated(cases, f), tabs, f, chi2_table))
        if f == acquire_at:
            ver = ctx_acquire(ctx, cases, tabs, f, chi2_table)
            follow(cases, ver)
    return out, ver


class GnssAcquireForm(GnssForm):
    """GnssForm plus, behind the epoch of frame acquire_at, ONE ingvio_gnss_init_nominal for the batch (it synchronises; the host then
    extends the clock indices of the next frame's stage).  The frames' integers come from the cases' books, so no stage is prepared
    ahead.  self.verdicts: the acquisition's results."""

    def __init__(self, chi2_table, acquire_at, want_dx=True):
        super().__init__(chi2_table)
        self.acquire_at, self.want_dx, self.verdicts, self.raw = acquire_at, want_dx, None, None

    def prepare(self, ctx, cases, f):
        from ingvio_amd.closed_loop_gnss import gnss_stage_call
        return gnss_stage_call(ctx, gated(cases, f), f, self.chi2_table)

    def after(self, loop, i):
        super().after(loop, i)
        f = loop.frames[i]
        if f == self.acquire_at:
            self.raw = loop.ctx.gnss_init_nominal(0, init_blocks(loop.cases, f), self.chi2_table, CHI2_MULT, True, self.want_dx)
            self.verdicts = verdicts_of(self.raw)
            follow(loop.cases, self.verdicts)
        if i + 1 < len(loop.frames):
            book_frame(loop.cases, loop.frames[i + 1])


def device_loop_acquire(ctx, cases, frames, chi2_table, pipelined, acquire_at):
    """the device loop with the acquisition behind frame acquire_at; -> [(frame results, GNSS results)], the form (its verdicts)"""
    from ingvio_amd.closed_loop import DeviceLoop
    form = GnssAcquireForm(chi2_table, acquire_at)
    book_frame(cases, frames[0])
    return DeviceLoop(ctx, cases, frames, form, pipelined, sync_every_call=not pipelined).run(), form


def fresh(cases):
    """a deep copy: the loops move a case's gnss_slots, book and frames"""
    return copy.deepcopy(cases)
