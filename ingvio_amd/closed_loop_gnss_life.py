"""The life cycle of the GNSS scalars in the closed loop of the device-resident nominal state (ingvio_set_gnss_adjust_yof,
ingvio_nominal_add_gnss, ingvio_nominal_marg_gnss) - harness code beside closed_loop_gnss.py and closed_loop_gnss_init.py,
shared by tests/test_gnss_life_model.py, tests/test_gnss_life_schedule.py and tests/test_gpu_gnss_life.py: loops whose start state holds NO
GNSS scalar, the yaw-offset column of the update rows and of the acquisition rows in numpy, StateManager::addGNSSVariable /
margGNSSVariable on a HostTable, the host loop (on the oracle alone: oracle_life; on a context's host-fed entry points: host_life) and the
loop's Form for closed_loop.DeviceLoop.

The loop (SCRIPT): YOF enters (checkYofStatus), FS and the clocks are acquired behind frame 0, the epochs update behind the frame and
inside it, one constellation vanishes and its clock is dropped, it reappears and is acquired again.

Positions are those of ingvio_nominal_set_gnss: 0..3 the clock biases GPS, GLO, GAL, BDS, 4 FS, 5 YOF."""
import math

import numpy as np

from ingvio_amd.closed_loop import SCALAR, SIZE, DeviceLoop, Form, host_step
from ingvio_amd.closed_loop_gnss import C_LIGHT, gnss_frame_stage_call, gnss_stage_call, host_clocks, make_gnss_loop, rot_z
from ingvio_amd.closed_loop_gnss_init import (CAND, CHI2_MULT, Book, book_frame, ctx_acquire, follow, gated, init_blocks, oracle_acquire,
                                              oracle_records, spp_of, verdicts_of)

YOF = 5
INIT_COV_YOF = 0.015                                                     # IngvioParams::_init_cov_yof, the variance addGNSSVariable takes (GnssUpdate.cpp:40-42)
N_SAT = 8                                                                # the fixture's first eight satellites: four GPS, two Galileo, two BeiDou
DROP = 2                                                                 # the constellation that vanishes and comes back: Galileo


# ---- the two column formulas -----------------------------------------------------------------------------------------------------
def dot_rz(yaw):
    """GnssManager::dotRw2enu (GnssManager.cpp:101-113): d Rz(yaw) / d yaw"""
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[-s, -c, 0.0], [c, -s, 0.0], [0.0, 0.0, 0.0]])


def update_yof_column(los, R_enu2ecef, yaw, x):
    """column 9 of the update rows (GnssUpdate.cpp:164-167 with x = p_w, :239-242 with x = v_w): -u^T R_enu2ecef dRz(yaw) x per row of los"""
    return -(np.asarray(los) @ (np.asarray(R_enu2ecef) @ dot_rz(yaw) @ np.asarray(x)))


def acquire_yof_column(los, R_enu2ecef, yaw, x):
    """column 9 of the acquisition rows AS WRITTEN (GnssUpdate.cpp:401-404 with x = v_w, :462-465 with x = p_w): getRecef2enu(), the
    transpose of what the update rows take"""
    return -(np.asarray(los) @ (np.asarray(R_enu2ecef).T @ dot_rz(yaw) @ np.asarray(x)))


def skew(x):
    return np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])


def update_rows(ep, rec, adjust_yof=True):
    """the candidate rows of updateTrackedSys (GnssUpdate.cpp:148-272) in numpy, in the layout k_gnss_front stages them: the
    pseudo-range rows of the satellites whose clock is in the state, in satellite order, then their Doppler rows; columns [SE23 (9), YOF,
    the clocks in order of first appearance, FS].  ep: an epoch of ingvio_gnss_front_stage (receiver state and idx_* included), rec: its
    satellite records.  -> (vidx, vsize, H, res, Rdiag, satellites) or None without a row"""
    eph, obs = np.asarray(ep["eph"]), np.asarray(ep["obs"])
    icb = list(ep["idx_cb"])
    sats = [i for i in range(len(eph)) if rec[i, 9] != 0 and 0 <= int(eph[i, 0]) <= 3 and icb[int(eph[i, 0])] >= 0]
    nr = len(sats)
    if not nr:
        return None
    order = []
    for i in sats:
        if int(eph[i, 0]) not in order:
            order.append(int(eph[i, 0]))
    nc = 10 + len(order) + 1
    R, yaw = np.asarray(ep["R_enu2ecef"]), float(ep["yaw_offset"])
    Rw = R @ rot_z(yaw)
    p, v = np.asarray(ep["p_w"], dtype=float), np.asarray(ep["v_w"], dtype=float)
    H, res, Rd = np.zeros((2 * nr, nc)), np.zeros(2 * nr), np.zeros(2 * nr)
    for r, i in enumerate(sats):
        u = rec[i, 2:5]
        uR = u @ Rw
        H[r, 0:3], H[r, 3:6] = uR @ skew(p), -uR
        H[nr + r, 0:3], H[nr + r, 6:9] = uR @ skew(v), -uR
        H[r, 10 + order.index(int(eph[i, 0]))] = 1.0
        H[nr + r, nc - 1] = 1.0
        res[r], res[nr + r] = -rec[i, 0], -rec[i, 1]
        se = math.sin(rec[i, 6])
        se = 1e-6 if abs(se) < 1e-6 else se
        Rd[r] = (ep.get("psr_amp", 1.0) * math.sqrt(eph[i, 24] * obs[i, 3] / (se * se))) ** 2
        Rd[nr + r] = (ep.get("dopp_amp", 1.0) * math.sqrt(eph[i, 24] * (obs[i, 4] * C_LIGHT / obs[i, 5]) / (se * se))) ** 2
    if adjust_yof:
        los = rec[sats, 2:5]
        H[:nr, 9], H[nr:, 9] = update_yof_column(los, R, yaw, p), update_yof_column(los, R, yaw, v)
    vidx = [int(ep["idx_se23"]), int(ep["idx_yof"])] + [icb[s] for s in order] + [int(ep["idx_fs"])]
    return vidx, [9, 1] + [1] * (len(order) + 1), H, res, Rd, sats


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class LifeBook(Book):
    """closed_loop_gnss_init.Book plus YOF's entry and a scalar's exit"""

    def add_yof(self, idx):
        assert idx == self.n
        self.n += 1

    def drop(self, gone):
        """the columns `gone` leave the state"""
        sh = lambda x: x - sum(1 for q in gone if q < x)
        self.cidx = [sh(x) for x in self.cidx]
        self.g = [-1 if x in gone else (sh(x) if x >= 0 else -1) for x in self.g]
        self.n -= len(gone)


def strip_scalars(c):
    """the case's start state without ANY GNSS scalar (closed_loop_gnss_init.remove_scalars for all six): c["yof"] keeps YOF's value"""
    t, sl = c["table"], list(c["gnss_slots"])
    c["yof"] = float(t.slots[sl[YOF]]["p"][0])
    cut = sorted(t.slots[s]["idx"] for s in sl if s >= 0)
    keep = [i for i in range(c["P"].shape[0]) if i not in cut]
    c["P"] = np.ascontiguousarray(c["P"][np.ix_(keep, keep)])
    for s in sl:
        if s >= 0:
            t.slots[s] = None
    for s in t.slots:
        if s is not None:
            s["idx"] -= sum(1 for x in cut if x < s["idx"])
    c["gnss_slots"] = [-1] * 6


SCRIPT = {0: dict(mode=None, acquire=True), 1: dict(mode="behind"), 2: dict(mode="inframe", drop=1 << DROP), 3: dict(mode="behind", absent=DROP),
          4: dict(mode="inframe", absent=DROP), 5: dict(mode="behind", acquire=True), 6: dict(mode="inframe"), 7: dict(mode="behind")}


def make_life_loop(z, B, n_frames=8, script=SCRIPT, **kw):
    """make_gnss_loop (every filter has epochs of N_SAT satellites) whose start state holds no GNSS scalar; per case "yof", "spp", "book";
    the epochs of the frames the script marks `absent` lack that constellation's satellites"""
    cases = make_gnss_loop(z, B, n_frames, every=0, n_sat=N_SAT, **kw)
    for c in cases:
        strip_scalars(c)
        c["spp"] = spp_of(z)
        c["book"] = LifeBook(c)
        for f, ep in enumerate(c["epochs"]):
            gone = script.get(f, {}).get("absent")
            if gone is not None:
                keep = ep["eph"][:, 0].astype(int) != gone
                c["epochs"][f] = dict(ep, eph=ep["eph"][keep], obs=ep["obs"][keep])
    return cases


# ---- addGNSSVariable / margGNSSVariable on a HostTable -----------------------------------------------------------------------------
def table_add_gnss(tab, slots, pos, idx, value):
    """StateManager.cpp:216-231 on the table: the lowest free slot becomes a Scalar at idx, registered at position pos; -> the slot"""
    assert slots[pos] < 0
    slot = next((i for i, s in enumerate(tab.slots) if s is None), len(tab.slots))
    new = dict(kind=SCALAR, idx=int(idx), anchor=-1, R=np.eye(3), p=np.array([float(value), 0.0, 0.0]), v=np.zeros(3))
    if slot == len(tab.slots):
        tab.slots.append(new)
    else:
        tab.slots[slot] = new
    slots[pos] = slot
    return slot


def table_marg_gnss(tab, slots, mask):
    """StateManager.cpp:233-242 on the table for every position named in mask; -> the columns that leave, ascending"""
    gone = sorted(tab.slots[slots[s]]["idx"] for s in range(6) if (mask >> s) & 1)
    for s in range(6):
        if (mask >> s) & 1:
            tab.slots[slots[s]] = None
            slots[s] = -1
    for v in tab.slots:
        if v is not None:
            v["idx"] -= sum(1 for q in gone if q < v["idx"])
    return gone


def check_state_continuity(tab, n):
    """StateManager::checkStateContinuity (StateManager.cpp:27-40): the variables' [idx, idx + size) tile [0, n)"""
    spans = sorted((s["idx"], SIZE[s["kind"]]) for s in tab.slots if s is not None)
    at = 0
    for i, sz in spans:
        if i != at:
            return False
        at += sz
    return at == n


def table_epoch(tab, slots, ep):
    """the epoch ingvio_gnss_front_stage takes at the table's receiver (closed_loop_gnss.table_epochs for one HostTable)"""
    e = tab.slots[tab.v_pose]
    val = lambda s: float(tab.slots[s]["p"][0]) if s >= 0 else 0.0
    idx = lambda s: int(tab.slots[s]["idx"]) if s >= 0 else -1
    return dict(ep, p_w=e["p"], v_w=e["v"], cb=[val(s) for s in slots[:4]], fs=val(slots[4]), yaw_offset=val(slots[YOF]),
                idx_se23=int(e["idx"]), idx_yof=idx(slots[YOF]), idx_fs=idx(slots[4]), idx_cb=[idx(s) for s in slots[:4]])


def updatable(slots):
    """checkGnssStates: YOF, FS and a clock in the state"""
    return slots[4] >= 0 and slots[YOF] >= 0 and any(s >= 0 for s in slots[:4])


# ---- the host loop on the oracle alone ---------------------------------------------------------------------------------------------
def oracle_life(c, chi2_table, adjust_yof=True, check=None):
    """One filter's GNSS scalars through their life on orc.Cov, without camera frames: YOF enters, FS and the clocks are acquired from
    epoch 0, an epoch updates (no row gate: the oracle has none for these rows), the DROP clock leaves, and is acquired again.
    check(step, tab, slots, cov) after every step.  -> (tab, slots, P, log); log: per step what it did"""
    import copy
    from oracle import oracle as orc
    tab, slots = copy.deepcopy(c["table"]), list(c["gnss_slots"])
    cov = orc.Cov(c["P"], ld=c["P"].shape[0] + 32)
    log = []

    def done(step, **what):
        log.append(dict(step=step, n=cov.n, **what))
        if check:
            check(step, tab, slots, cov)

    idx = cov.append_independent(np.array([[INIT_COV_YOF]]))
    table_add_gnss(tab, slots, YOF, idx, c["yof"])
    done("add_yof", idx=idx)

    def acquire(step, ep):
        ver, P = oracle_acquire(cov.P, tab, slots, ep, c["spp"], chi2_table, ld=cov.ld, adjust_yof=adjust_yof)
        cov.buf[:] = 0.0
        cov.n = P.shape[0]
        cov.buf[:cov.n, :cov.n] = P
        done(step, added=[g for g in range(CAND) if ver[g]["added"]], verdicts=ver)

    def update(step, ep):
        e = table_epoch(tab, slots, ep)
        rows = update_rows(e, oracle_records(e), adjust_yof)
        dx, rc = cov.ekf_update(rows[0], rows[1], rows[2], rows[3], rows[4])
        tab.box_plus(dx)
        done(step, rows=rows[2].shape[0], col9=float(np.abs(rows[2][:, 9]).max()), rc=rc)

    acquire("acquire", c["epochs"][0])
    update("update", c["epochs"][1])
    gone = table_marg_gnss(tab, slots, 1 << DROP)
    for q in reversed(gone):
        cov.marginalize(q, 1)
    done("drop", gone=gone)
    update("update_without", c["epochs"][3])
    acquire("reacquire", c["epochs"][5])
    update("update_again", c["epochs"][6])
    return tab, slots, cov.P, log


# ---- the host loop on a context's host-fed entry points ----------------------------------------------------------------------------
def host_add_yof(ctx, cases, tabs):
    for b, (c, t) in enumerate(zip(cases, tabs)):
        idx = int(ctx.append_independent(b, np.array([[INIT_COV_YOF]]))[0])
        table_add_gnss(t, c["gnss_slots"], YOF, idx, c["yof"])
        c["book"].add_yof(idx)


def host_epoch(ctx, cases, tabs, f, chi2_table, adjust_yof=True):
    """updateTrackedSys with the numpy rows: ingvio_gnss_sat_eval at the host tables' receivers, update_rows, ingvio_gnss_stage (the row
    gates run on the device as they do for the front's rows), ingvio_gnss_run, ingvio_gnss_fetch, host boxPlus"""
    live = [b for b, c in enumerate(cases) if c["epochs"][f] is not None and len(c["epochs"][f]["eph"]) and updatable(c["gnss_slots"])]
    blocks = [None] * len(cases)
    if live:
        eps = [table_epoch(tabs[b], cases[b]["gnss_slots"], cases[b]["epochs"][f]) for b in live]
        recs = ctx.gnss_sat_eval(eps)
        for b, e, rec in zip(live, eps, recs):
            rows = update_rows(e, rec, adjust_yof)
            blocks[b] = None if rows is None else rows[:5]
    if all(blk is None for blk in blocks):
        return None
    ctx.gnss_stage(0, blocks, chi2_table, gate_rows=True, strong_reject=True)
    ctx.gnss_run()
    g = ctx.gnss_fetch()
    for b, t in enumerate(tabs):
        if blocks[b] is not None:
            t.box_plus(g[0][b])
    return g


def host_drop(ctx, cases, tabs, mask):
    for b, (c, t) in enumerate(zip(cases, tabs)):
        gone = table_marg_gnss(t, c["gnss_slots"], mask)
        for q in reversed(gone):
            ctx.marginalize(b, [q], 1)
        c["book"].drop(gone)


def host_life(ctx, cases, tabs, frames, chi2_table, script=SCRIPT, adjust_yof=True, probe=None):
    """the reference loop: the host table, today's host-fed entry points for the covariance.  The cases' books and slots move.
    probe(f): behind everything frame f does.  -> [(frame results, GNSS results or ())], {frame: the acquisition's verdicts}"""
    host_add_yof(ctx, cases, tabs)
    out, ver = [], {}
    for f in frames:
        s = script.get(f, {})
        book_frame(cases, f)
        for c, t in zip(cases, tabs):
            host_clocks(t, c["gnss_slots"], c["frames"][f]["imu"])
        frame = host_step(ctx, cases, tabs, f)
        g = host_epoch(ctx, cases, tabs, f, chi2_table, adjust_yof) if s.get("mode") else None
        if s.get("acquire"):
            ver[f] = ctx_acquire(ctx, cases, tabs, f, chi2_table, adjust_yof=adjust_yof)
            follow(cases, ver[f])
        if s.get("drop"):
            host_drop(ctx, cases, tabs, s["drop"])
        out.append((frame, () if g is None else g))
        if probe:
            probe(f)
    return out, ver


# ---- the device loop ---------------------------------------------------------------------------------------------------------------
class LifeForm(Form):
    """The script on the device.  Per frame: its epoch from the table, behind the frame (ingvio_gnss_front_stage_nominal + ingvio_gnss_run)
    or staged with it (ingvio_gnss_frame_stage_nominal); then ingvio_gnss_init_nominal where the script acquires and
    ingvio_nominal_marg_gnss where it drops.  Late: an acquisition or a drop must reach the table before the next frame is staged.
    The epoch's results are fetched inside after() - the run of the next frame may carry an epoch of its own.  The frames' integers come
    from the cases' books."""
    late = True

    def __init__(self, chi2_table, script=SCRIPT, fetch=True, probe=None):
        self.chi2_table, self.script, self.fetch, self.probe = chi2_table, script, fetch, probe
        self.verdicts, self.raw, self.how, self.last = {}, {}, {}, None

    def staged(self, loop, i):
        f = loop.frames[i]
        if self.script.get(f, {}).get("mode") == "inframe":
            gnss_frame_stage_call(loop.ctx, gated(loop.cases, f), f, self.chi2_table)()
            loop.sync()

    def after(self, loop, i):
        ctx, cases, f = loop.ctx, loop.cases, loop.frames[i]
        s = self.script.get(f, {})
        if s.get("mode") == "behind":
            gnss_stage_call(ctx, gated(cases, f), f, self.chi2_table)()
            loop.sync()
            ctx.gnss_run()
            loop.sync()
        self.last = ctx.gnss_fetch() if s.get("mode") and self.fetch else None
        if s.get("mode") == "inframe" and self.fetch:
            self.how[f] = ctx.debug_gnss_fused_last()
        if s.get("acquire"):
            self.raw[f] = ctx.gnss_init_nominal(0, init_blocks(cases, f), self.chi2_table, CHI2_MULT, True, True)
            self.verdicts[f] = verdicts_of(self.raw[f])
            follow(cases, self.verdicts[f])
        if s.get("drop"):
            ctx.nominal_marg_gnss(0, [s["drop"]] * len(cases))
            loop.sync()
            assert not s["drop"] >> YOF                                   # (the book keeps the clocks and FS)
            for c in cases:
                c["book"].drop(sorted(c["book"].g[q] for q in range(YOF) if (s["drop"] >> q) & 1))
                c["gnss_slots"] = [-1 if (s["drop"] >> q) & 1 else v for q, v in enumerate(c["gnss_slots"])]
        if self.probe:
            self.probe(f)
        if i + 1 < len(loop.frames):
            book_frame(cases, loop.frames[i + 1])

    def collect(self, ctx):
        return () if self.last is None else self.last                    # (None would make DeviceLoop hand back the frame results alone)


def device_add_yof(ctx, cases):
    """checkYofStatus' addGNSSVariable for the batch: one call, no synchronisation; books and slots follow the mirror's answer"""
    slot, idx = ctx.nominal_add_gnss(0, [YOF] * len(cases), [c["yof"] for c in cases], [INIT_COV_YOF] * len(cases))
    for c, s, i in zip(cases, slot, idx):
        c["gnss_slots"] = list(c["gnss_slots"][:YOF]) + [int(s)]
        c["book"].add_yof(int(i))


def device_life(ctx, cases, frames, chi2_table, pipelined, script=SCRIPT, fetch=True, probe=None):
    """the device loop of the script; the context's switch (ingvio_set_gnss_adjust_yof) is the caller's.  -> [(frame results, GNSS
    results or ())], the form (verdicts, how the in-frame epochs were applied)"""
    device_add_yof(ctx, cases)
    form = LifeForm(chi2_table, script, fetch, probe)
    book_frame(cases, frames[0])
    return DeviceLoop(ctx, cases, frames, form, pipelined, sync_every_call=not pipelined).run(), form


def life_ctx(cases, F, c_max=12, adjust_yof=None):
    """a context with room for the six scalars and the new clone, the cases' covariances and tables set; adjust_yof None: the switch
    is never touched"""
    from ingvio_amd import capi
    n_max = max(c["P"].shape[0] for c in cases) + 6 + 6
    ctx = capi.Context(batch=len(cases), n_max=((n_max + 15) // 16) * 16, c_max=c_max, f_max=F, m_max=64)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c["P"])
    ctx.tracks_create(F)
    ctx.nominal_create(48)
    ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    if adjust_yof is not None:
        ctx.set_gnss_adjust_yof(adjust_yof)
    return ctx
