"""ingvio_gnss_init_nominal (k_delayed_front<DL_GNSS>, kernels_delayed.hip): GnssUpdate::addNewTrackedSys from the device
nominal table - the frequency shift and the clock biases the SPP fix reports and the table lacks are initialised on the device, one
round per candidate, one synchronisation.  Checked against the round trip through the host made of today's entry points
(closed_loop_gnss_init.host_acquire), against the oracle (oracle_acquire), and inside the closed loop against a host loop.
The scenario (closed_loop_gnss_init.MIXED: ten filters, windows of 5-11 clones) is shown to exercise additions, refusals and skips by
tests/test_gnss_init_model.py on the oracle alone."""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from conftest import rel_err as rel
from ingvio_amd.closed_loop import DeviceLoop, loop_ctx, nominal_stage
from ingvio_amd.closed_loop_gnss import R_ENU, gnss_frame_stage_call, gnss_stage_call, rot_z
from ingvio_amd.closed_loop_gnss_init import (CAND, CHI2_MULT, GnssAcquireForm, book_frame, candidates, device_loop_acquire, follow, fresh, gated,
                                              gpos, host_acquire, host_loop, init_blocks, make_mixed, oracle_acquire, oracle_records, receiver,
                                              rows_of, table_from, verdicts_of)
from nominal_helpers import TABLE_KEYS, assert_table, refused, same_state, table_ctx
from nominal_helpers import device_state as state

pytestmark = pytest.mark.gpu

F = 24
TOL = 1e-9                               # tests/test_gpu_nominal_gnss.py


def chi2():
    from ingvio_amd import synth
    return synth.chi2_table()


@pytest.fixture(scope="module")
def mixed():
    return make_mixed(load_golden("gnss_front"))


@pytest.fixture(scope="module")
def one_call(mixed):
    """the export on the mixed scenario's start state, once: (raw results, verdicts, state before, state after, n after, GNSS slots after)"""
    ctx = table_ctx(mixed, F, gnss=True)
    B = len(mixed)
    s0 = state(ctx, B)
    raw = ctx.gnss_init_nominal(0, init_blocks(mixed, 0), chi2(), CHI2_MULT)
    out = (raw, verdicts_of(raw), s0, state(ctx, B), [ctx.n(b) for b in range(B)], ctx.nominal_get_gnss())
    ctx.close()
    return out


@pytest.fixture(scope="module")
def round_trip(mixed):
    """host_acquire on the same start state: (verdicts, state after, n after, the cases' slots after)"""
    cases = fresh(mixed)
    ctx = table_ctx(cases, F, gnss=True)
    B = len(cases)
    ver = host_acquire(ctx, cases, 0, chi2())
    out = (ver, state(ctx, B), [ctx.n(b) for b in range(B)], [list(c["gnss_slots"]) for c in cases])
    ctx.close()
    return out


@pytest.fixture(scope="module")
def device_records(mixed):
    """the satellite records of the device front at every filter's overridden receiver (None: no epoch)"""
    ctx = table_ctx(mixed, F, gnss=True)
    out = [None if c["epochs"][0] is None else ctx.gnss_sat_eval([receiver(c["table"], c["gnss_slots"], c["epochs"][0], c["spp"])])[0] for c in mixed]
    ctx.close()
    return out


# ---- 1. the rows -------------------------------------------------------------------------------------------------------------------
def test_rows_equal_numpy_rows_from_the_satellite_records_and_the_oracle(mixed, orc):
    cases = mixed
    ctx = table_ctx(cases, F, gnss=True)
    B = len(cases)
    s0 = state(ctx, B)
    blocks = init_blocks(cases, 0)
    tried = 0
    for b, c in enumerate(cases):
        ep, sl = c["epochs"][0], c["gnss_slots"]
        if ep is None:
            for g in range(CAND):
                H, res, noise = ctx.debug_gnss_init_rows(b, blocks[b], g)
                assert H.shape == (0, 10) and noise == 0.0
            continue
        t = c["table"]
        rcv = receiver(t, sl, ep, c["spp"])
        rec = ctx.gnss_sat_eval([rcv])[0]
        orec = oracle_records(rcv)
        Rw = R_ENU @ rot_z(t.slots[sl[5]]["p"][0])
        e = t.slots[t.v_pose]
        for g in range(CAND):                                            # every candidate, whether the call would try it or not
            H, res, noise = ctx.debug_gnss_init_rows(b, blocks[b], g)
            x = e["v"] if g == 0 else e["p"]
            Hx, rx, nz, sats = rows_of(g, ep, rec, Rw, x)
            assert H.shape == Hx.shape and len(res) == len(sats), (b, g, H.shape, Hx.shape)      # m
            assert np.array_equal(res, rx), (b, g)                       # bit-equal to minus the record's residual, in the record's order
            if not len(sats):
                continue
            scale = 1.0 + np.linalg.norm(x)
            assert np.abs(H - Hx).max() <= 1e-12 * scale, (b, g, np.abs(H - Hx).max())
            assert not H[:, 9].any() and not H[:, (3 if g == 0 else 6):(6 if g == 0 else 9)].any(), (b, g)      # the unwritten columns are zero
            assert abs(noise - nz) <= 1e-12 * nz, (b, g, noise, nz)
            Ho, ro, no, so = rows_of(g, ep, orec, Rw, x)                 # the oracle's gnss_residuals at the same receiver
            assert so == sats
            assert np.abs(res - ro).max() < (1e-9 if g == 0 else 1e-6), (b, g)
            assert np.abs(H - Ho).max() <= 1e-12 * scale * 10 and abs(noise - no) <= 1e-9 * no, (b, g)
            tried += 1
    assert tried >= 40
    same_state(s0, state(ctx, B), what="the hook changes nothing")
    ctx.close()


# ---- 2. one call against the round trip and the oracle -----------------------------------------------------------------------------
def test_one_call_equals_the_round_trip_and_the_oracle(mixed, one_call, round_trip, device_records, orc):
    """chi2, noise, dx, P and the table to 1e-9, verdicts, slots and registrations exactly, against two references: the round trip
    (host_acquire) and oracle_acquire on orc.Cov.add_variable_delayed.
    A deviation from the issue, which names oracle_acquire without saying where its residuals come from: here oracle_acquire is fed the
    satellite records of the device front (ingvio_gnss_sat_eval at the overridden receiver), so that the reference and the export consume
    bit-identical residuals and 1e-9 holds for every named quantity.  With the oracle's OWN satellite evaluation (gnss_front_oracle.c) the
    pseudo-range residuals agree with the device front's to 1e-6 m only - the bound of
    test_front_from_the_table_equals_the_host_fed_front_and_the_oracle: metres left over from ranges of 2e7 m - and chi2 and dx, which are
    linear / quadratic in the residuals, cannot hold 1e-9 (chi2 was measured 5e-8 relative apart).  That reference is compared as well,
    further down, in what does not hinge on the last digits of a residual."""
    cases = mixed
    raw, ver, s0, s1, n1, slots1 = one_call
    vh, sh, nh, slots_h = round_trip
    table = chi2()
    n_added = 0
    for b, c in enumerate(cases):
        tab_o, slots_o = copy.deepcopy(c["table"]), list(c["gnss_slots"])
        vo, Po = oracle_acquire(c["P"], tab_o, slots_o, c["epochs"][0], c["spp"], table, rec=device_records[b])
        cands = candidates(c["gnss_slots"], c["spp"]) if c["epochs"][0] is not None else []
        for name, ref in (("round trip", vh[b]), ("oracle", vo)):
            for g in range(CAND):
                d, r = ver[b][g], ref[g]
                assert (d["added"], d["new_idx"], d["slot"]) == (r["added"], r["new_idx"], r["slot"]), (name, b, g, d, r)
                if g not in cands:
                    assert d["chi2"] == 0.0 and d["noise"] == 0.0 and not d["added"], (b, g)
                    continue
                if r["m"] <= 1:                                          # skipped on the device: only it knows the usable satellites
                    assert d["chi2"] == 0.0 and d["noise"] == 0.0, (b, g)
                    continue
                assert abs(d["noise"] - r["noise"]) <= TOL * r["noise"], (name, b, g, d["noise"], r["noise"])
                assert abs(d["chi2"] - r["chi2"]) <= TOL * max(r["chi2"], 1.0), (name, b, g, d["chi2"], r["chi2"])
                if d["added"]:
                    k = d["new_idx"] + 1
                    assert rel(d["dx"][:k], r["dx"][:k]) <= TOL and not d["dx"][k:].any(), (name, b, g, rel(d["dx"][:k], r["dx"][:k]))
        n_added += sum(ver[b][g]["added"] for g in range(CAND))
        assert n1[b] == nh[b] == Po.shape[0] == c["P"].shape[0] + sum(ver[b][g]["added"] for g in range(CAND)), b
        assert list(slots1[b]) == slots_h[b] == slots_o, (b, slots1[b], slots_h[b], slots_o)
        for name, Pref in (("round trip", sh[1][b]), ("oracle", Po)):
            assert rel(s1[1][b], Pref) <= TOL, (name, b, rel(s1[1][b], Pref))
        assert_table(s1[0][b], table_from(sh[0][b]), TOL, ("round trip", b))
        assert_table(s1[0][b], tab_o, TOL, ("oracle", b))
        if not any(ver[b][g]["added"] for g in range(CAND)):             # a filter without candidates (or without an accepted one): bit for bit
            assert n1[b] == c["P"].shape[0] and np.array_equal(s1[1][b], s0[1][b]), b
            for key in TABLE_KEYS:
                assert np.array_equal(s1[0][b][key], s0[0][b][key]), (b, key)
    assert n_added >= 20


def test_one_call_against_the_oracles_own_satellite_evaluation(mixed, one_call, orc):
    """Beyond the issue: oracle_acquire with NO input from the device (residuals of gnss_front_oracle.c, 1e-6 m from the device front's
    in a pseudo-range, 1e-9 m/s in a Doppler residual).  Verdicts, slots and registrations are exact; the noise, P (neither depends on
    the residuals) and the table hold 1e-9.  chi2 and dx are held to what a residual error dr per row allows: with S >= noise^2 I,
    chi2 = |S^-1/2 r|^2 moves by at most 2 sqrt(chi2) sqrt(m) dr / noise; and dx = K r with K = P+ H^T / noise^2 (P+ the round's posterior,
    H the rotated lower rows of [Hx | H_new], whose norm is at most the Frobenius norm of the unrotated block) moves by at most
    lambda_max(P+) |[Hx | H_new]|_F sqrt(m) dr / noise^2.  Both factors come from the oracle's run, none from the device."""
    cases = mixed
    raw, ver, s0, s1, n1, slots1 = one_call
    table = chi2()
    for b, c in enumerate(cases):
        tab_o, slots_o = copy.deepcopy(c["table"]), list(c["gnss_slots"])
        vo, Po = oracle_acquire(c["P"], tab_o, slots_o, c["epochs"][0], c["spp"], table)
        for g in range(CAND):
            d, r = ver[b][g], vo[g]
            assert (d["added"], d["new_idx"], d["slot"]) == (r["added"], r["new_idx"], r["slot"]), (b, g, d, r)
            if r["m"] <= 1 or r["noise"] == 0.0:
                assert d["chi2"] == 0.0 and d["noise"] == 0.0, (b, g)
                continue
            dr = 1e-9 if g == 0 else 1e-6
            assert abs(d["noise"] - r["noise"]) <= TOL * r["noise"], (b, g)
            assert abs(d["chi2"] - r["chi2"]) <= TOL * max(r["chi2"], 1.0) + 2.0 * np.sqrt(r["chi2"] * r["m"]) * dr / r["noise"], (b, g, d["chi2"], r["chi2"])
            if d["added"]:
                k = d["new_idx"] + 1
                bound = TOL * np.linalg.norm(r["dx"][:k]) + r["lam_post"] * r["hnorm"] * np.sqrt(r["m"]) * dr / r["noise"] ** 2
                assert np.linalg.norm(d["dx"][:k] - r["dx"][:k]) <= bound, (b, g, np.linalg.norm(d["dx"][:k] - r["dx"][:k]), bound)
        assert list(slots1[b]) == slots_o and rel(s1[1][b], Po) <= TOL, (b, rel(s1[1][b], Po))
        assert_table(s1[0][b], tab_o, TOL, ("oracle's own front", b))


def test_a_refused_or_skipped_candidate_leaves_the_state_bit_for_bit(mixed):
    """the filters whose ONLY candidate is the one that fails: the SPP fix reports nothing but GLONASS for the filter with one GLONASS
    satellite, nothing but BeiDou for the two with the outlier, nothing for the others"""
    cases = fresh(mixed)
    expect = {}
    for b, c in enumerate(cases):
        pos, vel = np.zeros(7), np.zeros(4)
        g = 2 if c["mixed"].get("one_glo") else (4 if c["mixed"].get("bds_outlier") else None)
        if g is not None:
            pos[2 + g] = c["spp"]["pos_spp"][2 + g]
            expect[b] = g
        c["spp"] = dict(pos_spp=pos, vel_spp=vel)
    assert len(expect) == 3
    ctx = table_ctx(cases, F, gnss=True)
    B = len(cases)
    s0, n0, g0 = state(ctx, B), [ctx.n(b) for b in range(B)], ctx.nominal_get_gnss()
    raw = ctx.gnss_init_nominal(0, init_blocks(cases, 0), chi2(), CHI2_MULT)
    assert not raw["added"].any() and (raw["new_idx"] == -1).all() and (raw["slot"] == -1).all() and not raw["dx"].any() and not raw["status"].any()
    for b in range(B):
        for g in range(CAND):
            if expect.get(b) == g and g == 4:
                assert raw["chi2"][b, g] > CHI2_MULT * chi2()[3] and raw["noise"][b, g] > 0.0, (b, raw["chi2"][b, g])      # refused at m = 3
            else:
                assert raw["chi2"][b, g] == 0.0 and raw["noise"][b, g] == 0.0, (b, g)
    same_state(s0, state(ctx, B), what="refused / skipped")
    assert [ctx.n(b) for b in range(B)] == n0 and np.array_equal(ctx.nominal_get_gnss(), g0)
    ctx.close()


def test_a_partial_range_gives_the_same_bits_and_leaves_the_other_filters(mixed, one_call):
    raw, ver, s0, s1, n1, slots1 = one_call
    ctx = table_ctx(mixed, F, gnss=True)
    B, b0, nb = len(mixed), 2, 3
    part = ctx.gnss_init_nominal(b0, init_blocks(mixed, 0)[b0:b0 + nb], chi2(), CHI2_MULT)
    sp, gp = state(ctx, B), ctx.nominal_get_gnss()
    assert part["added"].sum() >= 10
    for key in ("added", "new_idx", "slot", "chi2", "noise", "dx", "status"):
        assert np.array_equal(part[key], raw[key][b0:b0 + nb]), key
    for b in range(B):
        ref = s1 if b0 <= b < b0 + nb else s0                            # the whole-batch call's result inside the range, the start state outside
        assert np.array_equal(sp[1][b], ref[1][b]), b
        for key in TABLE_KEYS:
            assert np.array_equal(sp[0][b][key], ref[0][b][key]), (b, key)
        assert ctx.n(b) == (n1[b] if b0 <= b < b0 + nb else mixed[b]["P"].shape[0])
        assert list(gp[b]) == (list(slots1[b]) if b0 <= b < b0 + nb else mixed[b]["gnss_slots"]), b
    ctx.close()


# ---- 3. the moved state ------------------------------------------------------------------------------------------------------------
def test_every_round_reads_the_state_the_previous_round_left(mixed, one_call, round_trip):
    cases = mixed
    b = next(i for i, c in enumerate(cases) if c["mixed"].get("moved"))
    ver, s1 = one_call[1][b], one_call[3]
    vh = round_trip[0][b]
    assert all(ver[g]["added"] for g in range(CAND))
    for g in range(CAND):                                                # the per-round host reference
        k = ver[g]["new_idx"] + 1
        assert rel(ver[g]["dx"][:k], vh[g]["dx"][:k]) <= TOL, (g, rel(ver[g]["dx"][:k], vh[g]["dx"][:k]))
    # the read-once variant: p, v taken before the loop
    once = fresh(cases)
    ctx = table_ctx(once, F, gnss=True)
    v1 = host_acquire(ctx, once, 0, chi2(), read_once=True)[b]
    P1 = ctx.cov_get(b)
    ctx.close()
    assert all(v1[g]["added"] for g in range(CAND))
    k = ver[1]["new_idx"] + 1
    assert rel(ver[0]["dx"][:k - 1], v1[0]["dx"][:k - 1]) <= TOL          # the first candidate sees the same state either way
    assert rel(ver[1]["dx"][:k], v1[1]["dx"][:k]) > 100 * TOL, rel(ver[1]["dx"][:k], v1[1]["dx"][:k])
    assert rel(s1[1][b], P1) > 100 * TOL, rel(s1[1][b], P1)


# ---- 4. in the loop ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_cases():
    return make_mixed(load_golden("gnss_front"), n_frames=5)


def test_acquisition_in_the_loop_device_equals_host(loop_cases):
    from ingvio_amd import capi
    table = chi2()
    frames, at = list(range(5)), 1
    ch_cases, cd_cases = fresh(loop_cases), fresh(loop_cases)
    B = len(ch_cases)
    ch = loop_ctx(ch_cases, F)
    tabs = [copy.deepcopy(c["table"]) for c in ch_cases]
    ho, hv = host_loop(ch, ch_cases, tabs, frames, table, at)
    cd = table_ctx(cd_cases, F, gnss=True)
    do, form = device_loop_acquire(cd, cd_cases, frames, table, False, at)
    dv = form.verdicts
    n_added = 0
    for b in range(B):
        for g in range(CAND):
            assert (dv[b][g]["added"], dv[b][g]["new_idx"], dv[b][g]["slot"]) == (hv[b][g]["added"], hv[b][g]["new_idx"], hv[b][g]["slot"]), (b, g)
            n_added += dv[b][g]["added"]
        assert ch_cases[b]["gnss_slots"] == cd_cases[b]["gnss_slots"], b
    assert n_added >= 20
    assert np.array_equal(cd.nominal_get_gnss(), np.array([c["gnss_slots"] for c in cd_cases]))      # registered by the call, never by ingvio_nominal_set_gnss
    for f, (((dxh, acch, rowsh), gh), ((dxd, accd, rowsd), gd)) in enumerate(zip(ho, do)):
        assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd), f      # masks and row counts
        assert np.array_equal(gh[1], gd[1]) and np.array_equal(gh[4], gd[4]), (f, gh[1], gd[1], gh[4], gd[4])      # the epoch's rows, statuses
    # the epoch's rows grow by the acquired constellations: no rows without FS and a clock, rows once they are there
    rows = np.array([g[1] for (_, g) in do])
    for b, c in enumerate(loop_cases):
        had = c["gnss_slots"][4] >= 0 and any(s >= 0 for s in c["gnss_slots"][:4])
        got = sum(dv[b][g]["added"] for g in range(CAND))
        if not had:
            assert not rows[:at + 1, b].any(), b
        if got and c["epochs"][0] is not None and (rows[at + 1:, b] > 0).any():
            assert rows[at + 1:, b].max() > rows[:at + 1, b].max(), (b, rows[:, b])
    assert sum(1 for b, c in enumerate(loop_cases) if c["gnss_slots"][4] < 0 and rows[at + 1:, b].any()) >= 3
    nom = cd.nominal_get()
    for b in range(B):
        assert_table(nom[b], tabs[b], TOL, b)
        Ph, Pd = ch.cov_get(b), cd.cov_get(b)
        assert Ph.shape == Pd.shape and rel(Pd, Ph) <= TOL, (b, rel(Pd, Ph))
    assert all(int(s) in (capi.OK, capi.NEG_DIAG) for s in form.raw["status"])
    ch.close(); cd.close()


def test_acquired_clocks_advance_in_the_imu_steps_without_set_gnss(loop_cases):
    cases = fresh(loop_cases)
    table = chi2()
    ctx = table_ctx(cases, F, gnss=True)
    form = GnssAcquireForm(table, 1)
    book_frame(cases, 0)
    loop = DeviceLoop(ctx, cases, [0, 1, 2], form, pipelined=False)
    loop.start()
    loop.frame(0)
    loop.frame(1)                                                        # the acquisition behind frame 1's epoch; frame 2 is booked
    before = ctx.nominal_get()
    nominal_stage(ctx, cases, 2)()                                       # k_imu_steps of frame 2
    after = ctx.nominal_get()
    moved = 0
    for b, c in enumerate(cases):
        sl, imu = c["gnss_slots"], c["frames"][2]["imu"]
        for g in range(1, CAND):
            if not form.verdicts[b][g]["added"]:
                continue
            s = sl[gpos(g)]
            assert s == form.verdicts[b][g]["slot"] and sl[4] >= 0
            cb, fs = before[b]["val"][s, 9], before[b]["val"][sl[4], 9]
            for q in range(imu.shape[0]):
                cb = cb + imu[q, 6] * fs
            got = after[b]["val"][s, 9]
            assert abs(got - cb) <= 1e-13 * abs(cb) and got != before[b]["val"][s, 9], (b, g, got, cb)
            moved += 1
    assert moved >= 15
    ctx.frame_run(); ctx.frame_fetch()
    ctx.close()


def test_pipelined_loop_with_acquisition_equals_serial_loop(loop_cases):
    table = chi2()
    res = []
    for pipelined in (False, True):
        cases = fresh(loop_cases)
        ctx = table_ctx(cases, F, gnss=True)
        out, form = device_loop_acquire(ctx, cases, list(range(5)), table, pipelined, 1)
        res.append((out, form.raw, state(ctx, len(cases)), ctx.nominal_get_gnss()))
        ctx.close()
    (o0, r0, s0, g0), (o1, r1, s1, g1) = res
    for f, ((fr0, gn0), (fr1, gn1)) in enumerate(zip(o0, o1)):
        for x, y in zip(fr0, fr1):
            assert np.array_equal(x, y), f
        for x, y in zip(gn0, gn1):
            assert np.array_equal(x, y), f
    for key in ("added", "new_idx", "slot", "chi2", "noise", "dx", "status"):
        assert np.array_equal(r0[key], r1[key]), key
    same_state(s0, s1, what="pipelined")
    assert np.array_equal(g0, g1)


# ---- 5. snapshot / restore ---------------------------------------------------------------------------------------------------------
def test_snapshot_restore_replays_the_call_and_the_epoch_behind_it(mixed):
    table = chi2()
    base = fresh(mixed)
    ctx = table_ctx(base, F, gnss=True)
    B = len(base)
    g_start, n_start = ctx.nominal_get_gnss(), [ctx.n(b) for b in range(B)]
    ctx.snapshot()
    runs = []
    for it in range(2):
        cases = fresh(base)
        raw = ctx.gnss_init_nominal(0, init_blocks(cases, 0), table, CHI2_MULT)
        follow(cases, verdicts_of(raw))
        mid = (state(ctx, B), ctx.nominal_get_gnss())
        gnss_stage_call(ctx, gated(cases, 0), 0, table)()                 # an epoch on the acquired clocks, read from the table
        ctx.gnss_run()
        g = ctx.gnss_fetch()
        runs.append((raw, mid, g, state(ctx, B)))
        ctx.restore()
        assert [ctx.n(b) for b in range(B)] == n_start and np.array_equal(ctx.nominal_get_gnss(), g_start)
    (ra, ma, ga, sa), (rb, mb, gb, sb) = runs
    assert ra["added"].sum() >= 20 and (ga[1] > 0).sum() >= 6
    for key in ("added", "new_idx", "slot", "chi2", "noise", "dx", "status"):
        assert np.array_equal(ra[key], rb[key]), key
    same_state(ma[0], mb[0], what="call"); same_state(sa, sb, what="epoch")
    assert np.array_equal(ma[1], mb[1])
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)
    ctx.close()


def test_snapshot_restore_replays_the_loop_with_the_acquisition_bit_for_bit(loop_cases):
    """frames 0-1 without the clocks, the acquisition, frames 2-4 with them; restore; the same loop again from fresh cases (their books,
    slots and frames start over): frame results, epoch results, verdicts, state, sizes and the registered slots give the same bits"""
    table = chi2()
    start = fresh(loop_cases)
    ctx = table_ctx(start, F, gnss=True)
    B = len(start)
    g_start, n_start = ctx.nominal_get_gnss(), [ctx.n(b) for b in range(B)]
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            assert not np.array_equal(ctx.nominal_get_gnss(), g_start)   # the call registered clocks ...
            ctx.restore()
            assert np.array_equal(ctx.nominal_get_gnss(), g_start) and [ctx.n(b) for b in range(B)] == n_start      # ... the restore took them back
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        cases = fresh(loop_cases)
        out, form = device_loop_acquire(ctx, cases, list(range(5)), table, False, 1)
        runs.append((out, form.raw, state(ctx, B), ctx.nominal_get_gnss(), [ctx.n(b) for b in range(B)], [c["gnss_slots"] for c in cases]))
        live = [[c["frames"][f]["new_idx"] + 6 for c in cases] for f in range(5)]      # the state a frame's update sees, the new clone included
    (o0, r0, s0, g0, n0, sl0), (o1, r1, s1, g1, n1, sl1) = runs
    assert r0["added"].sum() >= 20
    for f, ((fr0, gn0), (fr1, gn1)) in enumerate(zip(o0, o1)):
        # dx over the live state: behind it the shared dx buffer keeps what a LATER frame of the first run, on a state grown by the
        # acquisition, left there (tests/test_gpu_nominal_gnss.py compares a GNSS dx the same way)
        for b in range(B):
            assert np.array_equal(fr0[0][b, :live[f][b]], fr1[0][b, :live[f][b]]), (f, b)
            assert np.array_equal(gn0[0][b, :live[f][b]], gn1[0][b, :live[f][b]]), (f, b)
            nf = len(loop_cases[b]["frames"][f]["delta"]["feat_track"])      # the accept mask over the features the frame staged (frame 0: none)
            assert np.array_equal(fr0[1][b, :nf], fr1[1][b, :nf]), (f, b)
        assert np.array_equal(fr0[2], fr1[2]), f                        # the frame's row counts
        assert np.array_equal(gn0[1], gn1[1]) and np.array_equal(gn0[4], gn1[4]), f      # the epoch's rows and statuses
        for b, c in enumerate(loop_cases):                               # keep and gamma over the epoch's candidate rows (behind them: leftovers)
            sl = c["gnss_slots"] if f <= 1 else sl1[b]
            ep = c["epochs"][f]
            if ep is None or sl[4] < 0 or not any(v >= 0 for v in sl[:4]):
                continue
            sys, freq = ep["eph"][:, 0].astype(int), ep["obs"][:, 5]
            m = 2 * sum(1 for q, fq in zip(sys, freq) if 0 <= q <= 3 and fq >= 0 and sl[q] >= 0)
            assert m > 0 and np.array_equal(gn0[2][b, :m], gn1[2][b, :m]) and np.array_equal(gn0[3][b, :m], gn1[3][b, :m]), (f, b)
    for key in ("added", "new_idx", "slot", "chi2", "noise", "dx", "status"):
        assert np.array_equal(r0[key], r1[key]), key
    same_state(s0, s1, what="loop replay")
    assert np.array_equal(g0, g1) and n0 == n1 and sl0 == sl1 and np.array_equal(g1, np.array(sl1))
    ctx.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, b0, nb, arr, table, chi2_len=None, added_ok=True):
    K = CAND
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ai = [np.zeros((max(nb, 1), K), dtype=np.int32) for _ in range(3)]
    ad = [np.zeros((max(nb, 1), K)) for _ in range(2)]
    tab = np.ascontiguousarray(table, dtype=np.float64)
    return ctx.L.ingvio_gnss_init_nominal(ctx.h, b0, nb, arr, tab.ctypes.data_as(dp) if table is not None else None,
                                          len(tab) if chi2_len is None else chi2_len, C.c_double(CHI2_MULT), 1,
                                          ai[0].ctypes.data_as(ip) if added_ok else None, ai[1].ctypes.data_as(ip), ai[2].ctypes.data_as(ip),
                                          ad[0].ctypes.data_as(dp), ad[1].ctypes.data_as(dp), None, None)


def test_refusals_leave_everything_unchanged(mixed):
    from ingvio_amd import capi
    cases = mixed
    table = chi2()
    ctx = table_ctx(cases, F, gnss=True)
    B = len(cases)

    def snap():
        return state(ctx, B), [ctx.n(b) for b in range(B)], ctx.nominal_get_gnss()
    s0 = snap()

    def code(blocks, b0=0, nb=None, edit=None, **kw):
        arr, keep = capi.make_gnss_init_blocks(blocks)
        if edit:
            edit(arr)
        rc = raw_call(ctx, b0, len(blocks) if nb is None else nb, arr, kw.pop("table", table), **kw)
        s1 = snap()
        same_state(s0[0], s1[0])
        assert s0[1] == s1[1] and np.array_equal(s0[2], s1[2])
        return rc
    blocks = init_blocks(cases, 0)
    assert code(blocks[:2], b0=B - 1) == capi.E_ARG                                            # range
    assert code(blocks, nb=0) == capi.E_ARG
    assert code(blocks, added_ok=False) == capi.E_ARG                                          # NULL where data is needed
    assert raw_call(ctx, 0, B, None, table) == capi.E_ARG                                      # no blocks
    assert code(blocks, table=None, chi2_len=40) == capi.E_ARG
    assert code(blocks, chi2_len=12) == capi.E_ARG                                             # chi2_len <= n_sat (12 satellites)
    assert code(blocks, edit=lambda a: setattr(a[0].epoch, "n_sat", 65)) == capi.E_ARG         # n_sat outside 0..64
    assert code(blocks, edit=lambda a: setattr(a[0].epoch, "n_sat", -1)) == capi.E_ARG
    assert code(blocks, edit=lambda a: setattr(a[0].epoch, "eph", None)) == capi.E_ARG         # a missing array
    assert code(blocks, edit=lambda a: setattr(a[2].epoch, "obs", None)) == capi.E_ARG
    # a frame staged from the table / a GNSS epoch staged from the table that has not run
    whole = fresh(cases)
    book_frame(whole, 0)
    nominal_stage(ctx, whole, 0)()
    refused(ctx, lambda: ctx.gnss_init_nominal(0, blocks, table), capi.E_ARG, sizes=True)
    gnss_frame_stage_call(ctx, gated(whole, 0), 0, table)()              # ... and with its in-frame epoch staged as well
    refused(ctx, lambda: ctx.gnss_init_nominal(0, blocks, table), capi.E_ARG, sizes=True)
    ctx.frame_run(); ctx.frame_fetch()
    gnss_stage_call(ctx, gated(whole, 0), 0, table)()
    refused(ctx, lambda: ctx.gnss_init_nominal(0, blocks, table), capi.E_ARG, sizes=True)
    ctx.gnss_run(); ctx.gnss_fetch()
    ctx.close()
    # no table
    bare = loop_ctx(cases[:1], F)
    P0 = bare.cov_get(0)
    arr, keep = capi.make_gnss_init_blocks(blocks[:1])
    assert raw_call(bare, 0, 1, arr, table) == capi.E_ARG and np.array_equal(bare.cov_get(0), P0)
    bare.close()
    # no registered YOF: the reference returns silently (GnssUpdate.cpp:300) - no candidates, not an error
    c0 = [cases[0]]
    ctx = table_ctx(c0, F)
    ctx.nominal_set_gnss(0, [c0[0]["gnss_slots"][:5] + [-1]])
    s0 = state(ctx, 1)
    raw = ctx.gnss_init_nominal(0, blocks[:1], table)
    assert not raw["added"].any() and not raw["chi2"].any() and ctx.n(0) == c0[0]["P"].shape[0]
    same_state(s0, state(ctx, 1), what="no YOF")
    # YOF / the extended pose beyond the live state
    d = c0[0]["table"].as_dict()
    for v in (c0[0]["gnss_slots"][5], d["v_pose"]):
        dd = dict(d, idx=list(d["idx"]))
        dd["idx"][v] = c0[0]["P"].shape[0] + (0 if v != d["v_pose"] else -8)
        ctx.nominal_set(0, [dd]); ctx.nominal_set_gnss(0, [c0[0]["gnss_slots"]])
        refused(ctx, lambda: ctx.gnss_init_nominal(0, blocks[:1], table), capi.E_NOT_IN_STATE, sizes=True)
    ctx.close()
    # capacity: fewer free table slots than candidates; n + candidates > n_max; n_sat > ingvio_mld
    c = cases[0]                                                          # lacks FS, GPS, BDS: three candidates
    n0, d = c["P"].shape[0], c["table"].as_dict()
    free = [i for i, k in enumerate(d["kind"]) if k < 0]
    assert len(free) == 3 and len(candidates(c["gnss_slots"], c["spp"])) == 3
    full = dict(d, kind=list(d["kind"]), idx=list(d["idx"]))             # one of the three free slots taken (a second name for the gyroscope bias)
    full["kind"][free[0]], full["idx"][free[0]] = d["kind"][d["v_bg"]], d["idx"][d["v_bg"]]
    for n_max, v_max, tile in ((n0 + 16, len(d["kind"]), 1), (n0 + 2, 48, 1), (n0 + 16, 48, 6)):
        small = capi.Context(batch=1, n_max=n_max, c_max=6, f_max=F, m_max=8)
        small.cov_set(0, c["P"]); small.tracks_create(F); small.nominal_create(v_max)
        small.nominal_set(0, [full if v_max < 48 else d]); small.nominal_set_gnss(0, [c["gnss_slots"]])
        blk = dict(blocks[0])
        if tile > 1:
            mld = small.L.ingvio_mld(small.h)
            assert mld < 64, mld
            ep = blk["epoch"]
            blk["epoch"] = dict(ep, eph=np.tile(ep["eph"], (tile, 1))[:mld + 1], obs=np.tile(ep["obs"], (tile, 1))[:mld + 1])
        refused(small, lambda: small.gnss_init_nominal(0, [blk], chi2()), capi.E_CAPACITY, sizes=True)
        small.close()


@pytest.mark.parametrize("what", ["landmarks", "split"])
def test_refused_while_other_work_is_pending(what, mixed):
    """a stand-alone landmark update staged from the table and not yet run, a split frame step between its halves: INGVIO_E_ARG, state unchanged"""
    from ingvio_amd import capi, host, synth
    blocks = init_blocks(mixed, 0)[:2]
    table = chi2()
    if what == "split":
        ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
        cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
        ctx.tracks_create(32); ctx.nominal_create(16)
        ctx.snapshot()
        ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
        ctx.frame_run_phase(1, restore_prior=True)
        before = [(ctx.n(b), ctx.cov_get(b)) for b in range(2)]
        arr, keep = capi.make_gnss_init_blocks(blocks)
        assert raw_call(ctx, 0, 2, arr, table) == capi.E_ARG and b"split" in ctx.L.ingvio_last_error(ctx.h)
        for b in range(2):
            assert ctx.n(b) == before[b][0] and np.array_equal(ctx.cov_get(b), before[b][1])
        ctx.frame_run_phase(2)
        ctx.frame_fetch()
        ctx.close()
        return
    import ingvio_amd.closed_loop_lm as clm
    cases, o = clm.make_lm_loop(2, 2), clm.lm_opts()
    ctx = table_ctx(cases)
    ctx.landmark_stage_nominal_prepare(0, clm.nominal_frames(cases, 0), o["stereo"], o["noise"], o["chi2_thr"], o["R_cl2cr"], o["t_cl2cr"], in_frame=False)()
    refused(ctx, lambda: ctx.gnss_init_nominal(0, blocks, table), capi.E_ARG, sizes=True)
    ctx.landmark_run(); ctx.landmark_fetch()
    ctx.close()
