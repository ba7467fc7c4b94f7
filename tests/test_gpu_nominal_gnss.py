"""GNSS epochs in the device-resident closed loop (include/ingvio_hip.h: ingvio_nominal_set_gnss, ingvio_gnss_front_stage_nominal, the
nominal ingvio_gnss_run): the receiver clocks advance with the frequency shift in k_imu_steps<true>, the GNSS front reads the
receiver from the table, and the update ends with boxPlus on the device.  Checked against the host's sequential clock recursion, against
the host-fed front on the same table values (bit for bit), against the oracle, and against a host loop built from the host-fed entry
points.  Inputs: ingvio_amd/closed_loop_gnss.py (satellites: tests/golden/gnss_front.npz; the GNSS scalars lie BEHIND the start
window's clones, so the frames' marginalisations shift their idx).

dx of a GNSS update is compared over the live state [0, n): the host-fed run leaves the frame's entries behind n in the shared dx
buffer, the nominal run's own buffer holds zeros there."""
import copy

import numpy as np
import pytest

from conftest import load_golden
from conftest import rel_err as rel
from ingvio_amd.closed_loop import loop_ctx, nominal_stage
from ingvio_amd.closed_loop_gnss import R_ENU, device_loop_gnss, gnss_stage_call, host_step_gnss, make_gnss_loop, rot_z, table_epochs
from nominal_helpers import TABLE_KEYS, assert_table, refused, same_state, table_ctx
from nominal_helpers import device_state as state

pytestmark = pytest.mark.gpu

F = 24


def chi2():
    from ingvio_amd import synth
    return synth.chi2_table()


def same_gnss(cases, f, ga, gb, ns, what=""):
    """dx over the live state, rows, keep and gamma of the candidate rows, status"""
    for b, c in enumerate(cases):
        n = c["P"].shape[0]
        assert np.array_equal(ga[0][b, :n], gb[0][b, :n]), (what, b)
        assert ga[1][b] == gb[1][b] and ga[4][b] == gb[4][b], (what, b)
        if c["epochs"][f] is not None:
            assert np.array_equal(ga[2][b, :2 * ns], gb[2][b, :2 * ns]) and np.array_equal(ga[3][b, :2 * ns], gb[3][b, :2 * ns]), (what, b)


# ---- 1. the clock recursion of k_imu_steps<true> ---------------------------------------------------------------------------------
def test_clock_recursion_matches_the_sequential_host_sum():
    z = load_golden("gnss_front")
    cases = make_gnss_loop(z, 10, 1, ks=(1, 9, 10, 33, 64))
    B = len(cases)
    assert sorted({c["frames"][0]["imu"].shape[0] for c in cases}) == [1, 9, 10, 33, 64]
    full = [list(c["gnss_slots"]) for c in cases]
    partly = [sl if b < 5 else [sl[0], -1, sl[2], -1, sl[4], sl[5]] for b, sl in enumerate(full)]      # k 1..64 with GLO and BDS absent
    no_fs = [sl[:4] + [-1, sl[5]] for sl in full]

    def staged(slots, eg):
        ctx = table_ctx(cases, F)
        if slots is not None:
            ctx.nominal_set_gnss(0, slots)
            assert np.array_equal(ctx.nominal_get_gnss(), np.array(slots))
        before = ctx.nominal_get()
        nominal_stage(ctx, cases, 0, enable_gnss=eg)()
        after = ctx.nominal_get()                                        # after the stage, before the run
        ctx.frame_run()
        res = (before, after, ctx.frame_fetch(), [ctx.cov_get(b) for b in range(B)])
        ctx.close()
        return res

    refs = {eg: staged(None, eg) for eg in (0, 1)}                       # no registration: the scalars stay, with and without enable_gnss
    for ref in refs.values():
        for b, c in enumerate(cases):
            for s in c["gnss_slots"]:
                assert np.array_equal(ref[0][b]["val"][s], ref[1][b]["val"][s]), b
    moved = 0
    for name, slots, eg in (("all", full, 1), ("partly", partly, 1), ("no_fs", no_fs, 1), ("disabled", full, 0)):
        before, after, frame, Ps = staged(slots, eg)
        ref = refs[eg]
        for b, c in enumerate(cases):
            sl, imu = slots[b], c["frames"][0]["imu"]
            on = eg and sl[4] >= 0
            clocks = {c["gnss_slots"][s]: sl[s] >= 0 for s in range(4)}
            for v in range(len(after[b]["kind"])):
                if on and clocks.get(v, False):
                    cb, fs = before[b]["val"][v, 9], before[b]["val"][sl[4], 9]
                    for q in range(imu.shape[0]):
                        cb = cb + imu[q, 6] * fs
                    got = after[b]["val"][v, 9]
                    assert abs(got - cb) <= 1e-13 * abs(cb), (name, b, got, cb)
                    assert got != before[b]["val"][v, 9]
                    assert np.array_equal(np.delete(after[b]["val"][v], 9), np.delete(before[b]["val"][v], 9))
                    moved += 1
                else:                                                    # absent / disabled / not a clock: R, p, v and every other value
                    assert np.array_equal(after[b]["val"][v], ref[1][b]["val"][v]), (name, b, v)
            for key in ("kind", "idx", "anchor", "clone_var"):
                assert np.array_equal(after[b][key], ref[1][b][key]), (name, b, key)
            # Phi, G and the staged frame: the frame that runs on them gives the same bits
            assert np.array_equal(Ps[b], ref[3][b]), (name, b)
        for x, y in zip(frame, ref[2]):
            assert np.array_equal(x, y), name
    assert moved == 10 * 4 + (5 * 4 + 5 * 2)


# ---- 2. the front from the table -------------------------------------------------------------------------------------------------
def test_front_from_the_table_equals_the_host_fed_front_and_the_oracle(orc):
    z = load_golden("gnss_front")
    cases = make_gnss_loop(z, 6, 1, every=0)
    B, ns = len(cases), len(z["eph"])
    table = chi2()
    res = []
    for nominal in (True, False):
        ctx = table_ctx(cases, F, gnss=True)
        nominal_stage(ctx, cases, 0)()
        ctx.frame_run()
        ctx.frame_fetch()
        tab = ctx.nominal_get()
        if nominal:
            gnss_stage_call(ctx, cases, 0, table)()
        else:
            ctx.gnss_front_stage(0, table_epochs(tab, cases, 0), table, gate_rows=True, strong_reject=True)
        front = ctx.gnss_front_fetch()
        ctx.gnss_run()
        res.append((tab, front, ctx.gnss_fetch(), state(ctx, B)))
        ctx.close()
    (tab, fa, ga, sa), (tab_b, fb, gb, sb) = res
    for b, c in enumerate(cases):                                        # the frame marginalised a clone in front of the scalars
        fs_slot = c["gnss_slots"][4]
        assert tab[b]["idx"][fs_slot] == c["table"].slots[fs_slot]["idx"] - 6
        for key in TABLE_KEYS:
            assert np.array_equal(tab[b][key], tab_b[b][key])
    assert np.array_equal(fa, fb)
    same_gnss(cases, 0, ga, gb, ns)
    assert (ga[1] > 0).any() and (ga[4] == 0).any()                      # the comparison carried real updates
    # the table after the run: the host-fed context has not retracted; its boxPlus with the fetched dx gives the nominal one's table
    for b in range(B):
        assert np.array_equal(sa[1][b], sb[1][b]), b
        assert np.array_equal(sb[0][b]["val"], tab[b]["val"])
        assert not np.array_equal(sa[0][b]["val"], tab[b]["val"]) or ga[1][b] == 0 or ga[4][b] != 0
    for b, c in enumerate(cases):
        e, sl, t = c["epochs"][0], c["gnss_slots"], tab[b]
        Rw = R_ENU @ rot_z(t["val"][sl[5], 9])
        xyzt = np.r_[Rw @ t["val"][t["v_pose"], 9:12] + e["anchor_ecef"], [t["val"][s, 9] for s in sl[:4]]]
        velt = np.r_[Rw @ t["val"][t["v_pose"], 12:15], t["val"][sl[4], 9]]
        o = orc.gnss_residuals(e["eph"], e["obs"], e["ion"], e["doy"], xyzt, velt)
        f = fa[b, :ns]
        assert np.array_equal(f[:, 9].astype(int), o["usable"])
        assert np.abs(f[:, 0] - o["res_pos"]).max() < 1e-6 and np.abs(f[:, 1] - o["res_vel"]).max() < 1e-9
        assert np.abs(f[:, 2:5] - o["los"]).max() < 1e-12 and np.abs(f[:, 5:7] - o["azel"]).max() < 1e-11 and np.abs(f[:, 7:9] - o["atmos"]).max() < 1e-9


# ---- 3. the closed loop ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_cases():
    return make_gnss_loop(load_golden("gnss_front"), 24, 13)


def test_closed_loop_with_gnss_device_equals_host(loop_cases):
    from ingvio_amd import capi
    cases = loop_cases
    B, ns = len(cases), 12
    table = chi2()
    ch, cd = loop_ctx(cases, F), table_ctx(cases, F, gnss=True)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    epochs = ok = 0
    for f in range(len(cases[0]["frames"])):
        (dxh, acch, rowsh), gh = host_step_gnss(ch, cases, tabs, f, table)
        nominal_stage(cd, cases, f)()
        cd.frame_run()
        dxd, accd, rowsd = cd.frame_fetch()
        gnss_stage_call(cd, cases, f, table)()
        cd.gnss_run()
        gd = cd.gnss_fetch()
        assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd), f
        assert np.array_equal(gh[1], gd[1]) and np.array_equal(gh[4], gd[4]), (f, gh[1], gd[1], gh[4], gd[4])
        for b, c in enumerate(cases):
            if c["epochs"][f] is None:
                assert gd[1][b] == 0 and not gd[0][b].any(), (f, b)
                continue
            assert np.array_equal(gh[2][b, :2 * ns], gd[2][b, :2 * ns]), (f, b)
            # the condition of the comparison, on the HOST loop's results: the update is exercised
            assert gh[1][b] >= 8, (f, b, gh[1][b])
            epochs += 1
            ok += int(gh[4][b] == capi.OK)
        nom = cd.nominal_get()
        for b in range(B):
            assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph, Pd = ch.cov_get(b), cd.cov_get(b)
            assert Ph.shape == Pd.shape and rel(Pd, Ph) <= 1e-9, (f, b, rel(Pd, Ph))
    assert epochs == 16 * 13 and ok >= 0.9 * epochs, (epochs, ok)
    ch.close(); cd.close()


# ---- 4. pipelined = serial -------------------------------------------------------------------------------------------------------
def test_pipelined_gnss_loop_equals_serial_loop(loop_cases):
    cases = loop_cases
    B = len(cases)
    table = chi2()
    res = []
    for pipelined in (False, True):
        ctx = table_ctx(cases, F, gnss=True)
        out = device_loop_gnss(ctx, cases, list(range(len(cases[0]["frames"]))), table, pipelined, sync_every_call=not pipelined)
        res.append((out, state(ctx, B)))
        ctx.close()
    (o0, s0), (o1, s1) = res
    for f, ((fr0, g0), (fr1, g1)) in enumerate(zip(o0, o1)):
        for x, y in zip(fr0, fr1):                                       # frame_fetch_end(f) after gnss_run(f): frame f's MSCKF results
            assert np.array_equal(x, y), f
        assert fr1[2].sum() == 0 or fr1[0].any()
        same_gnss(cases, f, g0, g1, 12, f)
    same_state(s0, s1)


# ---- 5. snapshot / restore -------------------------------------------------------------------------------------------------------
def test_snapshot_restore_replays_the_gnss_loop_bit_for_bit(loop_cases):
    cases = loop_cases
    B, N = len(cases), 6
    table = chi2()
    ctx = table_ctx(cases, F, gnss=True)
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            ctx.nominal_set_gnss(0, [[-1] * 6] * B)                      # the registration travels with the snapshot
            ctx.restore()
            assert np.array_equal(ctx.nominal_get_gnss(), np.array([c["gnss_slots"] for c in cases]))
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        out = device_loop_gnss(ctx, cases, list(range(N)), table, False)
        runs.append((out, state(ctx, B)))
    (o0, s0), (o1, s1) = runs
    for f, ((fr0, g0), (fr1, g1)) in enumerate(zip(o0, o1)):
        assert np.array_equal(fr0[0], fr1[0]) and np.array_equal(fr0[2], fr1[2]), f
        same_gnss(cases, f, g0, g1, 12, f)
    same_state(s0, s1)
    ctx.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_table_covariance_and_staged_rows_unchanged(loop_cases):
    from ingvio_amd import capi
    cases = loop_cases[:4]                                               # filter 2 has no epochs
    B = len(cases)
    table = chi2()
    slots = [c["gnss_slots"] for c in cases]
    tabs = [c["table"].as_dict() for c in cases]

    # -- ingvio_nominal_set_gnss
    ctx = loop_ctx(cases, F)
    with pytest.raises(capi.IngvioError) as e:
        ctx.nominal_set_gnss(0, slots)                                   # no table
    assert e.value.code == capi.E_ARG
    with pytest.raises(capi.IngvioError) as e:
        gnss_stage_call(ctx, cases, 0, table)()                          # no table, n_sat > 0
    assert e.value.code == capi.E_ARG
    P0 = [ctx.cov_get(b) for b in range(B)]
    with pytest.raises(capi.IngvioError) as e:
        ctx.gnss_front_stage_nominal(0, [None] * B, table, gate_rows=True, strong_reject=True)      # no table, no satellite anywhere
    assert e.value.code == capi.E_ARG
    with pytest.raises(capi.IngvioError) as e:
        ctx.gnss_run(0, B)                                               # ... and nothing was staged
    assert e.value.code == capi.E_ARG
    for b in range(B):
        assert np.array_equal(P0[b], ctx.cov_get(b))
    ctx.nominal_create(48)
    ctx.nominal_set(0, tabs)
    refused(ctx, gnss_stage_call(ctx, cases, 0, table), capi.E_ARG)      # no registered slots
    for bad in (48, 200, -2, cases[0]["table"].v_bg, cases[0]["table"].clones[0], 47):      # out of range / not a Scalar / a free slot
        refused(ctx, lambda: ctx.nominal_set_gnss(0, [[bad] + list(slots[0][1:])] + slots[1:]), capi.E_ARG)
    assert (ctx.nominal_get_gnss() == -1).all()
    ctx.nominal_set_gnss(0, slots)
    ctx.nominal_set(1, tabs[1:2])                                        # a new table for filter 1 clears its registration only
    got = ctx.nominal_get_gnss()
    assert (got[1] == -1).all() and np.array_equal(got[[0, 2, 3]], np.array(slots)[[0, 2, 3]])
    ctx.nominal_set_gnss(1, slots[1:2])
    # -- the stage: in_frame, missing variables, a frame staged and not yet run
    refused(ctx, ctx.gnss_front_stage_nominal_prepare(0, [c["epochs"][0] for c in cases], table, in_frame=True), capi.E_UNSUPPORTED)
    for miss in (4, 5):                                                  # FS, YOF not in the state
        ctx.nominal_set_gnss(0, [[-1 if s == miss else v for s, v in enumerate(slots[0])]])
        refused(ctx, gnss_stage_call(ctx, cases, 0, table), capi.E_NOT_IN_STATE)
    # the extended pose not in the table
    ctx.nominal_set(0, [dict(tabs[0], v_pose=-1)])
    ctx.nominal_set_gnss(0, slots[0:1])
    refused(ctx, gnss_stage_call(ctx, cases, 0, table), capi.E_NOT_IN_STATE)
    ctx.nominal_set(0, tabs[0:1])
    ctx.nominal_set_gnss(0, slots[0:1])
    # the capacity checks of the host-fed front: more satellites than the ABI takes, more rows than the row buffers hold
    mld = ctx.L.ingvio_mld(ctx.h)
    n_over = mld // 2 + 1
    assert n_over <= 64
    ep0 = cases[0]["epochs"][0]
    for n_sat, code in ((65, capi.E_ARG), (n_over, capi.E_CAPACITY)):
        big = dict(ep0, eph=np.tile(ep0["eph"], (6, 1))[:n_sat], obs=np.tile(ep0["obs"], (6, 1))[:n_sat])
        refused(ctx, ctx.gnss_front_stage_nominal_prepare(0, [big] + [c["epochs"][0] for c in cases[1:]], table, strong_reject=True), code)
    # all of it without a satellite anywhere is a stage without rows: its run leaves table and covariance alone
    s0 = state(ctx, B)
    ctx.gnss_front_stage_nominal(0, [None] * B, table, gate_rows=True, strong_reject=True)
    ctx.gnss_run()
    g0 = ctx.gnss_fetch()
    assert not g0[0].any() and not g0[1].any() and not g0[4].any()
    same_state(s0, state(ctx, B))
    nominal_stage(ctx, cases, 0)()
    refused(ctx, gnss_stage_call(ctx, cases, 0, table), capi.E_ARG)
    refused(ctx, lambda: ctx.nominal_set_gnss(0, slots), capi.E_ARG)
    ctx.frame_run()
    ctx.frame_fetch()
    # -- while the epoch is staged and has not run
    gnss_stage_call(ctx, cases, 0, table)()
    front = ctx.gnss_front_fetch()
    refused(ctx, nominal_stage(ctx, cases, 1), capi.E_ARG)
    refused(ctx, lambda: ctx.nominal_set(0, tabs), capi.E_ARG)
    refused(ctx, lambda: ctx.nominal_box_plus(0, np.zeros((B, ctx.ldp))), capi.E_ARG)
    refused(ctx, lambda: ctx.nominal_set_gnss(0, slots), capi.E_ARG)
    refused(ctx, lambda: ctx.snapshot(), capi.E_ARG)
    refused(ctx, lambda: ctx.gnss_run(0, B - 1), capi.E_ARG)             # not the staged range
    assert np.array_equal(front, ctx.gnss_front_fetch())                 # the staged rows' source is untouched
    s0 = state(ctx, B)
    ctx.gnss_run()
    g1 = ctx.gnss_fetch()
    s1 = state(ctx, B)
    if g1[1][0] > 0 and g1[4][0] == capi.OK:
        assert not np.array_equal(s0[0][0]["val"], s1[0][0]["val"])      # the update's dx reached the table
    assert np.array_equal(s0[0][2]["val"], s1[0][2]["val"]) and np.array_equal(s0[1][2], s1[1][2])      # no epoch: dx = 0 is the identity
    refused(ctx, lambda: ctx.gnss_run(), capi.E_ARG)                     # once: the table is not retracted twice
    g2 = ctx.gnss_fetch()                                                # the results stay fetchable
    for x, y in zip(g1, g2):
        assert np.array_equal(x, y)
    # -- a host-fed stage on a context with a table still works, may be repeated and leaves the table alone
    tab = ctx.nominal_get()
    ctx.gnss_front_stage(0, table_epochs(tab, cases, 1), table, gate_rows=True, strong_reject=True)
    ctx.gnss_run()
    ctx.gnss_run()
    ctx.gnss_fetch()
    t2 = ctx.nominal_get()
    for b in range(B):
        for key in TABLE_KEYS:
            assert np.array_equal(tab[b][key], t2[b][key]), (b, key)
    # -- a restore abandons a staged epoch; the in-frame stage with the table stays refused
    ctx.snapshot()
    s0 = state(ctx, B)
    gnss_stage_call(ctx, cases, 1, table)()
    ctx.restore()
    same_state(s0, state(ctx, B))
    refused(ctx, lambda: ctx.gnss_run(), capi.E_ARG)
    nominal_stage(ctx, cases, 1)()                                       # ... and the loop goes on
    ctx.frame_run()
    blk = ([0], [9], np.eye(1, 9), np.zeros(1), np.ones(1))
    ctx.gnss_stage(0, [blk] * B, table, in_frame=True)
    refused(ctx, nominal_stage(ctx, cases, 2), capi.E_UNSUPPORTED)
    ctx.close()
