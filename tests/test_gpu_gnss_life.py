"""The GNSS scalars' life cycle in the device-resident closed loop (include/ingvio_hip.h: ingvio_set_gnss_adjust_yof,
ingvio_nominal_add_gnss, ingvio_nominal_marg_gnss): the yaw-offset column of the update rows (k_gnss_front) and of the
acquisition rows (k_delayed_front<DL_GNSS>) against the numpy formulas of ingvio_amd/closed_loop_gnss_life.py, addGNSSVariable and
margGNSSVariable on the table and the covariance bit for bit, and the loop in which YOF enters, FS and the clocks are acquired, the
epochs update behind the frame and inside it, a constellation's clock leaves and comes back - against a host loop (host table, numpy
rows, host-fed entry points for the covariance), pipelined against serial, snapshot against replay, switch on against switch off.
tests/test_gnss_life_model.py shows on the oracle alone that the scenario does all of that.

Shapes: 4 filters, windows of 5-8 clones (one loop at 20), 24 tracks, 8 satellites of three constellations.
Tolerances: rows 1e-12 * scale (tests/test_gpu_gnss_init.py), states, P and table 1e-9 (tests/test_gpu_nominal_gnss.py), verdicts, slots,
registrations and idx exact."""
import copy

import numpy as np
import pytest

from conftest import load_golden
from conftest import rel_err as rel
from ingvio_amd import closed_loop_gnss_life as gl
from ingvio_amd.closed_loop import nominal_stage
from ingvio_amd.closed_loop_gnss import (R_ENU, device_loop_gnss, gnss_frame_stage_call, gnss_stage_call, make_gnss_loop, move_scalars_behind_clones,
                                         rot_z, table_epochs)
from ingvio_amd.closed_loop_gnss_init import CAND, fresh, init_blocks, receiver, rows_of
from nominal_helpers import TABLE_KEYS, assert_table, refused, same_state, table_ctx
from nominal_helpers import device_state as state

pytestmark = pytest.mark.gpu

F = 24
B = 4
TOL = 1e-9                               # tests/test_gpu_nominal_gnss.py
YOF = gl.YOF


def chi2():
    from ingvio_amd import synth
    return synth.chi2_table()


@pytest.fixture(scope="module")
def z():
    return load_golden("gnss_front")


@pytest.fixture(scope="module")
def gnss_cases(z):
    """four filters WITH their six GNSS scalars (behind the clones), an epoch of 8 satellites each"""
    return make_gnss_loop(z, B, 2, every=0, n_sat=gl.N_SAT)


@pytest.fixture(scope="module")
def life_cases(z):
    return gl.make_life_loop(z, B)


# ---- 1. the update rows ------------------------------------------------------------------------------------------------------------
def staged_rows(cases, nominal, on):
    """the rows of epoch 0 as staged, with the switch `on` (None: never touched): (rows per filter, satellite records, the table)"""
    ctx = table_ctx(cases, F, gnss=True)
    if on is not None:
        ctx.set_gnss_adjust_yof(on)
    tab = ctx.nominal_get()
    if nominal:
        gnss_stage_call(ctx, cases, 0, chi2())()
    else:
        ctx.gnss_front_stage(0, table_epochs(tab, cases, 0), chi2(), gate_rows=True, strong_reject=True)
    out = ([ctx.debug_gnss_staged_rows(b) for b in range(len(cases))], ctx.gnss_front_fetch(), tab)
    ctx.gnss_run()
    ctx.close()
    return out


@pytest.mark.parametrize("nominal", [False, True], ids=["host_fed", "from_the_table"])
def test_update_rows_carry_the_yaw_offset_column(gnss_cases, nominal):
    cases = gnss_cases
    rows_on, front, tab = staged_rows(cases, nominal, 1)
    rows_off, front_off, _ = staged_rows(cases, nominal, 0)
    rows_never, _, _ = staged_rows(cases, nominal, None)
    assert np.array_equal(front, front_off)
    for b, c in enumerate(cases):
        (H, res, noise, cm), (H0, res0, noise0, cm0) = rows_on[b], rows_off[b]
        for x, y in zip(rows_off[b], rows_never[b]):                     # switch off = never set, bit for bit
            assert np.array_equal(x, y), b
        assert H.shape == H0.shape == (2 * gl.N_SAT, 14) and np.array_equal(cm, cm0), (b, H.shape)
        assert not H0[:, 9].any(), b                                     # off: exactly zero
        assert np.array_equal(np.delete(H, 9, axis=1), np.delete(H0, 9, axis=1)) and np.array_equal(res, res0) and np.array_equal(noise, noise0), b
        # column 9 from the device's own satellite records and the table's yaw, p_w, v_w
        t, sl = tab[b], c["gnss_slots"]
        yaw, p, v = t["val"][sl[YOF], 9], t["val"][t["v_pose"], 9:12], t["val"][t["v_pose"], 12:15]
        los = front[b, :gl.N_SAT, 2:5]
        assert (front[b, :gl.N_SAT, 9] == 1).all()
        assert cm[9] == t["idx"][sl[YOF]]
        for rows, x in ((slice(0, gl.N_SAT), p), (slice(gl.N_SAT, None), v)):
            want = gl.update_yof_column(los, R_ENU, yaw, x)
            err = np.abs(H[rows, 9] - want).max()
            print("filter", b, "max |col 9|", np.abs(want).max(), "err", err)
            assert err <= 1e-12 * (1.0 + np.linalg.norm(x)), (b, err)
        assert np.abs(H[:, 9]).max() >= 0.1
        # and the whole block against the numpy rows
        ep = table_epochs([t], [c], 0)[0]
        vidx, vsize, Hn, rn, Rn, sats = gl.update_rows(ep, front[b], True)
        assert [int(q) for q in cm] == [i + k for i, s in zip(vidx, vsize) for k in range(s)]
        assert np.abs(H - Hn).max() <= 1e-12 * (1.0 + np.linalg.norm(p)) and np.array_equal(res, rn) and np.abs(noise - Rn).max() <= 1e-12 * Rn.max()


def test_the_switch_is_refused_while_an_epoch_is_staged(gnss_cases):
    from ingvio_amd import capi
    cases = gnss_cases
    ctx = table_ctx(cases, F, gnss=True)
    table = chi2()
    gnss_stage_call(ctx, cases, 0, table)()                               # from the table, not yet run
    refused(ctx, lambda: ctx.set_gnss_adjust_yof(1), capi.E_ARG)
    ctx.gnss_run()
    ctx.set_gnss_adjust_yof(1); ctx.set_gnss_adjust_yof(0)
    ctx.gnss_front_stage(0, table_epochs(ctx.nominal_get(), cases, 0), table, gate_rows=True, strong_reject=True)      # host-fed, not yet run
    refused(ctx, lambda: ctx.set_gnss_adjust_yof(1), capi.E_ARG)
    ctx.gnss_run()
    ctx.set_gnss_adjust_yof(1); ctx.set_gnss_adjust_yof(0)
    nominal_stage(ctx, cases, 0)()
    gnss_frame_stage_call(ctx, cases, 0, table)()                         # with its frame, not yet run
    refused(ctx, lambda: ctx.set_gnss_adjust_yof(1), capi.E_ARG)
    ctx.frame_run(); ctx.frame_fetch()
    ctx.set_gnss_adjust_yof(1)
    ctx.close()


def test_the_folded_in_frame_epoch_carries_the_column(z):
    """the epoch staged with its frame and folded into the MSCKF write-back (scalars in front of the clones, 16 candidate rows), switch
    on: tables and covariances equal the two calls behind the frame to 1e-9, the GNSS dx to 1e-7 of max|dx| (the bounds and their reasons:
    tests/test_gpu_nominal_gnss_inframe.py), and the update moves the yaw offset otherwise than with the switch off"""
    cases = make_gnss_loop(z, B, 3, every=0, scalars_in_front=True, n_sat=gl.N_SAT)
    table = chi2()
    ctxs = [table_ctx(cases, F, gnss=True) for _ in range(3)]
    for ctx, on in zip(ctxs, (1, 1, 0)):
        ctx.set_gnss_adjust_yof(on)
    moved = 0
    for f in range(3):
        res = []
        for ctx, in_frame in zip(ctxs, (True, False, True)):
            nominal_stage(ctx, cases, f)()
            if in_frame:
                gnss_frame_stage_call(ctx, cases, f, table)()
            ctx.frame_run()
            fr = ctx.frame_fetch()
            if not in_frame:
                gnss_stage_call(ctx, cases, f, table)()
                ctx.gnss_run()
            res.append((fr, ctx.gnss_fetch(), ctx.debug_gnss_fused_last(), state(ctx, B)))
        (fa, ga, how_a, sa), (fb, gb, how_b, sb), (fc, gc, how_c, sc) = res
        assert (how_a, how_b, how_c) == (2, 1, 2), (f, how_a, how_b, how_c)      # folded, a pass of its own, folded
        assert np.array_equal(ga[1], gb[1]) and np.array_equal(ga[4], gb[4]) and (ga[1] >= 8).all(), (f, ga[1], gb[1])
        for b, c in enumerate(cases):
            n = c["P"].shape[0]
            da, db = ga[0][b, :n], gb[0][b, :n]
            print("frame", f, "filter", b, "gnss dx: max|diff| / max|dx|", float(np.abs(da - db).max() / np.abs(db).max()))
            assert np.abs(da - db).max() <= 1e-7 * np.abs(db).max(), (f, b)
            for key in ("kind", "idx", "anchor", "clone_var"):
                assert np.array_equal(sa[0][b][key], sb[0][b][key]), (f, b, key)
            live = sa[0][b]["kind"] >= 0
            assert rel(sa[0][b]["val"][live], sb[0][b]["val"][live]) <= TOL and rel(sa[1][b], sb[1][b]) <= TOL, (f, b, rel(sa[1][b], sb[1][b]))
            iy = sa[0][b]["idx"][c["gnss_slots"][YOF]]
            print("   yaw offset dx: switch on", ga[0][b, iy], "off", gc[0][b, iy])
            moved += int(abs(ga[0][b, iy] - gc[0][b, iy]) > 1e-6)        # (off, YOF moves through its prior correlations alone)
    assert moved >= B, moved
    for ctx in ctxs:
        ctx.close()


# ---- 2. the acquisition rows -------------------------------------------------------------------------------------------------------
def test_acquisition_rows_carry_the_column_as_the_reference_writes_it(life_cases):
    cases = fresh(life_cases)
    got = {}
    for on in (1, 0, None):
        cs = fresh(cases)
        ctx = gl.life_ctx(cs, F, adjust_yof=on)
        gl.device_add_yof(ctx, cs)
        s0 = state(ctx, B)
        blocks = init_blocks(cs, 0)
        got[on] = [[ctx.debug_gnss_init_rows(b, blocks[b], g) for g in range(CAND)] for b in range(B)]
        if on:
            recs = [ctx.gnss_sat_eval([receiver(gl_table(ctx, b), c["gnss_slots"], c["epochs"][0], c["spp"])])[0] for b, c in enumerate(cs)]
            tabs = [gl_table(ctx, b) for b in range(B)]
        same_state(s0, state(ctx, B), what="the hook changes nothing")
        ctx.close()
    tried = 0
    for b, c in enumerate(cases):
        t = tabs[b]
        yo, e = next(s for s in t.slots if s is not None and s["kind"] == 3), t.slots[t.v_pose]
        yaw = float(yo["p"][0])
        assert yaw == c["yof"]
        Rw = R_ENU @ rot_z(yaw)
        for g in range(CAND):
            (H, res, noise), (H0, res0, noise0), (Hn, resn, noisen) = got[1][b][g], got[0][b][g], got[None][b][g]
            assert np.array_equal(H0, Hn) and np.array_equal(res0, resn) and noise0 == noisen, (b, g)      # off = never set
            x = e["v"] if g == 0 else e["p"]
            Hx, rx, nz, sats = rows_of(g, c["epochs"][0], recs[b], Rw, x, yaw)
            assert H.shape == Hx.shape == H0.shape and np.array_equal(res, rx) and np.array_equal(res, res0), (b, g, H.shape, Hx.shape)
            if not len(sats):
                continue
            scale = 1.0 + np.linalg.norm(x)
            err = np.abs(H - Hx).max()
            print("filter", b, "candidate", g, "rows", len(sats), "max |col 9|", np.abs(Hx[:, 9]).max(), "err", err)
            assert err <= 1e-12 * scale, (b, g, err)
            assert np.abs(H[:, 9]).max() >= 0.01 and not H0[:, 9].any(), (b, g)
            assert np.array_equal(H[:, :9], H0[:, :9]) and noise == noise0, (b, g)                          # every other entry: the same bits
            # the quirk is kept: the update rows' formula on the same inputs is somewhere else
            assert np.abs(H[:, 9] - gl.update_yof_column(recs[b][sats, 2:5], R_ENU, yaw, x)).max() > 1e-3, (b, g)
            tried += 1
    assert tried >= 4 * B


def gl_table(ctx, b):
    from ingvio_amd.closed_loop_gnss_init import table_from
    return table_from(ctx.nominal_get(b, 1)[0])


# ---- 3. ingvio_nominal_add_gnss ----------------------------------------------------------------------------------------------------
def test_add_gnss_appends_an_independent_block_and_enters_the_table(life_cases):
    from ingvio_amd import capi
    cases = life_cases
    ctx = gl.life_ctx(cases, F)
    s0, n0 = state(ctx, B), [ctx.n(b) for b in range(B)]
    gtype, value, var = [YOF, -1, 4, 0], [0.3, 9.0, 5.1, 152.0], [0.015, 9.0, 1.5, 4.0]
    slot, idx = ctx.nominal_add_gnss(0, gtype, value, var)
    s1 = state(ctx, B)
    reg = ctx.nominal_get_gnss()
    for b, c in enumerate(cases):
        tab, sl = copy.deepcopy(c["table"]), [-1] * 6
        if gtype[b] < 0:
            assert slot[b] == -1 and idx[b] == -1 and ctx.n(b) == n0[b] and (reg[b] == -1).all()
            assert np.array_equal(s1[1][b], s0[1][b])
            for key in TABLE_KEYS:
                assert np.array_equal(s1[0][b][key], s0[0][b][key]), (b, key)
            continue
        want = gl.table_add_gnss(tab, sl, gtype[b], n0[b], value[b])
        assert slot[b] == want == next(i for i, s in enumerate(c["table"].slots) if s is None) and idx[b] == n0[b] and ctx.n(b) == n0[b] + 1
        assert list(reg[b]) == sl
        P = s1[1][b]
        assert P.shape == (n0[b] + 1, n0[b] + 1) and np.array_equal(P[:-1, :-1], s0[1][b])      # the old block: untouched
        assert not P[-1, :-1].any() and not P[:-1, -1].any() and P[-1, -1] == var[b]              # exactly zero, exactly var
        d, h = s1[0][b], tab.as_dict()
        assert list(d["kind"]) == list(h["kind"]) and list(d["idx"]) == list(h["idx"]) and list(d["anchor"]) == list(h["anchor"])
        assert np.array_equal(d["val"], h["val"]) and list(d["clone_var"]) == list(h["clone_var"])
    # a second scalar for a partial range: the other filters' bits stay
    slot2, idx2 = ctx.nominal_add_gnss(2, [YOF, 4], [0.31, 5.0], [0.015, 1.5])
    s2 = state(ctx, B)
    assert list(idx2) == [n0[2] + 1, n0[3] + 1] and ctx.n(2) == n0[2] + 2
    for b in (0, 1):
        assert np.array_equal(s2[1][b], s1[1][b])
        for key in TABLE_KEYS:
            assert np.array_equal(s2[0][b][key], s1[0][b][key]), (b, key)
    assert np.array_equal(s2[1][2][:-1, :-1], s1[1][2]) and s2[1][2][-1, -1] == 0.015 and not s2[1][2][-1, :-1].any()
    reg2 = ctx.nominal_get_gnss()
    assert reg2[2][YOF] == slot2[0] and reg2[2][4] == slot[2] and reg2[3][4] == slot2[1] and reg2[3][0] == slot[3]
    # refusals leave everything unchanged
    refused(ctx, lambda: ctx.nominal_add_gnss(0, [YOF, -1, -1, -1], 0.3, 0.015), capi.E_ARG, sizes=True)          # already registered
    refused(ctx, lambda: ctx.nominal_add_gnss(0, [-1, 6, -1, -1], 0.3, 0.015), capi.E_ARG, sizes=True)            # gtype outside -1..5
    refused(ctx, lambda: ctx.nominal_add_gnss(0, [-1, -2, -1, -1], 0.3, 0.015), capi.E_ARG, sizes=True)
    refused(ctx, lambda: ctx.nominal_add_gnss(3, [1, 1], 0.3, 0.015), capi.E_ARG, sizes=True)                     # range
    book = fresh(cases)
    for b, c in enumerate(book):
        c["book"].n = ctx.n(b)
        c["book"].frame(c["frames"][0])
    nominal_stage(ctx, book, 0)()                                         # a frame staged from the table that has not run
    refused(ctx, lambda: ctx.nominal_add_gnss(0, [1] * B, 0.3, 0.015), capi.E_ARG, sizes=True)
    ctx.frame_run(); ctx.frame_fetch()
    ctx.close()
    # no table; no free slot; n + 1 > n_max
    bare = capi.Context(batch=1, n_max=96, c_max=6, f_max=F, m_max=8)
    bare.cov_set(0, cases[0]["P"])
    with pytest.raises(capi.IngvioError) as e:
        bare.nominal_add_gnss(0, [YOF], 0.3, 0.015)
    assert e.value.code == capi.E_ARG and np.array_equal(bare.cov_get(0), cases[0]["P"])
    bare.close()
    c, d = cases[0], cases[0]["table"].as_dict()
    nP = c["P"].shape[0]
    full = dict(d, kind=list(d["kind"]), idx=list(d["idx"]))
    for i, k in enumerate(full["kind"]):                                  # every free slot taken (more names for the gyroscope bias)
        if k < 0:
            full["kind"][i], full["idx"][i] = d["kind"][d["v_bg"]], d["idx"][d["v_bg"]]
    for n_max, v_max, tab in ((nP + 16, len(d["kind"]), full), (nP, 48, d)):
        small = capi.Context(batch=1, n_max=n_max, c_max=6, f_max=F, m_max=8)
        small.cov_set(0, c["P"]); small.tracks_create(F); small.nominal_create(v_max); small.nominal_set(0, [tab])
        refused(small, lambda: small.nominal_add_gnss(0, [YOF], 0.3, 0.015), capi.E_CAPACITY, sizes=True)
        small.close()


# ---- 4. ingvio_nominal_marg_gnss ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def both_orders(z):
    """filters 0, 1: the scalars in front of the clones; filters 2, 3: behind them (move_scalars_behind_clones)"""
    cases = make_gnss_loop(z, B, 1, every=0, n_sat=gl.N_SAT, scalars_in_front=True)
    for c in cases[2:]:
        move_scalars_behind_clones(c)
    return cases


@pytest.mark.parametrize("masks", [[1 << 2, 1 << 4, 1 << 2, 1 << 4], [0b101001, 0b010110, 0b101001, 0b010110], [0b111111, 0, 1 << YOF, 0b000111]],
                         ids=["one", "three", "all_none_yof_three"])
def test_marg_gnss_deletes_rows_and_columns_in_one_sweep(both_orders, masks):
    cases = both_orders
    front = [min(c["table"].slots[s]["idx"] for s in c["gnss_slots"]) < min(c["table"].slots[v]["idx"] for v in c["table"].clones) for c in cases]
    assert front == [True, True, False, False]
    ctx = table_ctx(cases, F, gnss=True)
    s0, n0 = state(ctx, B), [ctx.n(b) for b in range(B)]
    ctx.nominal_marg_gnss(0, masks)
    s1, reg = state(ctx, B), ctx.nominal_get_gnss()
    for b, c in enumerate(cases):
        tab, sl = copy.deepcopy(c["table"]), list(c["gnss_slots"])
        assert all(s >= 0 for s in sl)
        gone = gl.table_marg_gnss(tab, sl, masks[b])
        assert len(gone) == bin(masks[b]).count("1") and ctx.n(b) == n0[b] - len(gone)
        assert list(reg[b]) == sl, (b, reg[b], sl)
        want = np.delete(np.delete(s0[1][b], gone, axis=0), gone, axis=1)
        assert np.array_equal(s1[1][b], want), b                          # np.delete of the prior on both axes, bitwise
        d, h = s1[0][b], tab.as_dict()
        n = len(h["kind"])
        assert list(d["kind"][:n]) == list(h["kind"]) and list(d["idx"][:n]) == list(h["idx"]) and list(d["anchor"][:n]) == list(h["anchor"]), b
        assert list(d["clone_var"]) == list(h["clone_var"])
        for v in range(n):                                                # no surviving value changes
            if h["kind"][v] >= 0:
                assert np.array_equal(d["val"][v], s0[0][b]["val"][v]), (b, v)
        if not masks[b]:
            for key in TABLE_KEYS:
                assert np.array_equal(s1[0][b][key], s0[0][b][key]), (b, key)
        assert gl.check_state_continuity(tab, ctx.n(b))
    ctx.close()


def test_marg_gnss_refusals_and_the_empty_call(both_orders):
    from ingvio_amd import capi
    cases = both_orders
    ctx = table_ctx(cases, F, gnss=True)
    s0 = state(ctx, B)
    ctx.nominal_marg_gnss(0, [0] * B)                                     # every mask 0: nothing is launched, nothing changes
    same_state(s0, state(ctx, B), what="empty")
    refused(ctx, lambda: ctx.nominal_marg_gnss(0, [1, 1 << 6, 1, 1]), capi.E_ARG, sizes=True)        # bits above 5
    refused(ctx, lambda: ctx.nominal_marg_gnss(3, [1, 1]), capi.E_ARG, sizes=True)                   # range
    ctx.nominal_marg_gnss(1, [1 << 3])
    refused(ctx, lambda: ctx.nominal_marg_gnss(0, [1, 1 << 3, 1, 1]), capi.E_NOT_IN_STATE, sizes=True)      # not registered (any more)
    cs = fresh(cases)
    gnss_stage_call(ctx, cs, 0, chi2())()                                  # a GNSS epoch staged from the table that has not run
    refused(ctx, lambda: ctx.nominal_marg_gnss(0, [1] * B), capi.E_ARG, sizes=True)
    ctx.gnss_run()
    # a table variable beyond the filter's n: every column index the compaction forms has to lie inside the live state
    d = cases[0]["table"].as_dict()
    dd = dict(d, idx=list(d["idx"]))
    dd["idx"][d["v_bg"]] = cases[0]["P"].shape[0] - 2
    ctx.nominal_set(0, [dd]); ctx.nominal_set_gnss(0, [cases[0]["gnss_slots"]])
    refused(ctx, lambda: ctx.nominal_marg_gnss(0, [1]), capi.E_NOT_IN_STATE, sizes=True)
    ctx.close()
    bare = capi.Context(batch=1, n_max=96, c_max=6, f_max=F, m_max=8)
    with pytest.raises(capi.IngvioError) as e:
        bare.nominal_marg_gnss(0, [1])
    assert e.value.code == capi.E_ARG
    bare.close()


# ---- 5. the loop -------------------------------------------------------------------------------------------------------------------
def run_device(cases, frames, pipelined, adjust, c_max=12, probe=False, ctx=None):
    cs = fresh(cases)
    own = ctx is None
    if own:
        ctx = gl.life_ctx(cs, F, c_max=c_max, adjust_yof=adjust)
    snaps = {}
    out, form = gl.device_life(ctx, cs, frames, chi2(), pipelined,
                               probe=(lambda f: snaps.__setitem__(f, (state(ctx, len(cs)), [ctx.n(b) for b in range(len(cs))]))) if probe else None)
    res = dict(out=out, raw=form.raw, verdicts=form.verdicts, how=form.how, snaps=snaps, state=state(ctx, len(cs)), n=[ctx.n(b) for b in range(len(cs))],
               reg=ctx.nominal_get_gnss(), slots=[list(c["gnss_slots"]) for c in cs])
    if own:
        ctx.close()
    return res


def run_host(cases, frames, adjust, c_max=12):
    cs = fresh(cases)
    ch = gl.life_ctx(cs, F, c_max=c_max)
    tabs = [copy.deepcopy(c["table"]) for c in cs]
    snaps = {}
    out, ver = gl.host_life(ch, cs, tabs, frames, chi2(), adjust_yof=adjust,
                            probe=lambda f: snaps.__setitem__(f, (copy.deepcopy(tabs), [ch.cov_get(b) for b in range(len(cs))])))
    ch.close()
    return dict(out=out, verdicts=ver, snaps=snaps, slots=[list(c["gnss_slots"]) for c in cs])


def device_equals_host(dev, hst, frames):
    from ingvio_amd import capi
    worst_t = worst_p = 0.0
    for f in sorted(hst["verdicts"]):
        for b in range(B):
            for g in range(CAND):
                d, h = dev["verdicts"][f][b][g], hst["verdicts"][f][b][g]
                assert (d["added"], d["new_idx"], d["slot"]) == (h["added"], h["new_idx"], h["slot"]), (f, b, g, d, h)
    for i, f in enumerate(frames):
        (fd, gd), (fh, gh) = dev["out"][i], hst["out"][i]
        assert np.array_equal(fd[1], fh[1]) and np.array_equal(fd[2], fh[2]), f              # accept masks, row counts of the frame
        assert (len(gd) > 0) == (len(gh) > 0), f
        if len(gd):
            assert np.array_equal(gd[1], gh[1]) and np.array_equal(gd[4], gh[4]), (f, gd[1], gh[1], gd[4], gh[4])      # the epoch's rows and statuses
            assert all(int(s) in (capi.OK, capi.NEG_DIAG) for s in gd[4]), (f, gd[4])
        (nom, Ps), ns = dev["snaps"][f]
        tabs, Ph = hst["snaps"][f]
        for b in range(B):
            worst_t = max(worst_t, assert_table(nom[b], tabs[b], TOL, (f, b)))
            assert Ps[b].shape == Ph[b].shape and rel(Ps[b], Ph[b]) <= TOL, (f, b, rel(Ps[b], Ph[b]))
            worst_p = max(worst_p, rel(Ps[b], Ph[b]))
            assert gl.check_state_continuity(tabs[b], ns[b]), (f, b)
    assert dev["slots"] == hst["slots"] and np.array_equal(dev["reg"], np.array(dev["slots"]))
    print("worst table value", worst_t, "worst covariance", worst_p)


@pytest.fixture(scope="module")
def serial_on(life_cases):
    return run_device(life_cases, list(range(8)), False, 1, probe=True)


def test_the_loop_device_equals_host(life_cases, serial_on):
    frames = list(range(8))
    hst = run_host(life_cases, frames, True)
    dev = serial_on
    device_equals_host(dev, hst, frames)
    # what the scenario did, on the device's results: FS and three clocks behind frame 0, Galileo's clock again behind frame 5
    for b in range(B):
        assert [g for g in range(CAND) if dev["verdicts"][0][b][g]["added"]] == [0, 1, 3, 4], (b, dev["verdicts"][0][b])
        assert [g for g in range(CAND) if dev["verdicts"][5][b][g]["added"]] == [3], (b, dev["verdicts"][5][b])
        n = [dev["snaps"][f][1][b] for f in frames]
        n0 = life_cases[b]["P"].shape[0]
        assert n == [n0 + 5, n0 + 5, n0 + 4, n0 + 4, n0 + 4, n0 + 5, n0 + 5, n0 + 5], (b, n, n0)
        rows = [int(dev["out"][f][1][1][b]) for f in range(1, 8)]
        print("filter", b, "epoch rows kept", rows, "in-frame epochs applied as", dev["how"])
        assert min(rows) >= 6 and max(rows[2:4]) <= 12, (b, rows)         # the epochs update; frames 3, 4 lack Galileo's four rows
        assert dev["reg"][b][1] == -1 and (dev["reg"][b][[0, 2, 3, 4, 5]] >= 0).all()


def test_the_yaw_offset_is_estimated_only_with_the_switch(life_cases, serial_on):
    off = run_device(life_cases, list(range(8)), False, 0)
    for b, c in enumerate(life_cases):
        for res, on in ((serial_on, True), (off, False)):
            t, P = res["state"][0][b], res["state"][1][b]
            sl = res["reg"][b][YOF]
            yaw, var = t["val"][sl, 9], P[t["idx"][sl], t["idx"][sl]]
            print("filter", b, "switch", on, "yaw", yaw, "variance", var)
            if on:
                assert var < gl.INIT_COV_YOF and yaw != c["yof"], (b, var, yaw)
            else:
                assert var == gl.INIT_COV_YOF and yaw == c["yof"], (b, var, yaw)
        assert serial_on["state"][0][b]["val"][serial_on["reg"][b][YOF], 9] != off["state"][0][b]["val"][off["reg"][b][YOF], 9]


CAND_ROWS = {1: 16, 2: 16, 3: 12, 4: 12, 5: 12, 6: 16, 7: 16}             # candidate rows of the script's epochs: two per satellite whose clock is in the state


def same_runs(a, b, frames, what, live=None, cases=None):
    """live: per filter the columns of dx to compare, and keep / gamma over the candidate rows only - two runs on ONE context, whose shared
    buffers keep behind the live entries what an earlier, larger state left there (tests/test_gpu_gnss_init.py compares a replay the same way)"""
    for i, f in enumerate(frames):
        (fa, ga), (fb, gb) = a["out"][i], b["out"][i]
        assert len(ga) == len(gb)
        if live is None:
            for x, y in zip(list(fa) + list(ga), list(fb) + list(gb)):
                assert np.array_equal(x, y), (what, f)
            continue
        for q in range(B):
            assert np.array_equal(fa[0][q, :live[q]], fb[0][q, :live[q]]), (what, f, q)
            if len(ga):
                m = CAND_ROWS[f]
                assert np.array_equal(ga[0][q, :live[q]], gb[0][q, :live[q]]), (what, f, q)
                assert np.array_equal(ga[2][q, :m], gb[2][q, :m]) and np.array_equal(ga[3][q, :m], gb[3][q, :m]), (what, f, q)
            nf = len(cases[q]["frames"][f]["delta"]["feat_track"])       # the accept mask over the features the frame staged (frame 0: none)
            assert np.array_equal(fa[1][q, :nf], fb[1][q, :nf]), (what, f, q)
        assert np.array_equal(fa[2], fb[2]), (what, f)
        if len(ga):
            assert np.array_equal(ga[1], gb[1]) and np.array_equal(ga[4], gb[4]), (what, f)
    assert sorted(a["raw"]) == sorted(b["raw"])
    for f in a["raw"]:
        for key in ("added", "new_idx", "slot", "chi2", "noise", "dx", "status"):
            assert np.array_equal(a["raw"][f][key], b["raw"][f][key]), (what, f, key)
    same_state(a["state"], b["state"], what=what)
    assert a["n"] == b["n"] and np.array_equal(a["reg"], b["reg"]) and a["slots"] == b["slots"] and a["how"] == b["how"]


def test_pipelined_loop_equals_serial_loop(life_cases, serial_on):
    same_runs(serial_on, run_device(life_cases, list(range(8)), True, 1), list(range(8)), "pipelined")


def test_snapshot_restore_replays_the_loop_bit_for_bit(life_cases):
    frames = list(range(8))
    ctx = gl.life_ctx(fresh(life_cases), F, adjust_yof=1)
    n_start = [ctx.n(b) for b in range(B)]
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            assert (ctx.nominal_get_gnss() >= 0).any()
            ctx.restore()
            assert (ctx.nominal_get_gnss() == -1).all() and [ctx.n(b) for b in range(B)] == n_start      # the scalars left with the restore
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        runs.append(run_device(life_cases, frames, False, 1, ctx=ctx))
    ctx.close()
    same_runs(runs[0], runs[1], frames, "replay", live=[n + 1 + 6 for n in n_start], cases=life_cases)      # every frame's update sees at least YOF and the new clone


def test_the_loop_with_a_window_of_twenty_clones(z):
    """the large-window frame path (windows beyond 16 clones) behind and around the epochs: frames 0-3 of the script - acquisition, an
    epoch behind the frame, an epoch staged with the frame (never folded at this width), the drop, an epoch without Galileo"""
    cases = gl.make_life_loop(z, B, 4, windows=(20,))
    assert all(c["C"] == 20 for c in cases)
    frames = list(range(4))
    dev = run_device(cases, frames, False, 1, c_max=21, probe=True)
    hst = run_host(cases, frames, True, c_max=21)
    device_equals_host(dev, hst, frames)
    assert dev["how"] == {2: 1}                                          # a pass of its own behind the frame
    for b in range(B):
        assert sum(dev["verdicts"][0][b][g]["added"] for g in range(CAND)) == 4, b


# ---- 6. switch off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_frame", [False, True], ids=["behind", "in_frame"])
def test_switch_off_is_bit_identical_to_never_setting_it(z, in_frame):
    cases = make_gnss_loop(z, B, 4, scalars_in_front=in_frame, n_sat=gl.N_SAT if in_frame else None)
    frames = list(range(4))
    res = []
    for touch in (False, True):
        ctx = table_ctx(cases, F, gnss=True)
        if touch:
            ctx.set_gnss_adjust_yof(1)
            ctx.set_gnss_adjust_yof(0)
        out = device_loop_gnss(ctx, cases, frames, chi2(), False, in_frame=in_frame)
        res.append((out, state(ctx, B)))
        ctx.close()
    (o0, s0), (o1, s1) = res
    for f, ((fr0, g0), (fr1, g1)) in enumerate(zip(o0, o1)):
        for x, y in zip(list(fr0) + list(g0), list(fr1) + list(g1)):
            assert np.array_equal(x, y), f
    same_state(s0, s1, what="switch off")
    assert any((g[1] > 0).any() for _, g in o0)
