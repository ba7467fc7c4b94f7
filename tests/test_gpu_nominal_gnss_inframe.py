"""The GNSS epoch staged WITH its frame in the device-resident closed loop (include/ingvio_hip.h: ingvio_gnss_frame_stage_nominal; DESIGN
4.5, 4.11): ingvio_frame_run forms the epoch's rows on the device at the state after the MSCKF update and applies them - folded into the
MSCKF write-back where that is possible (one read and one write of P for MSCKF update, GNSS update and marginalisation, then one
retraction with drop and shift: k_nominal_update_post), else as the kernels of ingvio_gnss_front_stage_nominal + ingvio_gnss_run behind
the frame.  Checked against the host loop in the reference's order built from the host-fed entry points, against the device two-call
form, pipelined against serial, snapshot against replay, the new retraction kernel alone against the host table, and every refusal.

Inputs: ingvio_amd/closed_loop_gnss.py.  The fold's loops keep the GNSS scalars in front of the clones and the fixture's first eight
satellites (four GPS, two Galileo, two BDS: 16 candidate rows, the fold's limit); the default loop (scalars behind the clones, 11 usable
satellites) cannot fold.

Bounds.  Tables and covariances: 1e-9, the bound of every closed-loop test here.  GNSS dx of the fold against another form: 1e-7 of
max|dx| - the two forms hand the front receiver positions that differ in the last bits, one ulp of an ECEF coordinate (6.4e6 m: 9e-10 m)
or of a pseudo-range (2.6e7 m: 4e-9 m) moves a residual of the order of a metre by some 1e-9 of itself, and a handful of them add up.
The retraction kernel alone: 1e-13 as tests/test_gpu_nominal_state.py has it for the other retractions."""
import copy

import numpy as np
import pytest

from conftest import load_golden
from conftest import rel_err as rel
from ingvio_amd.closed_loop import LM, DeviceLoop, loop_ctx, nominal_stage
from ingvio_amd.closed_loop_gnss import (GnssForm, GnssInFrameForm, gnss_frame_stage_call, gnss_stage_call, host_step_gnss,
                                         make_gnss_loop)
from ingvio_amd.closed_loop_lm import lm_opts, lm_stage_call, make_lm_loop
from nominal_helpers import assert_table, refused, same_state, table_ctx
from nominal_helpers import device_state as state
from test_gpu_nominal_state import random_dx, random_table

pytestmark = pytest.mark.gpu

F = 24
NS = 8                                                                   # satellites of the fold's epochs
FOLDED, OWN_PASS = 2, 1                                                  # ingvio_debug_gnss_fused_last


def chi2():
    from ingvio_amd import synth
    return synth.chi2_table()


@pytest.fixture(scope="module")
def fold_cases():
    return make_gnss_loop(load_golden("gnss_front"), 12, 8, scalars_in_front=True, n_sat=NS)


@pytest.fixture(scope="module")
def default_cases():
    return make_gnss_loop(load_golden("gnss_front"), 6, 5)


def step(ctx, cases, f, table, in_frame, lm=None, marg=None):
    """one frame of the serial loop, written out: -> (frame results, GNSS results, landmark results or None, how the epoch was applied).
    in_frame: the epoch staged with the frame; else the two-call form behind it.  marg: per filter marg_idx instead of the loop's"""
    if marg is None:
        nominal_stage(ctx, cases, f)()
    else:
        cs = [dict(c, frames={f: dict(c["frames"][f], marg=m)}) for c, m in zip(cases, marg)]
        nominal_stage(ctx, cs, f)()
    if lm is not None:
        lm_stage_call(ctx, cases, f, lm)()
    if in_frame:
        gnss_frame_stage_call(ctx, cases, f, table)()
    ctx.frame_run()
    fr = ctx.frame_fetch()
    if not in_frame:
        gnss_stage_call(ctx, cases, f, table)()
        ctx.gnss_run()
    g = ctx.gnss_fetch()
    return fr, g, (ctx.landmark_fetch() if lm is not None else None), ctx.debug_gnss_fused_last()


def all_equal(xs, ys, what):
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert np.array_equal(x, y), (what, i)


def same_step(cases, ra, rb, what):
    """bit for bit: frame_fetch, gnss_fetch (dx over the live state: the buffers' tails belong to nobody), landmark_fetch"""
    all_equal(ra[0], rb[0], (what, "frame"))
    for b, c in enumerate(cases):
        n = c["P"].shape[0]
        assert np.array_equal(ra[1][0][b, :n], rb[1][0][b, :n]), (what, b)
    all_equal(ra[1][1:], rb[1][1:], (what, "gnss"))
    if ra[2] is not None:
        all_equal(ra[2], rb[2], (what, "landmarks"))


# ---- 1. folded, against the host reference -----------------------------------------------------------------------------------------
def test_folded_loop_equals_the_host_loop_in_the_reference_order(fold_cases):
    from ingvio_amd import capi
    cases = fold_cases
    B = len(cases)
    table = chi2()
    thr = table[1]
    ch, cd = loop_ctx(cases, F), table_ctx(cases, F, gnss=True)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    epochs = ok = 0
    for f in range(len(cases[0]["frames"])):
        (dxh, acch, rowsh), gh = host_step_gnss(ch, cases, tabs, f, table)
        (dxd, accd, rowsd), gd, _, how = step(cd, cases, f, table, in_frame=True)
        assert how == FOLDED, (f, how)                                   # the path taken was the fold
        assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd), f
        print("frame", f, "gnss rows host", gh[1].tolist(), "device", gd[1].tolist(), "status host", gh[4].tolist(), "device", gd[4].tolist())
        assert np.array_equal(gh[1], gd[1]) and np.array_equal(gh[4], gd[4]), (f, gh[1], gd[1], gh[4], gd[4])
        for b, c in enumerate(cases):
            if c["epochs"][f] is None:
                assert gd[1][b] == 0 and gd[4][b] == capi.OK and not gd[0][b].any(), (f, b)
                continue
            assert np.array_equal(gh[2][b, :2 * NS], gd[2][b, :2 * NS]), (f, b)
            # the conditions of the comparison, on the HOST loop's results: the update is exercised and no gate is a coin toss
            assert gh[1][b] >= 8, (f, b, gh[1][b])
            gam = gh[3][b, :2 * NS]
            print("  filter", b, "min |gamma - thr| / thr", float(np.abs(gam - thr).min() / thr))
            assert (np.abs(gam - thr) > 1e-6 * thr).all(), (f, b, gam)
            epochs += 1
            ok += int(gh[4][b] == capi.OK)
        nom = cd.nominal_get()
        for b in range(B):
            worst = assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph, Pd = ch.cov_get(b), cd.cov_get(b)
            assert Ph.shape == Pd.shape and rel(Pd, Ph) <= 1e-9, (f, b, rel(Pd, Ph))
    print("epochs", epochs, "ok", ok, "worst table value of the last frame", worst)
    assert epochs == 8 * 8 and ok >= 0.9 * epochs, (epochs, ok)
    ch.close(); cd.close()


# ---- 2. folded, against the device two-call form -----------------------------------------------------------------------------------
def test_folded_loop_equals_the_two_call_device_loop(fold_cases):
    cases = fold_cases
    B = len(cases)
    table = chi2()
    ca, cb = table_ctx(cases, F, gnss=True), table_ctx(cases, F, gnss=True)
    updates = 0
    for f in range(len(cases[0]["frames"])):
        fa, ga, _, how_a = step(ca, cases, f, table, in_frame=True)
        fb, gb, _, how_b = step(cb, cases, f, table, in_frame=False)
        assert (how_a, how_b) == (FOLDED, OWN_PASS), (f, how_a, how_b)
        assert np.array_equal(fa[1], fb[1]) and np.array_equal(fa[2], fb[2]), f
        assert np.array_equal(ga[1], gb[1]) and np.array_equal(ga[4], gb[4]), (f, ga[1], gb[1], ga[4], gb[4])
        assert np.array_equal(ga[2][:, :2 * NS], gb[2][:, :2 * NS]), f
        for b, c in enumerate(cases):
            # both dx live in the index space behind the frame's marginalisation (the scalars in front of the clones never move)
            n = c["P"].shape[0]
            da, db = ga[0][b, :n], gb[0][b, :n]
            if db.any():
                updates += 1
                print("frame", f, "filter", b, "gnss dx: max|diff| / max|dx|", float(np.abs(da - db).max() / np.abs(db).max()))
                assert np.abs(da - db).max() <= 1e-7 * np.abs(db).max(), (f, b)
            else:
                assert not da.any(), (f, b)
            assert not ga[0][b, n:].any(), (f, b)
        sa, sb = state(ca, B), state(cb, B)
        for b in range(B):
            for key in ("kind", "idx", "anchor", "clone_var"):
                assert np.array_equal(sa[0][b][key], sb[0][b][key]), (f, b, key)
            live = sa[0][b]["kind"] >= 0
            assert rel(sa[0][b]["val"][live], sb[0][b]["val"][live]) <= 1e-9, (f, b)
            assert rel(sa[1][b], sb[1][b]) <= 1e-9, (f, b, rel(sa[1][b], sb[1][b]))
    assert updates >= 40
    ca.close(); cb.close()


# ---- 3. not folded: bit for bit the two calls behind the frame ----------------------------------------------------------------------
def test_default_loop_cannot_fold_and_equals_the_two_call_form_bit_for_bit(default_cases):
    cases = default_cases
    B = len(cases)
    table = chi2()
    ca, cb = table_ctx(cases, F, gnss=True), table_ctx(cases, F, gnss=True)
    rows = 0
    for f in range(len(cases[0]["frames"])):
        ra, rb = step(ca, cases, f, table, in_frame=True), step(cb, cases, f, table, in_frame=False)
        assert (ra[3], rb[3]) == (OWN_PASS, OWN_PASS), f                 # scalars behind the leaving clone, 22 candidate rows
        same_step(cases, ra, rb, f)
        same_state(state(ca, B), state(cb, B), what=f)
        rows += int(ra[1][1].sum())
    assert rows >= 8 * 4 * 5                                             # real updates in the four filters with epochs
    ca.close(); cb.close()


def test_one_filter_without_marginalisation_is_not_folded(fold_cases):
    cases = fold_cases[:6]
    B = len(cases)
    table = chi2()
    ca, cb = table_ctx(cases, F, gnss=True), table_ctx(cases, F, gnss=True)
    for f in range(3):                                                   # the same two-call frames in both: features arrive in frame 2
        same_step(cases, step(ca, cases, f, table, in_frame=False), step(cb, cases, f, table, in_frame=False), f)
    marg = [c["frames"][3]["marg"] for c in cases]
    marg[1] = -1
    ra, rb = step(ca, cases, 3, table, in_frame=True, marg=marg), step(cb, cases, 3, table, in_frame=False, marg=marg)
    assert (ra[3], rb[3]) == (OWN_PASS, OWN_PASS)
    assert ra[0][2].min() > 0 and ra[1][1].sum() >= 8 * 4                # MSCKF rows in every filter, GNSS rows in those with epochs
    same_step(cases, ra, rb, "marg -1")
    sa = state(ca, B)
    same_state(sa, state(cb, B))
    assert len(sa[0][1]["clone_var"]) == len(sa[0][0]["clone_var"]) + 2  # filter 1 kept its clone (its window starts one longer)
    ca.close(); cb.close()


def test_frame_with_landmark_stage_is_not_folded():
    z = load_golden("gnss_front")
    cases = make_gnss_loop(z, 6, 5, scalars_in_front=True, n_sat=NS, cases=make_lm_loop(6, 5))
    B = len(cases)
    table, opts = chi2(), lm_opts()
    ca, cb = table_ctx(cases, F, gnss=True), table_ctx(cases, F, gnss=True)
    lm_rows = g_rows = 0
    for f in range(5):
        ra, rb = step(ca, cases, f, table, in_frame=True, lm=opts), step(cb, cases, f, table, in_frame=False, lm=opts)
        assert (ra[3], rb[3]) == (OWN_PASS, OWN_PASS), f
        same_step(cases, ra, rb, f)
        same_state(state(ca, B), state(cb, B), what=f)
        lm_rows += int(ra[2][1].sum()); g_rows += int(ra[1][1].sum())
    assert lm_rows > 0 and g_rows >= 8 * 4 * 5
    ca.close(); cb.close()


# ---- 4. pipelined = serial, snapshot = replay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("folded", "not_folded"))
def test_pipelined_in_frame_loop_equals_serial_loop(fold_cases, default_cases, which):
    cases = fold_cases[:6] if which == "folded" else default_cases
    B, NF = len(cases), 5
    table = chi2()
    res = []
    for pipelined in (False, True):
        ctx = table_ctx(cases, F, gnss=True)
        out = DeviceLoop(ctx, cases, range(NF), GnssInFrameForm(table), pipelined, sync_every_call=not pipelined).run()
        res.append((out, state(ctx, B), ctx.debug_gnss_fused_last()))
        ctx.close()
    (o0, s0, h0), (o1, s1, h1) = res
    assert h0 == h1 == (FOLDED if which == "folded" else OWN_PASS)
    for f, ((fr0, g0), (fr1, g1)) in enumerate(zip(o0, o1)):
        # gnss_fetch(f) was issued after both stages of frame f + 1, frame_fetch_end(f) after run(f + 1): still frame f's results
        same_step(cases, (fr0, g0, None), (fr1, g1, None), f)
    assert sum(int(g[1].sum()) for _, g in o1) >= 8 * 4 * NF
    same_state(s0, s1)


def test_snapshot_restore_replays_the_in_frame_loop_bit_for_bit(fold_cases):
    cases = fold_cases[:6]
    B = len(cases)
    table = chi2()
    ctx = table_ctx(cases, F, gnss=True)
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            ctx.restore()
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        out = DeviceLoop(ctx, cases, range(4), GnssInFrameForm(table), pipelined=False).run()
        runs.append((out, state(ctx, B)))
    (o0, s0), (o1, s1) = runs
    for f, ((fr0, g0), (fr1, g1)) in enumerate(zip(o0, o1)):
        # (dx and rows, as tests/test_gpu_nominal_gnss.py compares a replay: frames 0 and 1 stage no feature, and the accept words of a
        # frame without features are those of whatever frame ran before it)
        same_step(cases, ((fr0[0], fr0[2]), g0, None), ((fr1[0], fr1[2]), g1, None), f)
    same_state(s0, s1)
    assert ctx.debug_gnss_fused_last() == FOLDED
    ctx.close()


# ---- 5. the trailing retraction kernel alone ----------------------------------------------------------------------------------------
def test_retraction_behind_the_marginalisation_matches_the_host_table():
    """k_nominal_update_post on the table alone: dx given in the index space behind the marginalisation; every kind of variable, a free
    slot, landmarks anchored below and ABOVE the clone that leaves, angles from 1e-12 to 3 rad"""
    from ingvio_amd import capi
    rng = np.random.default_rng(83)
    B = 2
    tabs = [random_table(rng, n_clones=4, n_lm=5 + b) for b in range(B)]
    margs, posts = [], []
    for t, n in tabs:
        for s in t.slots:                                                # nothing may hang on the clone that leaves: up to the last clone
            if s is not None and s["kind"] == LM and s["anchor"] == t.clones[1]:
                s["anchor"] = t.clones[3]
        m = t.slots[t.clones[1]]["idx"]
        assert any(s is not None and s["kind"] == LM and t.slots[s["anchor"]]["idx"] > m for s in t.slots) and None in t.slots
        margs.append(m)
    n_max = max(n for _, n in tabs)
    ctx = capi.Context(batch=B, n_max=((n_max + 15) // 16) * 16, c_max=8, f_max=16, m_max=64)
    ctx.nominal_create(32)
    ctx.nominal_set(0, [t.as_dict() for t, _ in tabs])
    for (t, n), m in zip(tabs, margs):
        pre = random_dx(rng, t, ctx.ldp)                                 # in the table's index space, the leaving clone's entries unused
        posts.append(np.r_[np.delete(pre, range(m, m + 6)), np.zeros(6)])
        pre[m:m + 6] = 0.0
        t.box_plus(pre)
        t.marginalize(m)
    ctx.debug_nominal_update_post(0, np.stack(posts), margs)
    got = ctx.nominal_get()
    for b, (t, _) in enumerate(tabs):
        print("filter", b, "worst relative error of a value", assert_table(got[b], t, 1e-13, b))
    with pytest.raises(capi.IngvioError) as e:                           # the idx that left names no clone any more
        ctx.debug_nominal_update_post(0, np.stack(posts), [margs[0] + 1, margs[1]])
    assert e.value.code == capi.E_NOT_IN_STATE
    ctx.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_table_covariance_and_results_unchanged(fold_cases):
    from ingvio_amd import capi
    cases = fold_cases[:4]                                               # filter 2 has no epochs
    B = len(cases)
    table = chi2()
    slots = [c["gnss_slots"] for c in cases]
    tabs = [c["table"].as_dict() for c in cases]
    stage = lambda ctx, f=0: gnss_frame_stage_call(ctx, cases, f, table)

    ctx = loop_ctx(cases, F)
    with pytest.raises(capi.IngvioError) as e:
        stage(ctx)()                                                     # no table
    assert e.value.code == capi.E_ARG
    ctx.nominal_create(48)
    ctx.nominal_set(0, tabs)
    refused(ctx, stage(ctx), capi.E_ARG)                                 # no frame staged from the table
    ctx.snapshot()

    def fresh_frame(gnss=slots, table_0=None):
        """back to the start with the frame of index 0 staged from the table"""
        ctx.restore()
        ctx.tracks_create(F)
        if table_0 is not None:
            ctx.nominal_set(0, [table_0])
        if gnss is not None:
            ctx.nominal_set_gnss(0, gnss)
        nominal_stage(ctx, cases, 0)()

    fresh_frame(gnss=None)
    refused(ctx, stage(ctx), capi.E_ARG)                                 # no registered scalars, n_sat > 0
    for miss in (4, 5):                                                  # FS, YOF not in the table
        fresh_frame([[-1 if s == miss else v for s, v in enumerate(slots[0])]] + slots[1:])
        refused(ctx, stage(ctx), capi.E_NOT_IN_STATE)
    # a column outside the state the update sees / on the clone that leaves (a table whose integers do not fit the covariance)
    n0, marg0 = cases[0]["P"].shape[0], cases[0]["frames"][0]["marg"]
    for bad in (n0 + 6, marg0 + 2):
        t0 = copy.deepcopy(tabs[0])
        t0["idx"][slots[0][4]] = bad
        fresh_frame(table_0=t0)
        refused(ctx, stage(ctx), capi.E_NOT_IN_STATE)
    fresh_frame(table_0=tabs[0])
    eps = [c["epochs"][0] for c in cases]
    refused(ctx, ctx.gnss_frame_stage_nominal_prepare(0, eps[:B - 1], table, strong_reject=True), capi.E_ARG)      # not the whole batch
    refused(ctx, ctx.gnss_frame_stage_nominal_prepare(1, eps[1:], table, strong_reject=True), capi.E_ARG)
    mld = ctx.L.ingvio_mld(ctx.h)
    n_over = mld // 2 + 1
    assert n_over <= 64
    for n_sat, code in ((65, capi.E_ARG), (n_over, capi.E_CAPACITY)):    # the checks of the host-fed front, with its codes
        big = dict(eps[0], eph=np.tile(eps[0]["eph"], (9, 1))[:n_sat], obs=np.tile(eps[0]["obs"], (9, 1))[:n_sat])
        refused(ctx, ctx.gnss_frame_stage_nominal_prepare(0, [big] + eps[1:], table, strong_reject=True), code)
    # the refusals that stay as they were
    refused(ctx, ctx.gnss_front_stage_nominal_prepare(0, eps, table, in_frame=True), capi.E_UNSUPPORTED)
    refused(ctx, gnss_stage_call(ctx, cases, 0, table), capi.E_ARG)      # the two-call stage with a frame pending
    # staged: a second stage and ingvio_gnss_run are refused, the frame applies the epoch once
    stage(ctx)()
    refused(ctx, stage(ctx), capi.E_ARG)
    refused(ctx, lambda: ctx.gnss_run(0, B), capi.E_ARG)
    ctx.frame_run()
    fr0, g0 = ctx.frame_fetch(), ctx.gnss_fetch()
    assert ctx.debug_gnss_fused_last() == FOLDED
    refused(ctx, lambda: ctx.gnss_run(0, B), capi.E_ARG)                 # consumed
    refused(ctx, stage(ctx, 1), capi.E_ARG)                              # frame 1 is not staged yet
    all_equal(g0, ctx.gnss_fetch(), "results stay")
    # a restore abandons the stage with its frame
    ctx.snapshot()
    s0 = state(ctx, B)
    nominal_stage(ctx, cases, 1)()
    stage(ctx, 1)()
    ctx.restore()
    same_state(s0, state(ctx, B))
    refused(ctx, lambda: ctx.frame_run(), capi.E_ARG)
    refused(ctx, lambda: ctx.gnss_run(0, B), capi.E_ARG)
    ctx.close()


def test_frame_after_a_frame_with_the_stage_takes_the_plain_path(fold_cases):
    """the stage is consumed by its frame: the next frame without one runs as a frame whose epochs are all empty, bit for bit, and
    leaves the GNSS results of the frame before alone"""
    cases = fold_cases[:6]
    B = len(cases)
    table = chi2()
    res = []
    for empty_stage in (False, True):
        ctx = table_ctx(cases, F, gnss=True)
        for f in range(3):
            _, g2, _, how = step(ctx, cases, f, table, in_frame=True)
        assert how == FOLDED
        nominal_stage(ctx, cases, 3)()
        if empty_stage:
            ctx.gnss_frame_stage_nominal(0, [None] * B, table, gate_rows=True, strong_reject=True)
        ctx.frame_run()
        fr, g3 = ctx.frame_fetch(), ctx.gnss_fetch()
        if empty_stage:
            assert not g3[0].any() and not g3[1].any() and not g3[4].any() and ctx.debug_gnss_fused_last() == OWN_PASS
        else:
            all_equal(g2, g3, "frame 2's GNSS results")
        res.append((fr, state(ctx, B)))
        ctx.close()
    all_equal(res[0][0], res[1][0], "frame 3")
    same_state(res[0][1], res[1][1])


def test_two_call_loop_is_the_same_before_and_after_the_context_has_seen_the_new_stage(fold_cases):
    """a context that does not call the new export runs what it ran before: the two-call loop on a fresh context and on one that ran
    in-frame epochs and was restored give the same bits"""
    cases = fold_cases[:6]
    B = len(cases)
    table = chi2()
    fresh = table_ctx(cases, F, gnss=True)
    ref = DeviceLoop(fresh, cases, range(4), GnssForm(table), pipelined=True).run()
    s_ref = state(fresh, B)
    fresh.close()
    ctx = table_ctx(cases, F, gnss=True)
    ctx.snapshot()
    for f in range(3):
        step(ctx, cases, f, table, in_frame=True)
    ctx.restore()
    ctx.tracks_create(F)
    out = DeviceLoop(ctx, cases, range(4), GnssForm(table), pipelined=True).run()
    for f, ((fr0, g0), (fr1, g1)) in enumerate(zip(ref, out)):
        # (dx and rows: the two contexts have different histories, see the replay test)
        same_step(cases, ((fr0[0], fr0[2]), g0, None), ((fr1[0], fr1[2]), g1, None), f)
    same_state(s_ref, state(ctx, B))
    ctx.close()
