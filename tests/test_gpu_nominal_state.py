"""Device-resident nominal state (include/ingvio_hip.h: ingvio_nominal_*, ingvio_frame_stage_tracks_nominal).

The context holds every filter's typed nominal values (StateManager's _err_var list: extended pose, biases, extrinsics, clones, clock
scalars, anchored landmarks) and closes the filter loop on the device: boxPlus with the frame's dx, the marginalised clone's drop and
index shift, the IMU nominal integration and the new clone's pose.  Checked against the C oracle's retractions and against a host loop
that keeps the same values with the oracle's functions and the Var semantics of oracle/stream_filter.py."""
import numpy as np
import pytest

from conftest import rel_err as rel
from ingvio_amd.closed_loop import (LM, SCALAR, SE23, SE3, SIZE, VEC3, HostTable, device_loop, host_step, loop_ctx, make_loop,
                                     nominal_stage, stage_args)
from nominal_helpers import TABLE_KEYS, assert_table, device_state, same_state, table_ctx
from nominal_helpers import refused as refused_on

pytestmark = pytest.mark.gpu


def rot_block(rng, lo=-12.0, hi=np.log10(3.0)):
    ax = rng.normal(size=3)
    return ax / np.linalg.norm(ax) * 10.0 ** rng.uniform(lo, hi)


def random_rot(rng):
    from oracle import oracle as orc
    return orc.gamma(rot_block(rng, -1, np.log10(3.0)), 0)


# ---- 1. the retraction kernel against the C oracle ----------------------------------------------------------------------------
def random_table(rng, n_clones=4, n_scalar=3, n_lm=5, hole=True):
    """SE23 pose, two Vec3 biases, SE3 extrinsics, scalars, clones, landmarks anchored to different clones; one free slot"""
    slots = []
    idx = 0

    def add(kind, anchor=-1):
        nonlocal idx
        s = dict(kind=kind, idx=idx, anchor=anchor, R=random_rot(rng) if kind in (SE23, SE3) else np.eye(3) * 0.0,
                 p=rng.normal(size=3) * (5.0 if kind == LM else 1.0), v=rng.normal(size=3) if kind == SE23 else np.zeros(3))
        if kind == SCALAR:
            s["p"] = np.array([rng.normal(), 0.0, 0.0])
        idx += SIZE[kind]
        slots.append(s)
        return len(slots) - 1
    v_pose, v_bg, v_ba, v_ext = add(SE23), add(VEC3), add(VEC3), add(SE3)
    for _ in range(n_scalar):
        add(SCALAR)
    clones = [add(SE3) for _ in range(n_clones)]
    if hole:
        slots.append(None)
    for j in range(n_lm):
        add(LM, anchor=clones[j % n_clones])
    return HostTable(slots, clones, v_ext, v_pose, v_bg, v_ba, [0.0, 0.0, -9.8]), idx


def random_dx(rng, table, ld):
    dx = np.zeros(ld)
    for s in table.slots:
        if s is None:
            continue
        i, k = s["idx"], s["kind"]
        dx[i:i + SIZE[k]] = rng.normal(size=SIZE[k]) * 0.3
        if k in (SE23, SE3):
            dx[i:i + 3] = rot_block(rng)
    return dx


def test_box_plus_matches_the_oracle_retractions():
    from ingvio_amd import capi
    rng = np.random.default_rng(71)
    B = 6
    tabs = [random_table(rng, n_clones=3 + b % 3, n_lm=2 + b) for b in range(B)]
    n_max = max(n for _, n in tabs)
    ctx = capi.Context(batch=B, n_max=((n_max + 15) // 16) * 16, c_max=8, f_max=16, m_max=64)
    with pytest.raises(capi.IngvioError) as e:                           # nothing to retract yet
        ctx.nominal_box_plus(0, np.zeros((B, ctx.ldp)))
    assert e.value.code == capi.E_ARG
    ctx.nominal_create(32)
    ctx.nominal_set(0, [t.as_dict() for t, _ in tabs])
    for rep in range(3):
        dx = np.stack([random_dx(rng, t, ctx.ldp) for t, _ in tabs])
        ctx.nominal_box_plus(0, dx)
        for (t, _), d in zip(tabs, dx):
            t.box_plus(d)
        got = ctx.nominal_get()
        for b, (t, _) in enumerate(tabs):
            assert_table(got[b], t, 1e-13, (rep, b))
    # a partial range leaves the other filters alone
    dx = np.stack([random_dx(rng, t, ctx.ldp) for t, _ in tabs[2:4]])
    before = ctx.nominal_get()
    ctx.nominal_box_plus(2, dx)
    for (t, _), d in zip(tabs[2:4], dx):
        t.box_plus(d)
    got = ctx.nominal_get()
    for b in range(B):
        if 2 <= b < 4:
            assert_table(got[b], tabs[b][0], 1e-13, b)
        else:
            assert np.array_equal(got[b]["val"], before[b]["val"])
    ctx.close()


# ---- 2.-4. the closed loop -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_cases():
    return make_loop(24, 13)


def test_closed_loop_device_equals_host(loop_cases):
    import copy
    cases = loop_cases
    B, F = len(cases), 24
    ch, cd = loop_ctx(cases, F), table_ctx(cases, F)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    accepted = 0
    for f in range(len(cases[0]["frames"])):
        dxh, acch, rowsh = host_step(ch, cases, tabs, f)
        nominal_stage(cd, cases, f)()
        cd.frame_run()
        dxd, accd, rowsd = cd.frame_fetch()
        assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd), f
        accepted += int(rowsd.sum())
        # the frame's dx is written in the update's index space (orc_frame_update: n + 6 entries): the new clone's columns at the
        # pre-update N carry its correction, nothing lies beyond them; the post-frame boxPlus runs before the drop and shift
        for b, c in enumerate(cases):
            if rowsd[b] > 0:
                ni = c["frames"][f]["new_idx"]
                assert np.any(dxd[b, ni:ni + 6] != 0.0) and not np.any(dxd[b, ni + 6:]), (f, b)
        nom, Ps = device_state(cd, B)
        for b in range(B):
            assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape and rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
    assert accepted > 0                                                  # the loop carried real updates
    ch.close(); cd.close()


def test_pipelined_loop_equals_serial_loop(loop_cases):
    cases = loop_cases
    B, F = len(cases), 24
    res = []
    for pipelined in (False, True):
        ctx = table_ctx(cases, F)
        out = device_loop(ctx, cases, list(range(len(cases[0]["frames"]))), pipelined)
        res.append((out, device_state(ctx, B)))
        ctx.close()
    (o0, s0), (o1, s1) = res
    for f, (a, b) in enumerate(zip(o0, o1)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), f
    same_state(s0, s1)


def test_snapshot_restore_replays_bit_for_bit(loop_cases):
    cases = loop_cases
    B, F, N = len(cases), 24, 6
    ctx = table_ctx(cases, F)
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            ctx.restore()
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        out = device_loop(ctx, cases, list(range(N)), False)
        runs.append((out, device_state(ctx, B)))
    (o0, s0), (o1, s1) = runs
    for f, (a, b) in enumerate(zip(o0, o1)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), f
        for i, c in enumerate(cases):                                    # accept flags exist for the frame's features only
            nf = len(c["frames"][f]["delta"]["feat_track"])
            assert np.array_equal(a[1][i, :nf], b[1][i, :nf]), (f, i)
    same_state(s0, s1, keys=("kind", "idx", "val", "clone_var"))
    ctx.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_unchanged(loop_cases):
    from ingvio_amd import capi
    cases = loop_cases[:4]
    B, F = len(cases), 24
    ctx = loop_ctx(cases, F)
    with pytest.raises(capi.IngvioError) as e:
        ctx.v_max = 8
        ctx.nominal_get()
    assert e.value.code == capi.E_ARG
    ctx.nominal_create(48)
    tabs = [c["table"].as_dict() for c in cases]
    ctx.nominal_set(0, tabs)

    def refused(fn, code):
        refused_on(ctx, fn, code)

    # a landmark anchored to the clone that leaves: marginalise the FIRST clone (the landmarks' anchor)
    def bad_marg(idx_of):
        opts_frame, sigma, eg, scb, srw = stage_args(cases)
        steps = [dict(imu=c["frames"][0]["imu"], gnss_idx=c["step"]["gnss_idx"], marg_idx=idx_of(c)) for c in cases]
        return ctx.frame_stage_tracks_nominal_prepare(0, steps, [c["frames"][0]["delta"] for c in cases], opts_frame, sigma, eg, scb, srw)
    refused(bad_marg(lambda c: c["table"].slots[c["table"].clones[0]]["idx"]), capi.E_ARG)
    refused(bad_marg(lambda c: 3), capi.E_NOT_IN_STATE)                 # not a clone of the window
    ctx.set_frame_parts(2)
    refused(nominal_stage(ctx, cases, 0), capi.E_UNSUPPORTED)
    ctx.set_frame_parts(1)
    # an in-frame GNSS stage
    blk = ([0], [9], np.eye(1, 9), np.zeros(1), np.ones(1))
    ctx.gnss_stage(0, [blk] * B, cases[0]["frame"]["chi2_table"], in_frame=True)
    refused(nominal_stage(ctx, cases, 0), capi.E_UNSUPPORTED)
    ctx.close()
    # with a frame staged from the table and not yet run
    ctx = table_ctx(cases, F)
    nominal_stage(ctx, cases, 0)()
    refused(nominal_stage(ctx, cases, 1), capi.E_ARG)                    # a second stage
    refused(lambda: ctx.frame_stage(0, [c["step"] for c in cases], [c["frame"] for c in cases], cases[0]["step"]["sigma"], 1, 0.2, 0.2),
            capi.E_ARG)                                                   # the flattened stage
    refused(lambda: ctx.frame_run_phase(1), capi.E_UNSUPPORTED)           # the split step
    refused(lambda: ctx.frame_run(restore_prior=True), capi.E_ARG)
    refused(lambda: ctx.nominal_box_plus(0, np.zeros((B, ctx.ldp))), capi.E_ARG)
    refused(lambda: ctx.nominal_set(0, tabs), capi.E_ARG)
    ctx.set_frame_parts(2)
    refused(lambda: ctx.frame_run(), capi.E_UNSUPPORTED)
    ctx.set_frame_parts(1)
    ctx.frame_run()                                                       # the staged frame still runs, once
    ctx.frame_fetch()
    refused(lambda: ctx.frame_run(), capi.E_ARG)

    # a flattened frame after it runs as without the table, and leaves the table alone
    def flattened():
        ctx.frame_stage(0, [c["step"] for c in cases], [c["frame"] for c in cases], cases[0]["step"]["sigma"], 1, 0.2, 0.2)
        ctx.frame_run()
        return ctx.frame_fetch()
    t0 = ctx.nominal_get()
    flattened()
    t1 = ctx.nominal_get()
    for b in range(B):
        for key in TABLE_KEYS:
            assert np.array_equal(t0[b][key], t1[b][key]), (b, key)
    ctx.close()

    # a stage from the table is a whole-batch stage: the post-frame step covers every filter
    ctx = table_ctx(cases, F)
    opts_frame, sigma, eg, scb, srw = stage_args(cases)
    steps = [dict(imu=c["frames"][0]["imu"], gnss_idx=c["step"]["gnss_idx"], marg_idx=c["frames"][0]["marg"]) for c in cases]
    deltas = [c["frames"][0]["delta"] for c in cases]
    for b0, nb in ((0, B - 1), (1, B - 1), (2, 1)):
        refused(ctx.frame_stage_tracks_nominal_prepare(b0, steps[b0:b0 + nb], deltas[b0:b0 + nb], opts_frame, sigma, eg, scb, srw), capi.E_ARG)
    # a restore abandons a staged frame; a flattened frame runs after it
    ctx.snapshot()
    s0 = device_state(ctx, B)
    nominal_stage(ctx, cases, 0)()
    ctx.restore()
    same_state(s0, device_state(ctx, B))
    flattened()
    ctx.close()

    # a snapshot taken before the table exists holds none: restoring it would leave covariance and table disagreeing
    ctx = loop_ctx(cases, F)
    ctx.snapshot()
    ctx.nominal_create(48)
    ctx.nominal_set(0, tabs)
    refused(lambda: ctx.restore(), capi.E_ARG)
    ctx.close()
