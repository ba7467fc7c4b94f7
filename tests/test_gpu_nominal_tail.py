"""The landmark tail of a frame on the device (include/ingvio_hip.h: ingvio_nominal_tail): changeLandmarkAnchor
(LandmarkUpdate.cpp:273-361), margSwPose and the erase of lost landmarks (StateManager.cpp:340-353) for a range of filters in one
sweep over P, from what the device holds.

Against the C oracle applied in the reference's order (closed_loop_tail.sequential_tail: replace_var_linear landmark by landmark, then
marginalize variable by variable); the joint form equals it up to rounding (tests/test_nominal_tail_model.py), so P is compared at
the project's FP64 parity bound, 1e-11 of max|P|, and every integer exactly.  The closed loop runs a real window policy - the
oldest clone leaves every frame, or two clones every other frame - against the host reference loop of closed_loop_tail.py at the
closed-loop bound of test_gpu_nominal_landmarks.py, 1e-9."""
import copy

import numpy as np
import pytest

from conftest import rel_err as rel
from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_lm as clm
from ingvio_amd import closed_loop_tail as clt
from nominal_helpers import assert_table, device_state, same_state
from nominal_helpers import refused as refused_on

pytestmark = pytest.mark.gpu

F_LOOP, L_LOOP = 24, 6


# ---- 1. - 3. one call on a batch of mixed filters --------------------------------------------------------------------------------
def mixed_batch():
    """six filters in one call: 0 / 1 / 2 / 5 anchor changes (filters 2 and 3 with a landmark behind the new anchor), 0 - 2 erases,
    0 / 1 / 2 non-adjacent clones leaving, GNSS scalars behind the start window's clones in two; filter 5 has empty lists"""
    S = clt.synthetic_case
    flt = [S(3, 0, 11, marg_pos=(0,)),
           S(6, 1, 12, gnss=True, marg_pos=(0,)),
           S(11, 3, 13, marg_pos=(0, 2), behind=(2,), erase=(1,)),
           S(12, 8, 14, gnss=True, marg_pos=(0, 2), behind=(5,), erase=(1,), hole=True),
           S(6, 3, 15, marg_pos=(), erase=(0, 2)),
           S(6, 2, 16, marg_pos=())]
    assert [len(f["plan"]["lm_slot"]) for f in flt] == [0, 1, 2, 5, 0, 0]
    assert [len(f["plan"]["erase_slot"]) for f in flt] == [0, 0, 1, 1, 2, 0]
    assert [len(f["plan"]["marg_slot"]) for f in flt] == [1, 1, 2, 2, 0, 0]
    assert clt.plan_is_empty(flt[5]["plan"]) and not clt.plan_is_empty(flt[4]["plan"])
    return flt


def batch_ctx(flt, table=True):
    from ingvio_amd import capi
    n_max = max(f["P"].shape[0] for f in flt)
    ctx = capi.Context(batch=len(flt), n_max=((n_max + 15) // 16) * 16, c_max=12, f_max=8, m_max=64)
    for b, f in enumerate(flt):
        ctx.cov_set(b, f["P"])
    if table:
        ctx.nominal_create(48)
        ctx.nominal_set(0, [f["table"].as_dict() for f in flt])
        ctx.nominal_set_gnss(0, [f["gnss_slots"] for f in flt])
    return ctx


def full_state(ctx):
    B = ctx.batch
    return device_state(ctx, B), [ctx.n(b) for b in range(B)], ctx.nominal_get_gnss()


def same_full(s0, s1, only=None):
    for b in (range(len(s0[1])) if only is None else only):
        for key in ("kind", "idx", "anchor", "val", "clone_var"):
            assert np.array_equal(s0[0][0][b][key], s1[0][0][b][key]), (b, key)
        assert np.array_equal(s0[0][1][b], s1[0][1][b]) and s0[1][b] == s1[1][b], b
    assert np.array_equal(s0[2], s1[2])


def oracle_tail(f):
    """-> (P, table, verdicts, depths) of the sequential oracle on filter f"""
    from oracle import oracle as orc
    cov, t = orc.Cov(f["P"]), copy.deepcopy(f["table"])
    v, z = clt.sequential_tail(cov, t, f["plan"])
    return cov.P, t, v, z


def check_against_oracle(ctx, b, f, verdict):
    Po, to, vo, depth = oracle_tail(f)
    assert all(abs(z) >= 0.1 for z in depth), depth
    assert [int(x) for x in verdict[:len(vo)]] == vo and not verdict[len(vo):].any(), (b, verdict, vo)
    Pd = ctx.cov_get(b)
    assert ctx.n(b) == Po.shape[0] == Pd.shape[0], b
    err = float(np.max(np.abs(Pd - Po)) / np.max(np.abs(Po)))
    print("filter %d  n %3d -> %3d  verdicts %s  max|dP| / max|P| %.3e" % (b, f["P"].shape[0], Po.shape[0], vo, err))
    assert err <= 1e-11, (b, err)
    assert np.array_equal(Pd, Pd.T), b
    dev = ctx.nominal_get(b, 1)[0]
    assert assert_table(dev, to, 0.0, b) == 0.0                          # integers exact, surviving values bit for bit
    assert np.array_equal(ctx.nominal_get_gnss(b, 1)[0], f["gnss_slots"])
    return vo


def test_one_call_on_mixed_filters_against_the_sequential_oracle():
    flt = mixed_batch()
    ctx = batch_ctx(flt)
    s0 = full_state(ctx)
    verdict, status = ctx.nominal_tail(0, [f["plan"] for f in flt])
    assert not status.any()
    seen = []
    for b, f in enumerate(flt):
        seen += check_against_oracle(ctx, b, f, verdict[b])
    assert seen.count(0) == 2 and seen.count(1) == 6
    same_full(s0, full_state(ctx), only=[5])                             # empty lists: untouched bit for bit while the neighbours changed
    assert all(ctx.n(b) < s0[1][b] for b in range(5))
    # an all-empty call changes nothing anywhere
    s1 = full_state(ctx)
    v, _ = ctx.nominal_tail(0, [dict() for _ in flt])
    assert not v.any()
    same_full(s1, full_state(ctx))
    ctx.close()


def test_partial_range_leaves_the_other_filters_alone():
    flt = mixed_batch()
    ca, cb = batch_ctx(flt), batch_ctx(flt)
    s0 = full_state(cb)
    va, _ = ca.nominal_tail(0, [f["plan"] for f in flt])
    vb, _ = cb.nominal_tail(1, [f["plan"] for f in flt[1:4]])
    sa, sb = full_state(ca), full_state(cb)
    same_full(s0, sb, only=[0, 4, 5])
    same_full(sa, sb, only=[1, 2, 3])                                    # the same arithmetic in either range
    assert np.array_equal(va[1:4], vb)
    # the rest of the batch afterwards: the mirror of the skipped filters was left as it was
    cb.nominal_tail(0, [flt[0]["plan"]])
    cb.nominal_tail(4, [flt[4]["plan"], dict()])
    same_full(sa, full_state(cb))
    ca.close(); cb.close()


def test_refusals_leave_the_state_unchanged():
    from ingvio_amd import capi
    flt = mixed_batch()
    plans = [f["plan"] for f in flt]
    ctx = batch_ctx(flt, table=False)
    with pytest.raises(capi.IngvioError) as e:
        ctx.nominal_tail(0, plans)                                       # no table
    assert e.value.code == capi.E_ARG
    ctx.close()
    ctx = batch_ctx(flt)

    def with_plan(b, **kw):
        return [dict(p, **kw) if i == b else p for i, p in enumerate(plans)]

    def refused(pl, code, b0=0, lm_cap=None):
        refused_on(ctx, lambda: ctx.nominal_tail(b0, pl, lm_cap=lm_cap), code, sizes=True)
    t3, p3 = flt[3]["table"], plans[3]
    lm3, other_lm = p3["lm_slot"], [sl for sl in flt[3]["lm_slots"] if sl not in p3["lm_slot"] + p3["erase_slot"]]
    stay = [c for c in t3.clones[:-1] if c not in p3["marg_slot"]]
    # INGVIO_E_ARG
    refused(plans[:3], capi.E_ARG, b0=4)                                 # a range outside the batch
    refused(plans, capi.E_ARG, lm_cap=4)                                 # n_reanchor > lm_cap
    refused(with_plan(3, lm_slot=lm3 * 13), capi.E_ARG)                  # n_reanchor = 65 > 64
    refused(with_plan(3, lm_slot=lm3[:2] + lm3[:1]), capi.E_ARG)         # a slot named twice
    refused(with_plan(3, erase_slot=p3["erase_slot"] + lm3[:1]), capi.E_ARG)      # ... in both landmark lists
    refused(with_plan(3, marg_slot=p3["marg_slot"] + p3["marg_slot"][:1]), capi.E_ARG)
    refused(with_plan(3, marg_slot=p3["marg_slot"] + [p3["new_anchor"]]), capi.E_ARG)      # new_anchor leaves
    refused(with_plan(3, new_anchor=p3["marg_slot"][0], marg_slot=p3["marg_slot"][1:]), capi.E_ARG)      # already anchored to new_anchor
    refused(with_plan(3, lm_slot=lm3[:-1]), capi.E_ARG)                  # a survivor stays anchored to a clone that leaves
    refused(with_plan(3, marg_slot=p3["marg_slot"] + [t3.slots[other_lm[0]]["anchor"]]), capi.E_ARG)      # ... in neither list
    L = ctx.L
    assert L.ingvio_nominal_tail(ctx.h, 0, ctx.batch, None, 8, None, None) == capi.E_ARG      # NULL where data is needed
    arr = (capi.NominalTailBlock * ctx.batch)()
    arr[3].n_reanchor = 2
    assert L.ingvio_nominal_tail(ctx.h, 0, ctx.batch, arr, 8, capi._i(np.zeros((6, 8), dtype=np.int32)), None) == capi.E_ARG
    # INGVIO_E_NOT_IN_STATE
    refused(with_plan(3, lm_slot=lm3[:-1] + [47]), capi.E_NOT_IN_STATE)  # a free slot
    refused(with_plan(3, erase_slot=[t3.v_bg]), capi.E_NOT_IN_STATE)     # not a landmark
    refused(with_plan(3, marg_slot=[t3.v_ext]), capi.E_NOT_IN_STATE)     # an SE3 that is no window clone
    refused(with_plan(3, marg_slot=[lm3[0]]), capi.E_NOT_IN_STATE)
    refused(with_plan(3, new_anchor=t3.v_ext), capi.E_NOT_IN_STATE)
    refused(with_plan(3, new_anchor=40), capi.E_NOT_IN_STATE)
    assert stay
    # fewer than two window clones with an anchor change: a table of its own
    one = clt.synthetic_case(3, 1, 31, marg_pos=(0,))
    t1 = copy.deepcopy(one["table"])
    lone = t1.clones[0]
    t1.clones = [lone]
    ctx.nominal_set(0, [t1.as_dict()])
    ctx.cov_set(0, one["P"])
    refused([dict(lm_slot=one["plan"]["lm_slot"], new_anchor=lone)], capi.E_ARG)
    refused([dict(lm_slot=one["plan"]["lm_slot"], new_anchor=one["plan"]["new_anchor"])], capi.E_NOT_IN_STATE)
    ctx.nominal_set(0, [flt[0]["table"].as_dict()])
    ctx.cov_set(0, flt[0]["P"])
    # after all of it the valid call runs and gives what it gives on a fresh context
    verdict, _ = ctx.nominal_tail(0, plans)
    for b, f in enumerate(flt):
        check_against_oracle(ctx, b, f, verdict[b])
    ctx.close()


@pytest.mark.parametrize("what", ["frame", "gnss", "landmarks", "split"])
def test_refused_while_other_work_is_pending(what):
    """a frame, a GNSS epoch or a stand-alone landmark update staged from the table that has not run, a split frame step between its
    halves: INGVIO_E_ARG with the state unchanged; once the work has run the tail is accepted"""
    from conftest import load_golden
    from ingvio_amd import capi, host, synth
    from nominal_helpers import table_ctx
    if what == "split":
        ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
        cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
        ctx.tracks_create(32); ctx.nominal_create(16)
        ctx.snapshot()
        ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
        ctx.frame_run_phase(1, restore_prior=True)
        before = [(ctx.n(b), ctx.cov_get(b)) for b in range(2)]
        with pytest.raises(capi.IngvioError) as e:
            ctx.nominal_tail(0, [dict(marg_slot=[0]), dict()])
        assert e.value.code == capi.E_ARG and "split" in str(e.value)
        for b in range(2):
            assert ctx.n(b) == before[b][0] and np.array_equal(ctx.cov_get(b), before[b][1])
        ctx.frame_run_phase(2)
        ctx.frame_fetch()
        ctx.close()
        return
    if what == "gnss":
        from ingvio_amd.closed_loop_gnss import gnss_stage_call, make_gnss_loop
        cases = make_gnss_loop(load_golden("gnss_front"), 2, 2, every=0)
        ctx = table_ctx(cases, gnss=True)
        gnss_stage_call(ctx, cases, 0, synth.chi2_table())()
    else:
        cases, o = clm.make_lm_loop(2, 2), clm.lm_opts()
        ctx = table_ctx(cases)
        if what == "frame":
            cl.nominal_stage(ctx, cases, 0)()
        else:
            ctx.landmark_stage_nominal_prepare(0, clm.nominal_frames(cases, 0), o["stereo"], o["noise"], o["chi2_thr"], o["R_cl2cr"], o["t_cl2cr"],
                                               in_frame=False)()
    second = [int(c["table"].clones[1]) for c in cases]                  # no landmark of these loops hangs on the second clone
    plans = [dict(marg_slot=[s]) for s in second]
    refused_on(ctx, lambda: ctx.nominal_tail(0, plans), capi.E_ARG, sizes=True)
    if what == "gnss":
        ctx.gnss_run(); ctx.gnss_fetch()
    elif what == "frame":
        ctx.frame_run(); ctx.frame_fetch()
    else:
        ctx.landmark_run(); ctx.landmark_fetch()
    n0 = [ctx.n(b) for b in range(2)]
    plans = [dict(marg_slot=[int(t["clone_var"][1])]) for t in ctx.nominal_get()]      # (the frame has dropped the clone named above)
    ctx.nominal_tail(0, plans)
    assert [ctx.n(b) for b in range(2)] == [n - 6 for n in n0]
    ctx.close()


# ---- 4. / 5. the closed loop -------------------------------------------------------------------------------------------------------
def loop_ctx(cases, table, c_max):
    from ingvio_amd import capi
    n_max = max(c["P"].shape[0] for c in cases) + 12                    # mode "kf": two clones arrive before two leave
    ctx = capi.Context(batch=len(cases), n_max=((n_max + 15) // 16) * 16, c_max=c_max, f_max=F_LOOP, m_max=64)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c["P"])
    ctx.tracks_create(F_LOOP)
    if table:
        ctx.nominal_create(48)
        ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    return ctx


@pytest.fixture(scope="module")
def sw_cases():
    return clt.make_tail_loop(8, 12, L=L_LOOP, F=F_LOOP, mode="sw")


@pytest.fixture(scope="module")
def kf_cases():
    return clt.make_tail_loop(8, 6, L=L_LOOP, F=F_LOOP, mode="kf")


def closed_loop(cases, c_max):
    """8 filters, windows 5 ... 11, 6 landmarks with the in-frame landmark stage, the device loop frame by frame against the host
    reference loop"""
    opts = clm.lm_opts()
    B, n_frames = len(cases), len(cases[0]["frames"])
    assert sorted({c["C"] for c in cases}) == list(range(5, 12))
    ch, cd = loop_ctx(cases, False, c_max), loop_ctx(cases, True, c_max)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    alive = [list(range(L_LOOP)) for _ in cases]
    form = clt.TailForm(opts, cases)
    loop = cl.DeviceLoop(cd, cases, range(n_frames), form, pipelined=False)
    loop.start()
    worst_t = worst_p = 0.0
    n_behind = n_moved = n_erased = lm_rows = 0
    for f in range(n_frames):
        (dxh, acch, rowsh), (ldxh, lrowsh, lacch, lgamh, lsth), vh, depth = clt.host_step_tail(ch, cases, tabs, f, opts, alive)
        (dxd, accd, rowsd), ((ldxd, lrowsd, laccd, lgamd, lstd), vd) = loop.frame(f)
        assert all(abs(z) >= 0.1 for zs in depth for z in zs), depth
        assert not lsth.any(), f
        assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd), f
        assert np.array_equal(lacch, laccd) and np.array_equal(lrowsh, lrowsd), f
        assert vh == vd, (f, vh, vd)
        assert alive == form.alive, f
        n_behind += sum(v.count(0) for v in vh); n_moved += sum(v.count(1) for v in vh)
        n_erased += sum(len([l for l in c["frames"][f]["erase"]]) for c in cases)
        lm_rows += int(lrowsh.sum())
        nom, Ps = device_state(cd, B)
        for b in range(B):
            worst_t = max(worst_t, assert_table(nom[b], tabs[b], 1e-9, (f, b)))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape, (f, b)
            worst_p = max(worst_p, rel(Ps[b], Ph))
            assert rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
            assert np.array_equal(Ps[b], Ps[b].T), (f, b)
        print("frame %2d  anchor changes %s  landmark rows %s" % (f, [len(v) for v in vh], list(lrowsh)))
    print("worst table value %.3e  worst P %.3e  moved %d  behind %d  erased %d" % (worst_t, worst_p, n_moved, n_behind, n_erased))
    assert n_behind >= 1 and n_moved >= B and n_erased >= 1 and lm_rows > 0
    assert all(len(a) < L_LOOP for a in alive)
    ch.close(); cd.close()


def test_closed_loop_oldest_clone_leaves_every_frame(sw_cases):
    closed_loop(sw_cases, 12)


def test_closed_loop_two_clones_leave_every_other_frame(kf_cases):
    closed_loop(kf_cases, 12)


def run_device_loop(ctx, cases, frames, pipelined):
    out = cl.DeviceLoop(ctx, cases, frames, clt.TailForm(clm.lm_opts(), cases), pipelined=pipelined).run()
    return out, device_state(ctx, len(cases))


def same_outputs(o0, o1, cases):
    for f, ((fa, (la, va)), (fb, (lb, vb))) in enumerate(zip(o0, o1)):
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[2], fb[2]), f
        for i, c in enumerate(cases):                                    # accept flags exist for the frame's features only
            nf = len(c["frames"][f]["delta"]["feat_track"])
            assert np.array_equal(fa[1][i, :nf], fb[1][i, :nf]), (f, i)
        for x, y in zip(la, lb):
            assert np.array_equal(x, y), f
        assert va == vb, f


def test_pipelined_loop_equals_serial_loop(sw_cases):
    cases = sw_cases
    res = []
    for pipelined in (False, True):
        ctx = loop_ctx(cases, True, 12)
        res.append(run_device_loop(ctx, cases, range(len(cases[0]["frames"])), pipelined))
        ctx.close()
    same_outputs(res[0][0], res[1][0], cases)
    same_state(res[0][1], res[1][1])
    assert sum(v.count(0) for _, (_, vs) in res[0][0] for v in vs) >= 1


def test_snapshot_restore_replays_bit_for_bit(sw_cases):
    cases, N = sw_cases, 4
    ctx = loop_ctx(cases, True, 12)
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            ctx.restore()
            ctx.tracks_create(F_LOOP)                                    # the track store is not part of the snapshot
        runs.append(run_device_loop(ctx, cases, range(N), False))
    same_outputs(runs[0][0], runs[1][0], cases)
    same_state(runs[0][1], runs[1][1])
    assert [ctx.n(b) for b in range(len(cases))] == [r.shape[0] for r in runs[1][1][1]]
    ctx.close()
