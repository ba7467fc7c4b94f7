"""The second MSCKF update of a camera frame as an update-only frame from the table and the track store
(include/ingvio_hip.h: ingvio_update_stage_tracks_nominal, ingvio_frame_fetch_tri).

The reference's camera callback runs two MSCKF updates (IngvioFilter.cpp:271-324); the second one triangulates its features from every
stored observation and updates with selected stamps only.  Checked here: one such frame against the host-fed ingvio_msckf_update_tri +
ingvio_marginalize on the values of ingvio_nominal_get (and one filter against the oracle's dense evaluation), what the run leaves in the
track store, the two-update closed loop against the host reference loop (serial, pipelined, snapshot / restore), the in-frame landmark
stage on the update-only frame, the key-frame cadence with ingvio_nominal_tail behind it, a window of 17 / 19 clones, and the refusals.
The conditions these comparisons rest on are asserted on the CPU (tests/test_update_form_model.py).  1e-9 between device form and host form is the bound of the loop tests of DESIGN 4.11."""
import copy

import numpy as np
import pytest

from conftest import rel_err as rel
from ingvio_amd.closed_loop import device_loop, loop_ctx, nominal_stage
from ingvio_amd.closed_loop_update import (N_LOST, device_loop_update, host_step_update, host_table_of, host_update_frames, make_update_loop,
                                            table_clones, update_stage)
from nominal_helpers import assert_table, device_state, refused, same_state, table_ctx

pytestmark = pytest.mark.gpu

B, F, FRAMES = 8, 24, 10


@pytest.fixture(scope="module")
def stereo_cases():
    return make_update_loop(B, FRAMES, F)


@pytest.fixture(scope="module")
def mono_cases():
    # (a mono point needs more than four observations and 0.1 m of parallax, Triangulator.cpp:183-192: longer windows, no k = 1)
    return make_update_loop(4, 8, F, stereo=False, ks=(9, 10, 33), windows=(7, 9, 10, 11))


def advance(ctx, cases, n):
    """n camera frames of the two-update device loop, then the first update of camera frame n: the second one is due"""
    device_loop_update(ctx, cases, list(range(n)), False)
    nominal_stage(ctx, cases, n)()
    ctx.frame_run()
    return ctx.frame_fetch()


# ---- 1. one update-only frame against the host-fed entry points ----------------------------------------------------------------
@pytest.mark.parametrize("which,tri,sel,marg", [("stereo", True, True, True), ("stereo", True, False, True), ("stereo", True, True, False),
                                                ("mono", True, True, True), ("stereo", False, True, True)])
def test_update_only_frame_equals_host_fed_update(which, tri, sel, marg, stereo_cases, mono_cases):
    from ingvio_amd import capi
    from oracle import oracle as orc
    cases = stereo_cases if which == "stereo" else mono_cases
    nb, f = len(cases), 5
    cd = table_ctx(cases, F)
    advance(cd, cases, f)
    nom, Ps = device_state(cd, nb)
    stores = [cd.debug_tracks_read(b) for b in range(nb)]
    # the host form on a second context: the same covariances, clone poses and stored observations
    ch = loop_ctx(cases, F)
    for b in range(nb):
        ch.cov_set(b, Ps[b])
    frames, tri_masks = host_update_frames(cd, cases, [table_clones(nm) for nm in nom], f, sel)
    stereo = which == "stereo"
    if tri:
        dxh, acch, _, rowsh, pfh, okh = ch.msckf_update_tri(0, frames, selected_variant=1 if sel else 0, stereo=stereo, tri_masks=tri_masks)
    else:
        for b, fr in enumerate(frames):
            fr["pf"] = stores[b][2][np.asarray(cases[b]["frames"][f]["upd"]["feat_track"], dtype=np.int64)]
        dxh, acch, _, rowsh = ch.msckf_update(0, frames, selected_variant=1 if sel else 0)
    tabs = [host_table_of(nm) for nm in nom]
    for b, c in enumerate(cases):
        tabs[b].box_plus(dxh[b])
        if marg:
            ch.marginalize(b, c["frames"][f]["marg_upd"], 6)
            tabs[b].marginalize(c["frames"][f]["marg_upd"])
    # the device form
    update_stage(cd, cases, f, tri=tri, marg=marg, sel=sel)()
    cd.frame_run()
    dxd, accd, rowsd = cd.frame_fetch()
    nf = F - N_LOST                                                       # (flags and points exist for the frame's features only)
    if tri:
        pfd, okd = cd.frame_fetch_tri()
        assert np.array_equal(okd[:, :nf], okh[:, :nf]) and np.array_equal(pfd[:, :nf], pfh[:, :nf])      # same kernel, same input bits
        assert (okd[:, :nf] == 1).sum() >= 8 * nb and (okd[:, :nf] != 1).any()
    else:
        with pytest.raises(capi.IngvioError) as e:
            cd.frame_fetch_tri()
        assert e.value.code == capi.E_ARG
    assert np.array_equal(accd[:, :nf], acch[:, :nf]) and np.array_equal(rowsd, rowsh)
    # the comparison carries real updates: a filter whose features are all gated out (one of the four mono filters is) compares the
    # marginalisation only, so at least three filters in four must have rows, with 8 accepted features per filter on average
    assert (rowsd > 0).sum() >= 3 * nb // 4 and accd[:, :nf].sum() >= 8 * nb and (accd[:, :nf] == 0).any()
    nomd, Pd = device_state(cd, nb)
    for b in range(nb):
        assert rel(dxd[b], dxh[b]) <= 1e-9, (b, rel(dxd[b], dxh[b]))
        Ph = ch.cov_get(b)
        assert Pd[b].shape == Ph.shape and rel(Pd[b], Ph) <= 1e-9, (b, rel(Pd[b], Ph))
        assert_table(nomd[b], tabs[b], 1e-9, b)
    # one filter against the oracle's dense evaluation, at the bounds tests/test_gpu_parity.py has for the frame update
    b = int(np.argmax(rowsd))
    fr = dict(frames[b])
    if tri:
        fr["pf"] = pfd[b, :len(fr["dof"])]
        fr["obs_mask"] = np.where(okd[b, :len(fr["dof"])] == 1, fr["obs_mask"], np.uint64(0))
    oc = orc.Cov(Ps[b], ld=cd.ldp)
    dxo, acco, _, _ = oc.msckf_update(fr, max_accept=0, compress_rule=1, selected_variant=1 if sel else 0)
    if marg:
        oc.marginalize(cases[b]["frames"][f]["marg_upd"], 6)
    assert np.array_equal(accd[b, :len(acco)], acco)
    assert rel(Pd[b], oc.P) < 1e-11 and rel(dxd[b, :len(dxo)], dxo) < 1e-9, (rel(Pd[b], oc.P), rel(dxd[b, :len(dxo)], dxo))
    cd.close(); ch.close()


# ---- 2. what the run leaves in the track store -----------------------------------------------------------------------------------
def test_triangulated_points_reach_the_store_and_the_next_frame(stereo_cases):
    cases = stereo_cases
    f = 5
    cd = table_ctx(cases, F)
    advance(cd, cases, f)
    before = [cd.debug_tracks_read(b) for b in range(B)]
    update_stage(cd, cases, f)()
    cd.frame_run()
    cd.frame_fetch()
    pf, ok = cd.frame_fetch_tri()
    hit = 0
    for b, c in enumerate(cases):
        mask, uv, spf = cd.debug_tracks_read(b)
        assert np.array_equal(mask, before[b][0]) and np.array_equal(uv, before[b][1])
        want = before[b][2].copy()
        for j, t in enumerate(c["frames"][f]["upd"]["feat_track"]):
            if ok[b, j] == 1:
                want[t] = pf[b, j]; hit += 1
        assert np.array_equal(spf, want), b
    assert hit >= 8 * B
    # the next camera frame's first update lists track N_LOST without triangulating: the staged point is the store's
    nominal_stage(cd, cases, f + 1)()
    for b, c in enumerate(cases):
        j = c["frames"][f + 1]["delta"]["feat_track"].index(N_LOST)
        ju = c["frames"][f]["upd"]["feat_track"].index(N_LOST)
        assert ok[b, ju] == 1 and np.array_equal(cd.debug_staged_frame(b)["pf"][j], pf[b, ju]), b
    cd.frame_run()
    assert cd.frame_fetch()[2].min() > 0
    cd.close()


# ---- 3. the two-update closed loop -------------------------------------------------------------------------------------------------
def test_two_update_loop_equals_host_loop(stereo_cases):
    cases = stereo_cases
    ch, cd = loop_ctx(cases, F), table_ctx(cases, F)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    points = [dict() for _ in cases]
    out = device_loop_update(table_ctx(cases, F), cases, list(range(FRAMES)), True)      # the pipelined loop, compared frame by frame below
    accepted = failed = 0
    for f in range(FRAMES):
        h1, h2 = host_step_update(ch, cases, tabs, f, points)
        (d1, d2), = device_loop_update(cd, cases, [f], False)
        n1, n2 = len(cases[0]["frames"][f]["delta"]["feat_track"]), len(cases[0]["frames"][f]["upd"]["feat_track"])      # (the same for every filter)
        p1, p2 = out[f]
        for x, y in ((p1[0], d1[0]), (p1[1][:, :n1], d1[1][:, :n1]), (p1[2], d1[2]), (p2[0], d2[0]), (p2[1][:, :n2], d2[1][:, :n2]), (p2[2], d2[2]),
                     (p2[3][:, :n2], d2[3][:, :n2]), (p2[4][:, :n2], d2[4][:, :n2])):
            assert np.array_equal(x, y), f                                # pipelined equals serial, bit for bit
        assert np.array_equal(h1[1][:, :n1], d1[1][:, :n1]) and np.array_equal(h1[2], d1[2]), f
        assert np.array_equal(h2[1][:, :n2], d2[1][:, :n2]) and np.array_equal(h2[3], d2[2]) and np.array_equal(h2[5][:, :n2], d2[4][:, :n2]), f
        accepted += int(d2[1][:, :n2].sum()); failed += int((d2[4][:, :n2] != 1).sum())
        nom, Ps = device_state(cd, B)
        for b in range(B):
            assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape and rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
    assert accepted >= 8 * B * (FRAMES - 3) and failed > 0
    ch.close(); cd.close()


def test_two_update_loop_snapshot_restore(stereo_cases):
    cases = stereo_cases
    ctx = table_ctx(cases, F)
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            ctx.restore()
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        runs.append((device_loop_update(ctx, cases, [0, 1, 2, 3], False), device_state(ctx, B), [ctx.debug_tracks_read(b) for b in range(B)]))
    (o0, s0, t0), (o1, s1, t1) = runs
    for f, ((a1, a2), (b1, b2)) in enumerate(zip(o0, o1)):
        assert np.array_equal(a1[0], b1[0]) and np.array_equal(a1[2], b1[2]) and np.array_equal(a2[0], b2[0]) and np.array_equal(a2[2], b2[2]), f
        for i, c in enumerate(cases):                                    # flags and points exist for the frame's features only
            nf = len(c["frames"][f]["upd"]["feat_track"])
            assert np.array_equal(a2[1][i, :nf], b2[1][i, :nf]) and np.array_equal(a2[3][i, :nf], b2[3][i, :nf]) and np.array_equal(a2[4][i, :nf], b2[4][i, :nf]), (f, i)
    assert sum(int(a2[2].sum()) for _, a2 in o0) > 0
    same_state(s0, s1, keys=("kind", "idx", "val", "clone_var"))
    for a, b in zip(t0, t1):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    ctx.close()


# ---- 4. the in-frame landmark stage on the update-only frame ---------------------------------------------------------------------------
def test_landmark_stage_on_the_update_only_frame():
    """closed_loop_lm's six landmarks, 4 filters x 6 camera frames: the landmark update staged from the table behind the update-only
    frame's stage runs behind the second MSCKF update and in front of its marginalisation (IngvioFilter.cpp:281-289), against the host
    loop in that order; masks and rows equal, tables and P to 1e-9 (the bounds of tests/test_gpu_nominal_landmarks.py)"""
    from ingvio_amd import closed_loop_lm as clm
    from ingvio_amd.closed_loop_update import split_updates
    nb, nfr, L = 4, 6, 6
    cases = split_updates(clm.make_lm_loop(nb, nfr, L=L, F=F), F)
    opts = clm.lm_opts()
    ch, cd = loop_ctx(cases, F), table_ctx(cases, F)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    points = [dict() for _ in cases]
    lm_rows = lm_refused = 0
    for f in range(nfr):
        h1, h2, hl = host_step_update(ch, cases, tabs, f, points, lm_opts=opts)
        nominal_stage(cd, cases, f)()
        cd.frame_run()
        d1 = cd.frame_fetch()
        update_stage(cd, cases, f)()
        clm.lm_stage_call(cd, cases, f, opts)()
        cd.frame_run()
        d2 = cd.frame_fetch()
        dok = cd.frame_fetch_tri()[1]
        dl = cd.landmark_fetch()
        n1, n2 = len(cases[0]["frames"][f]["delta"]["feat_track"]), len(cases[0]["frames"][f]["upd"]["feat_track"])
        assert np.array_equal(h1[1][:, :n1], d1[1][:, :n1]) and np.array_equal(h1[2], d1[2]), f
        assert np.array_equal(h2[1][:, :n2], d2[1][:, :n2]) and np.array_equal(h2[3], d2[2]) and np.array_equal(h2[5][:, :n2], dok[:, :n2]), f
        assert np.array_equal(hl[1], dl[1]) and np.array_equal(hl[2][:, :L], dl[2][:, :L]) and not dl[4].any(), f
        lm_rows += int(dl[1].sum()); lm_refused += int((dl[2][:, :L] == 0).sum())
        nom, Ps = device_state(cd, nb)
        for b in range(nb):
            assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape and rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
    assert lm_rows >= 4 * nb * nfr and lm_refused > 0                     # (real landmark updates, both verdicts)
    ch.close(); cd.close()


# ---- 5. the key-frame cadence: marg_idx = -1, the clones leave through ingvio_nominal_tail -----------------------------------------------
def test_keyframe_cadence_with_the_nominal_tail():
    """4 filters x 6 camera frames: neither update marginalises, behind every other camera frame ingvio_nominal_tail drops two clones;
    against the host loop (ingvio_marginalize one clone at a time)"""
    from ingvio_amd import capi
    from ingvio_amd.closed_loop_update import host_tail_drop, make_keyframe_loop
    nb, nfr = 4, 6
    cases = make_keyframe_loop(nb, nfr, F)

    def ctx_of(table):
        n_max = max(c["P"].shape[0] for c in cases) + 18                 # the window grows by two clones before two leave
        ctx = capi.Context(batch=nb, n_max=((n_max + 15) // 16) * 16, c_max=12, f_max=F, m_max=64)
        for b, c in enumerate(cases):
            ctx.cov_set(b, c["P"])
        ctx.tracks_create(F)
        if table:
            ctx.nominal_create(48)
            ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
        return ctx
    ch, cd = ctx_of(False), ctx_of(True)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    points = [dict() for _ in cases]
    rows = dropped = 0
    for f in range(nfr):
        h1, h2 = host_step_update(ch, cases, tabs, f, points)
        slots = [[t.clones[q] for q in c["frames"][f]["tail_pos"]] for c, t in zip(cases, tabs)]      # (before the host drops them)
        host_tail_drop(ch, cases, tabs, f)
        (d1, d2), = device_loop_update(cd, cases, [f], False)
        if any(slots):
            verdict, status = cd.nominal_tail(0, [dict(marg_slot=s) for s in slots])
            assert not status.any(), f
            dropped += sum(len(s) for s in slots)
        n1, n2 = len(cases[0]["frames"][f]["delta"]["feat_track"]), len(cases[0]["frames"][f]["upd"]["feat_track"])
        assert np.array_equal(h1[1][:, :n1], d1[1][:, :n1]) and np.array_equal(h1[2], d1[2]), f
        assert np.array_equal(h2[1][:, :n2], d2[1][:, :n2]) and np.array_equal(h2[3], d2[2]) and np.array_equal(h2[5][:, :n2], d2[4][:, :n2]), f
        rows += int(d2[2].sum())
        nom, Ps = device_state(cd, nb)
        for b in range(nb):
            assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape and rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
    assert rows > 0 and dropped == 2 * nb * (nfr // 2)
    ch.close(); cd.close()


# ---- 7. a large window ---------------------------------------------------------------------------------------------------------------
def test_two_update_loop_large_window():
    """2 filters, windows of 17 and 19 clones (the large-window kernels), F = 12, 3 camera frames, both updates, against the
    host reference loop; the frame from the table has no other test above 12 clones"""
    from ingvio_amd import capi
    Fl, nfr = 12, 3
    cases = make_update_loop(2, nfr, Fl, windows=(17, 19), ks=(10, 9))

    def ctx_of(table):
        n_max = max(c["P"].shape[0] for c in cases) + 6
        ctx = capi.Context(batch=2, n_max=((n_max + 15) // 16) * 16, c_max=20, f_max=Fl, m_max=64)
        for b, c in enumerate(cases):
            ctx.cov_set(b, c["P"])
        ctx.tracks_create(Fl)
        if table:
            ctx.nominal_create(48)
            ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
        return ctx
    ch, cd = ctx_of(False), ctx_of(True)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    points = [dict() for _ in cases]
    rows = 0
    for f in range(nfr):
        h1, h2 = host_step_update(ch, cases, tabs, f, points)
        (d1, d2), = device_loop_update(cd, cases, [f], False)
        n1, n2 = len(cases[0]["frames"][f]["delta"]["feat_track"]), len(cases[0]["frames"][f]["upd"]["feat_track"])
        assert np.array_equal(h1[1][:, :n1], d1[1][:, :n1]) and np.array_equal(h1[2], d1[2]), f
        assert np.array_equal(h2[1][:, :n2], d2[1][:, :n2]) and np.array_equal(h2[3], d2[2]) and np.array_equal(h2[5][:, :n2], d2[4][:, :n2]), f
        rows += int(d1[2].sum()) + int(d2[2].sum())
        nom, Ps = device_state(cd, 2)
        for b in range(2):
            assert_table(nom[b], tabs[b], 1e-9, (f, b))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape and rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
    assert rows > 0
    ch.close(); cd.close()


# ---- 6. refusals; the other frames after it ------------------------------------------------------------------------------------------
def test_refusals_leave_everything_unchanged(stereo_cases):
    from ingvio_amd import capi
    cases = stereo_cases[:4]
    nb, f = len(cases), 5
    opts = cases[0]["frame"]
    upd = [c["frames"][f]["upd"] for c in cases]
    marg = [c["frames"][f]["marg_upd"] for c in cases]
    # no table / no track store
    ctx = capi.Context(batch=nb, n_max=160, c_max=12, f_max=F, m_max=64)
    with pytest.raises(capi.IngvioError) as e:
        ctx.update_stage_tracks_nominal_prepare(0, marg, upd, opts)()
    assert e.value.code == capi.E_ARG
    ctx.nominal_create(48)
    with pytest.raises(capi.IngvioError) as e:
        ctx.update_stage_tracks_nominal_prepare(0, marg, upd, opts)()
    assert e.value.code == capi.E_ARG
    ctx.close()
    ctx = table_ctx(cases, F)
    advance(ctx, cases, f)

    def store():
        return [ctx.debug_tracks_read(b) for b in range(nb)]

    def no(fn, code):
        s0 = store()
        refused(ctx, fn, code, sizes=True)
        for a, b in zip(s0, store()):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    stage = lambda **kw: update_stage(ctx, cases, f, **kw)
    no(ctx.update_stage_tracks_nominal_prepare(1, marg[1:], upd[1:], opts), capi.E_ARG)                       # not the whole batch
    no(ctx.update_stage_tracks_nominal_prepare(0, marg, [dict(u, append=3) for u in upd], opts), capi.E_ARG)
    no(ctx.update_stage_tracks_nominal_prepare(0, marg, [dict(u, append=3, obs_track=[0], obs_uv=np.zeros((1, 4))) for u in upd], opts), capi.E_ARG)
    no(ctx.update_stage_tracks_nominal_prepare(0, [3] * nb, upd, opts), capi.E_NOT_IN_STATE)                  # no clone of the window
    first = [c["table"].slots[c["table"].clones[0]]["idx"] for c in cases]                                    # the landmarks' anchor
    no(ctx.update_stage_tracks_nominal_prepare(0, first, upd, opts), capi.E_ARG)
    ctx.set_frame_parts(2)
    no(stage(), capi.E_UNSUPPORTED)
    ctx.set_frame_parts(1)
    with pytest.raises(capi.IngvioError) as e:                                                               # nothing ran that triangulated
        ctx.frame_fetch_tri()
    assert e.value.code == capi.E_ARG
    stage()()
    no(stage(), capi.E_ARG)                                                                                   # a second stage from the table
    no(nominal_stage(ctx, cases, f + 1), capi.E_ARG)
    no(lambda: ctx.gnss_frame_stage_nominal(0, [None] * nb, opts["chi2_table"]), capi.E_UNSUPPORTED)
    no(lambda: ctx.frame_run_phase(1), capi.E_UNSUPPORTED)
    no(lambda: ctx.frame_run(restore_prior=True), capi.E_ARG)
    ctx.set_frame_parts(2)
    no(lambda: ctx.frame_run(), capi.E_UNSUPPORTED)
    ctx.set_frame_parts(1)
    ctx.frame_run()                                                                                           # it still runs, once
    ctx.frame_fetch()
    no(lambda: ctx.frame_run(), capi.E_ARG)
    state = device_state(ctx, nb), store()
    ctx.close()
    # the same frames on a context that was never refused anything: bit for bit the same state
    ctx = table_ctx(cases, F)
    device_loop_update(ctx, cases, list(range(f + 1)), False)
    same_state(state[0], device_state(ctx, nb))
    for a, b in zip(state[1], [ctx.debug_tracks_read(b) for b in range(nb)]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ctx.close()


def test_other_frames_after_an_update_only_frame_run_as_before():
    """a plain loop's frames and a flattened ingvio_frame_stage give the same bits whether or not an update-only frame (without features,
    marginalising nothing: it leaves state and store alone) ran in front of them"""
    from ingvio_amd.closed_loop import make_loop
    cases = make_loop(4, 4)
    res = []
    for with_update in (False, True):
        ctx = table_ctx(cases, F)
        out = []
        for f in range(3):
            if with_update:
                empty = [dict(feat_track=[], feat_anchor=[], feat_dof=[]) for _ in cases]
                ctx.update_stage_tracks_nominal_prepare(0, [-1] * len(cases), empty, cases[0]["frame"], tri={})()
                ctx.frame_run()
                assert not ctx.frame_fetch()[2].any()
            out += device_loop(ctx, cases, [f], False)
        ctx.frame_stage(0, [c["step"] for c in cases], [c["frame"] for c in cases], cases[0]["step"]["sigma"], 1, 0.2, 0.2)
        ctx.frame_run()
        out.append(ctx.frame_fetch())
        res.append((out, device_state(ctx, len(cases))))
        ctx.close()
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    same_state(res[0][1], res[1][1], keys=("kind", "idx", "val", "clone_var"))
