"""ingvio_landmark_init_nominal (k_delayed_front<true>, kernels_delayed.hip): LandmarkUpdate::initNewLandmark{Mono,Stereo} from the
track store and the nominal table.  Scenarios and the CPU references are landmark_init_helpers.py's; their conditions (verdicts, distance
from the gate, the order gap) are asserted on the CPU by tests/test_landmark_init_scenarios.py."""
import ctypes as C

import numpy as np
import pytest

import landmark_init_helpers as H
from conftest import rel_err

V_MAX = 48


def dev_ctx(scn, batch=None):
    """a context with the scenario's covariances, tables and track store (filled column by column through the store's delta)"""
    from ingvio_amd import capi
    B = batch or len(scn)
    n_max = ((max(f["P"].shape[0] for f in scn) + 12 + 15) // 16) * 16
    ctx = capi.Context(batch=B, n_max=n_max, c_max=16, f_max=H.N_TRACKS, m_max=64)
    ctx.tracks_create(H.N_TRACKS)
    ctx.nominal_create(V_MAX)
    fs = [scn[b % len(scn)] for b in range(B)]
    for b, f in enumerate(fs):
        ctx.cov_set(b, f["P"])
    ctx.nominal_set(0, [f["table"].as_dict() for f in fs])
    raw = dict(imu=np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 9.8, 0.005]]), R=np.eye(3), p=np.zeros(3), v=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3),
               gravity=np.array([0.0, 0.0, -9.8]))
    sigma = fs[0]["case"]["step"]["sigma"]
    for col in range(max(f["uv"].shape[1] for f in fs)):
        frames = []
        for f in fs:
            tr = [j for j in range(H.N_TRACKS) if col < f["uv"].shape[1] and (int(f["mask"][j]) >> col) & 1]
            frames.append(dict(append=col if tr else -1, obs_track=tr, obs_uv=f["uv"][tr, col] if tr else np.zeros((0, 4)), clone_idx=[],
                               clone_R=np.zeros((0, 9)), clone_p=np.zeros((0, 3)), feat_track=[], feat_anchor=[], feat_dof=[]))
        ctx.frame_stage_tracks_prepare(0, [dict(raw=raw)] * B, frames, H.opts_frame(fs[0]["stereo"]), sigma)()
    ctx.sync()
    return ctx, fs


def table_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("kind", "idx", "anchor", "val", "clone_var"))


def check_against_oracle(ctx, b, got, ref, what):
    ga, gi, gc, gd, gs = got
    assert ga == ref["added"] and gi == ref["new_idx"] and gs == ref["slot"], (what, b, got[:2], gs, ref["added"], ref["new_idx"], ref["slot"])
    for j, a in enumerate(ref["added"]):
        assert abs(gc[j] - ref["chi2"][j]) <= 1e-9 * max(1.0, ref["chi2"][j]), (what, b, j, gc[j], ref["chi2"][j])
        if a:
            assert np.linalg.norm(gd[j] - ref["dx"][j]) < 1e-9 * max(1.0, np.linalg.norm(ref["dx"][j])), (what, b, j)
        else:
            assert gd[j] is None
    assert ctx.n(b) == ref["n"]
    Pg = ctx.cov_get(b)
    assert np.linalg.norm(Pg - ref["P"]) / np.linalg.norm(ref["P"]) < 1e-11, (what, b)


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [True, False])
def test_rows(stereo):
    """the debug hook's rows against the numpy restatement: 1e-11 of max|H|, m exactly; windows of 3, 6, 11 and 12 clones, no /
    one / two pending drop columns (column 0, a middle one, one above every observation), a mask with gaps that the anchor is not in,
    observer == anchor, a single observation"""
    scn = H.make_scenario(H.ROW_WINDOWS, seed=7, drops=H.ROW_DROPS, stereo=stereo)
    ctx, fs = dev_ctx(scn)
    o = H.opts_frame(stereo)
    for b, f in enumerate(fs):
        before = (ctx.nominal_get()[b], ctx.cov_get(b))
        for tr in (H.T_GOOD, H.T_GROSS, H.T_GAP, H.T_PAIR, H.T_SINGLE):
            H_old, H_new, r = H.rows_at(f, f["table"], tr)
            g_old, g_new, g_r = ctx.debug_landmark_init_rows(b, (tr, f["anchor"][tr], f["pf"][tr]), o, f["Cw"], f["drop"])
            assert g_old.shape == H_old.shape and g_new.shape == H_new.shape, (b, tr, g_old.shape, H_old.shape)
            s = np.abs(H_old).max()
            err = max(np.abs(g_old - H_old).max(), np.abs(g_new - H_new).max(), np.abs(g_r - r).max())
            print("rows stereo=%d window=%d track=%d m=%d err/max|H|=%.2e" % (stereo, f["Cw"], tr, H_old.shape[0], err / s))
            assert err <= 1e-11 * s, (b, tr, err / s)
        after = (ctx.nominal_get()[b], ctx.cov_get(b))
        assert table_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    if not stereo:                                               # one mono observation: m = 2 <= 3, skipped on the device, state bit-unchanged
        s0 = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(len(fs))])
        got = ctx.landmark_init_nominal(0, H.blocks_of(fs, [[H.T_SINGLE]] * len(fs)), o)
        for b in range(len(fs)):
            assert got[b][0] == [False] and got[b][1] == [-1] and got[b][2] == [0.0] and got[b][4] == [-1]
            assert table_equal(s0[0][b], ctx.nominal_get()[b]) and np.array_equal(s0[1][b], ctx.cov_get(b)) and ctx.n(b) == fs[b]["P"].shape[0]
    ctx.close()


def host_round_trip(ch, fs, tracks_per_filter, o):
    """the round-trip form on a context of the same type: nominal_get -> numpy rows -> add_variable_delayed_batch -> append to the table ->
    nominal_set -> nominal_box_plus, candidate by candidate"""
    from ingvio_amd import capi, synth
    tab = synth.chi2_table()
    out = [dict(added=[], new_idx=[], chi2=[], dx=[], slot=[]) for _ in fs]
    for j in range(max(len(t) for t in tracks_per_filter)):
        dev = ch.nominal_get()
        blocks, meta = [], []
        for b, f in enumerate(fs):
            if j >= len(tracks_per_filter[b]):
                blocks.append([]); meta.append(None); continue
            tr = tracks_per_filter[b][j]
            d = dev[b]
            cl = list(d["clone_var"])
            cR = [d["val"][s][0:9].reshape(3, 3) for s in cl]; cp = [d["val"][s][9:12] for s in cl]
            H_old, H_new, r = H.numpy_rows(cR, cp, f["pf"][tr], f["anchor"][tr], H.obs_of(f, tr), f["stereo"])
            vidx = [int(d["idx"][s]) for s in cl]
            blocks.append([(vidx, [6] * len(vidx), H_old, H_new, r, tab[H_old.shape[0]])]); meta.append((tr, cl))
        got = ch.add_variable_delayed_batch(0, blocks, H.NOISE)
        dxp = np.zeros((len(fs), ch.ldp))
        for b, f in enumerate(fs):
            if meta[b] is None:
                continue
            tr, cl = meta[b]
            a, i, g, dx = got[b][0][0], got[b][1][0], got[b][2][0], got[b][3][0]
            d = dev[b]
            free = [v for v in range(V_MAX) if v >= len(d["kind"]) or d["kind"][v] == capi.NOM_NONE]
            slot = free[sum(1 for x in out[b]["added"] if not x)] if a else -1      # the refused candidates before it left their slots free
            out[b]["added"].append(a); out[b]["new_idx"].append(i); out[b]["chi2"].append(g); out[b]["dx"].append(dx); out[b]["slot"].append(slot)
            if a:
                while len(d["kind"]) <= slot:
                    d["kind"] = np.append(d["kind"], capi.NOM_NONE); d["idx"] = np.append(d["idx"], -1); d["anchor"] = np.append(d["anchor"], -1)
                    d["val"] = np.vstack([d["val"], np.zeros(15)])
                row = np.zeros(15); row[0:9] = np.eye(3).reshape(9); row[9:12] = f["pf"][tr]
                d["kind"][slot] = capi.NOM_LANDMARK; d["idx"][slot] = i; d["anchor"][slot] = cl[f["anchor"][tr]]; d["val"][slot] = row
                dxp[b, :len(dx)] = dx
        ch.nominal_set(0, dev)
        ch.nominal_box_plus(0, dxp)
    return out


def compare_contexts(cd, ch, got, ref, fs, what):
    dd, dh = cd.nominal_get(), ch.nominal_get()
    for b in range(len(fs)):
        assert got[b][0] == ref[b]["added"] and got[b][1] == ref[b]["new_idx"] and got[b][4] == ref[b]["slot"], (what, b, got[b], ref[b])
        for j, a in enumerate(ref[b]["added"]):
            assert abs(got[b][2][j] - ref[b]["chi2"][j]) <= 1e-9 * max(1.0, ref[b]["chi2"][j]), (what, b, j)
            if a:
                assert rel_err(got[b][3][j], ref[b]["dx"][j]) < 1e-9, (what, b, j)
        assert cd.n(b) == ch.n(b) and rel_err(cd.cov_get(b), ch.cov_get(b)) < 1e-9, (what, b)
        for k in ("kind", "idx", "anchor", "clone_var"):
            assert np.array_equal(dd[b][k], dh[b][k]), (what, b, k)
        assert rel_err(dd[b]["val"], dh[b]["val"]) < 1e-9, (what, b)


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [True, False])
def test_one_candidate_per_filter(stereo):
    """a mixed batch (windows 3, 5, 8, 11), every filter's good candidate, then every filter's refused one"""
    scn = H.make_scenario(H.MIXED_WINDOWS, seed=11, stereo=stereo)
    o = H.opts_frame(stereo)
    cd, fs = dev_ctx(scn)
    ch, _ = dev_ctx(scn)
    tracks = [[H.T_GOOD]] * len(fs)
    got = cd.landmark_init_nominal(0, H.blocks_of(fs, tracks), o)
    assert list(cd.delayed_status) == [0] * len(fs)
    compare_contexts(cd, ch, got, host_round_trip(ch, fs, tracks, o), fs, "accepted")
    for b, f in enumerate(fs):
        ref = H.oracle_sequence(f, [H.T_GOOD])
        assert ref["added"] == [True]
        check_against_oracle(cd, b, got[b], ref, "accepted")
    s0 = (cd.nominal_get(), [cd.cov_get(b) for b in range(len(fs))], [cd.n(b) for b in range(len(fs))])
    got = cd.landmark_init_nominal(0, H.blocks_of(fs, [[H.T_GROSS]] * len(fs)), o)
    s1 = cd.nominal_get()
    for b in range(len(fs)):                                     # refused: P, n and the table bit-unchanged, the slot stays free
        assert got[b][0] == [False] and got[b][1] == [-1] and got[b][4] == [-1] and got[b][3] == [None] and got[b][2][0] > 0.0
        assert cd.n(b) == s0[2][b] and np.array_equal(cd.cov_get(b), s0[1][b]) and table_equal(s0[0][b], s1[b])
    cd.close(); ch.close()


@pytest.mark.gpu
def test_sequences_follow_the_reference_order():
    """three candidates, the middle one refused: the third one's rows are formed after the first one's boxPlus"""
    from ingvio_amd import capi
    import ingvio_amd.closed_loop_lm as clm
    scn = H.make_scenario(H.SEQ_WINDOWS, seed=21)
    o = H.opts_frame(True)
    cd, fs = dev_ctx(scn)
    ch, _ = dev_ctx(scn)
    tracks = [list(H.SEQ_TRACKS)] * len(fs)
    got = cd.landmark_init_nominal(0, H.blocks_of(fs, tracks), o)
    compare_contexts(cd, ch, got, host_round_trip(ch, fs, tracks, o), fs, "sequence")
    dev = cd.nominal_get()
    for b, f in enumerate(fs):
        ref = H.oracle_sequence(f, H.SEQ_TRACKS)
        up = H.oracle_sequence(f, H.SEQ_TRACKS, reform=False)
        check_against_oracle(cd, b, got[b], ref, "sequence")
        free = H.free_slots(f["table"])
        assert got[b][4] == [free[0], -1, free[2]]
        assert dev[b]["kind"][free[0]] == capi.NOM_LANDMARK and dev[b]["kind"][free[1]] == capi.NOM_NONE and dev[b]["kind"][free[2]] == capi.NOM_LANDMARK
        assert dev[b]["anchor"][free[2]] == f["table"].clones[f["anchor"][H.T_GOOD2]]
        # the rows-up-front order is a different result: the CPU scenario test measured the gap (> 1e-6), the device is 1e-9 from the other
        gap = abs(up["chi2"][2] - ref["chi2"][2]) / max(1.0, ref["chi2"][2])
        assert gap > 1e-6 and abs(got[b][2][2] - up["chi2"][2]) / max(1.0, ref["chi2"][2]) > 0.5 * gap
        assert rel_err(got[b][3][2], up["dx"][2]) > 0.5 * rel_err(ref["dx"][2], up["dx"][2]) > 5e-7
    # the host mirror knows the new landmarks: a landmark update staged on them from the table runs
    lo = clm.lm_opts()
    frames = []
    for b, f in enumerate(fs):
        sl = [s for s in got[b][4] if s >= 0]
        frames.append(dict(lm_var=sl, uv=np.stack([f["uv"][tr, f["cols"][f["Cw"] - 1]] for tr in (H.T_GOOD, H.T_GOOD2)]), tracked=[1, 1]))
    cd.landmark_stage_nominal(0, frames, lo["stereo"], lo["noise"], lo["chi2_thr"], lo["R_cl2cr"], lo["t_cl2cr"], in_frame=False)
    cd.landmark_run()
    dx, rows, acc, gam, st = cd.landmark_fetch()
    assert np.all(np.isfinite(dx)) and list(st) == [0] * len(fs)
    cd.close(); ch.close()


@pytest.mark.gpu
def test_snapshot_restore_gives_the_same_bits():
    scn = H.make_scenario(H.SEQ_WINDOWS, seed=21)
    o = H.opts_frame(True)
    ctx, fs = dev_ctx(scn)
    blocks = H.blocks_of(fs, [list(H.SEQ_TRACKS)] * len(fs))
    ctx.snapshot()
    g1 = ctx.landmark_init_nominal(0, blocks, o)
    s1 = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(len(fs))])
    ctx.restore()
    assert [ctx.n(b) for b in range(len(fs))] == [f["P"].shape[0] for f in fs]
    g2 = ctx.landmark_init_nominal(0, blocks, o)
    s2 = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(len(fs))])
    for b in range(len(fs)):
        assert g1[b][:3] == g2[b][:3] and g1[b][4] == g2[b][4]
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(g1[b][3], g2[b][3]))
        assert table_equal(s1[0][b], s2[0][b]) and np.array_equal(s1[1][b], s2[1][b])
    ctx.close()


def raw_call(ctx, b0, nb, arr, cap, o, slot_ok=True):
    added = np.zeros((max(nb, 1), max(cap, 1)), dtype=np.int32); idx = np.zeros_like(added); slot = np.zeros_like(added)
    ip = C.POINTER(C.c_int)
    return ctx.L.ingvio_landmark_init_nominal(ctx.h, b0, nb, arr, C.byref(o), C.c_double(1.0), 1, cap, added.ctypes.data_as(ip),
                                              idx.ctypes.data_as(ip), slot.ctypes.data_as(ip) if slot_ok else None, None, None, None)


@pytest.mark.gpu
def test_refusals_and_partial_range():
    from ingvio_amd import capi, synth
    scn = H.make_scenario((5, 5, 5, 5), seed=31)
    ctx, fs = dev_ctx(scn)
    B = len(fs)
    of = H.opts_frame(True)
    o, keep_tab = capi.make_opts(of)

    def state():
        return ctx.nominal_get(), [ctx.cov_get(b) for b in range(B)], [ctx.n(b) for b in range(B)]
    s0 = state()

    def code(blocks, b0=0, nb=None, cap=None, opts=None, edit=None):
        arr, cc, keep = capi.make_lm_init_blocks(blocks)
        if edit:
            edit(arr)
        rc = raw_call(ctx, b0, len(blocks) if nb is None else nb, arr, cc if cap is None else cap, opts or o)
        s1 = state()
        assert s1[2] == s0[2] and all(np.array_equal(x, y) for x, y in zip(s0[1], s1[1])) and all(table_equal(x, y) for x, y in zip(s0[0], s1[0]))
        return rc
    f = fs[0]
    good = (H.T_GOOD, 0, f["pf"][H.T_GOOD])
    blk = lambda cands, drop=(): dict(cands=cands, drop=list(drop))
    assert code([blk([good])] * 2, b0=B - 1) == capi.E_ARG                                      # range
    assert code([blk([good, good])], cap=1) == capi.E_ARG                                      # n_cand > cand_cap
    assert code([blk([(H.N_TRACKS, 0, good[2])])]) == capi.E_ARG                               # track outside the store
    assert code([blk([(-1, 0, good[2])])]) == capi.E_ARG
    assert code([blk([(H.T_GOOD, f["Cw"], good[2])])]) == capi.E_ARG                           # anchor outside the window
    assert code([blk([good], drop=[3, 2])]) == capi.E_ARG                                      # drop_cols not ascending
    assert code([blk([good], drop=[16])]) == capi.E_ARG                                        # outside c_max
    assert code([blk([good], drop=list(range(4, 16)))]) == capi.E_ARG                          # window + drops > c_max
    short, keep2 = capi.make_opts(dict(of, chi2_table=synth.chi2_table()[:4 * f["Cw"]]))
    assert code([blk([good])], opts=short) == capi.E_ARG                                       # chi2_table too short
    assert code([blk([good])], edit=lambda a: setattr(a[0], "cand", None)) == capi.E_ARG       # NULL where data is needed
    n0 = f["P"].shape[0]
    too_many = (((n0 + 12 + 15) // 16) * 16 - n0) // 3 + 1
    assert code([blk([good] * too_many)]) == capi.E_CAPACITY                                   # n + 3 n_cand > n_max
    # a context without table / without store
    bare = capi.Context(batch=1, n_max=64, c_max=8, f_max=8, m_max=32)
    arr, cc, keep = capi.make_lm_init_blocks([blk([good])])
    assert raw_call(bare, 0, 1, arr, cc, o) == capi.E_ARG
    bare.nominal_create(8)
    assert raw_call(bare, 0, 1, arr, cc, o) == capi.E_ARG
    bare.close()
    # fewer free table slots than candidates
    small = capi.Context(batch=1, n_max=((f["P"].shape[0] + 24) // 16) * 16, c_max=16, f_max=H.N_TRACKS, m_max=64)
    small.cov_set(0, f["P"]); small.tracks_create(H.N_TRACKS); small.nominal_create(len(f["table"].slots) + 1)
    small.nominal_set(0, [f["table"].as_dict()])
    arr2, cc2, keep3 = capi.make_lm_init_blocks([blk([good, good])])
    assert raw_call(small, 0, 1, arr2, cc2, o) == capi.E_CAPACITY and small.n(0) == f["P"].shape[0]
    small.close()
    # a partial range works and leaves the other filters bit-unchanged
    got = ctx.landmark_init_nominal(1, H.blocks_of(fs[1:3], [[H.T_GOOD], [H.T_GOOD, H.T_GOOD2]]), of)
    s1 = state()
    for i, b in enumerate((1, 2)):
        check_against_oracle(ctx, b, got[i], H.oracle_sequence(fs[b], [H.T_GOOD] if i == 0 else [H.T_GOOD, H.T_GOOD2]), "partial")
    for b in (0, 3):
        assert s1[2][b] == s0[2][b] and np.array_equal(s0[1][b], s1[1][b]) and table_equal(s0[0][b], s1[0][b])
    # a frame staged from the table that has not run: refused as ingvio_add_variable_delayed_batch refuses it, accepted after the run
    from ingvio_amd.closed_loop import nominal_stage
    from nominal_helpers import refused
    nominal_stage(ctx, [f["case"] for f in fs], 0)()
    refused(ctx, lambda: ctx.landmark_init_nominal(0, H.blocks_of(fs[:1], [[H.T_PAIR]]), of), capi.E_ARG, sizes=True)
    ctx.frame_run()
    ctx.frame_fetch()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["gnss", "landmarks", "split"])
def test_refused_while_other_work_is_pending(what):
    """a GNSS epoch / a stand-alone landmark update staged from the table and not yet run, a split frame step between its halves: refused
    (INGVIO_E_ARG) with the state unchanged, as ingvio_add_variable_delayed_batch refuses them"""
    from conftest import load_golden
    from ingvio_amd import capi, host, synth
    from nominal_helpers import refused, table_ctx
    of = H.opts_frame(True)
    blocks = [dict(cands=[(0, 0, np.array([0.0, 0.0, 5.0]))], drop=[])] * 2
    if what == "split":
        ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
        cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
        ctx.tracks_create(32); ctx.nominal_create(16)
        ctx.snapshot()
        ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
        ctx.frame_run_phase(1, restore_prior=True)
        before = [(ctx.n(b), ctx.cov_get(b)) for b in range(2)]
        arr, cap, keep = capi.make_lm_init_blocks(blocks)
        o, tab = capi.make_opts(of)
        assert raw_call(ctx, 0, 2, arr, cap, o) == capi.E_ARG and b"split" in ctx.L.ingvio_last_error(ctx.h)
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
        import ingvio_amd.closed_loop_lm as clm
        cases, o = clm.make_lm_loop(2, 2), clm.lm_opts()
        ctx = table_ctx(cases)
        ctx.landmark_stage_nominal_prepare(0, clm.nominal_frames(cases, 0), o["stereo"], o["noise"], o["chi2_thr"], o["R_cl2cr"], o["t_cl2cr"],
                                           in_frame=False)()
    refused(ctx, lambda: ctx.landmark_init_nominal(0, blocks, of), capi.E_ARG, sizes=True)
    if what == "gnss":
        ctx.gnss_run(); ctx.gnss_fetch()
    else:
        ctx.landmark_run(); ctx.landmark_fetch()
    ctx.close()


def synthetic_table(Cw, idx_shift=0):
    """extended pose, biases, extrinsics and Cw clones 0.3 m apart; idx_shift moves the LAST clone's idx"""
    val = np.zeros((4 + Cw, 15)); val[:, 0] = val[:, 4] = val[:, 8] = 1.0
    for c in range(Cw):
        val[4 + c, 9] = 0.3 * c
    idx = [0, 9, 12, 15] + [21 + 6 * c for c in range(Cw)]
    idx[-1] += idx_shift
    return dict(kind=[0, 2, 2, 1] + [1] * Cw, idx=idx, anchor=[-1] * (4 + Cw), val=val, clone_var=list(range(4, 4 + Cw)), v_ext=3, v_pose=0,
                v_bg=1, v_ba=2, gravity=np.array([0.0, 0.0, -9.8]))


@pytest.mark.gpu
def test_refusals_of_size():
    """the front's LDS bound (a stereo candidate on 20 clones keeps 8 ((2 nc + 1)(m | 1) + 9 m + (m - 2)^2) = 210 KB of rows and T: INGVIO_E_CAPACITY,
    while the same window in mono, 93 KB, is accepted) and a window clone beyond the live state (INGVIO_E_NOT_IN_STATE); the state unchanged.
    The worst-case m beyond ingvio_mld and more columns than the context holds cannot be produced: the context sizes mld and its column
    capacity as at least 6 c_max, and m <= 4 x window, nc = 6 x window with window <= c_max."""
    from ingvio_amd import capi
    from test_landmark_path import spd
    rng = np.random.default_rng(2)
    Cw = 20; n = 21 + 6 * Cw
    P0 = spd(n, rng, 1e-2)
    ctx = capi.Context(batch=1, n_max=160, c_max=21, f_max=8, m_max=64)
    ctx.cov_set(0, P0); ctx.tracks_create(8); ctx.nominal_create(32)
    ctx.nominal_set(0, [synthetic_table(Cw)])
    t0 = ctx.nominal_get()[0]
    arr, cap, keep = capi.make_lm_init_blocks([dict(cands=[(0, 0, np.array([1.0, 0.5, 8.0]))], drop=[])])
    stereo, k1 = capi.make_opts(H.opts_frame(True)); mono, k2 = capi.make_opts(H.opts_frame(False))
    assert raw_call(ctx, 0, 1, arr, cap, stereo) == capi.E_CAPACITY
    assert ctx.n(0) == n and np.array_equal(ctx.cov_get(0), P0) and table_equal(t0, ctx.nominal_get()[0])
    assert raw_call(ctx, 0, 1, arr, cap, mono) == capi.OK                                      # (the empty store: skipped on the device)
    assert ctx.n(0) == n and np.array_equal(ctx.cov_get(0), P0) and table_equal(t0, ctx.nominal_get()[0])
    ctx.close()
    Cw = 5; n = 21 + 6 * Cw
    P0 = spd(n, rng, 1e-2)
    ctx = capi.Context(batch=1, n_max=80, c_max=8, f_max=8, m_max=64)
    ctx.cov_set(0, P0); ctx.tracks_create(8); ctx.nominal_create(32)
    ctx.nominal_set(0, [synthetic_table(Cw, idx_shift=6)])                                    # the last clone's columns lie behind the live n
    t0 = ctx.nominal_get()[0]
    assert raw_call(ctx, 0, 1, arr, cap, stereo) == capi.E_NOT_IN_STATE
    assert ctx.n(0) == n and np.array_equal(ctx.cov_get(0), P0) and table_equal(t0, ctx.nominal_get()[0])
    ctx.close()


_loop = {}


def closed_loop_runs():
    """two frames, the call, one more frame, three times: the host loop (rows and table on the host, ingvio_add_variable_delayed), the
    device loop with every stage synchronous, and the device loop whose stage behind the call is asynchronous (copy stream)"""
    if _loop:
        return _loop
    import copy
    from ingvio_amd import capi, synth
    from ingvio_amd.closed_loop import host_step, make_loop, nominal_stage, stage_args
    F, TR = 24, 3
    cases = make_loop(2, 3, F=F, n_landmarks=0)
    n_max = ((max(c["P"].shape[0] for c in cases) + 9 + 15) // 16) * 16
    of = stage_args(cases)[0]
    tab = synth.chi2_table()

    def ctx_of(table):
        ctx = capi.Context(batch=len(cases), n_max=n_max, c_max=12, f_max=F, m_max=64)
        for b, c in enumerate(cases):
            ctx.cov_set(b, c["P"])
        ctx.tracks_create(F)
        if table:
            ctx.nominal_create(V_MAX)
            ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
        return ctx
    ch = ctx_of(False)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    for f in (0, 1):
        host_step(ch, cases, tabs, f)
    # the store after frame 1: the prior window's clones never observed, frame 0's clone at column C - 1 (after frame 1's drop of column 1),
    # frame 1's at column C; the clone frame 1 marginalised still holds column 1 - the drop the NEXT frame's delta carries
    blocks, href = [], []
    n0 = [ch.n(b) for b in range(len(cases))]
    for b, (c, t) in enumerate(zip(cases, tabs)):
        drop = list(c["frames"][2]["delta"]["drop"])
        Cw = len(t.clones)
        pf = np.array(c["frames"][0]["delta"]["pf"][TR])
        obs = [(Cw - 2, c["frames"][0]["delta"]["obs_uv"][TR]), (Cw - 1, c["frames"][1]["delta"]["obs_uv"][TR])]
        blocks.append(dict(cands=[(TR, Cw - 1, pf)], drop=drop))
        cR, cp, cidx = H.window_of(t)
        H_old, H_new, r = H.numpy_rows(cR, cp, pf, Cw - 1, obs, bool(of["stereo"]))
        m = H_old.shape[0]
        added, dxh, chi2h, idxh = ch.add_variable_delayed(b, cidx, [6] * Cw, H_old, H_new, r, of["noise"], 1.0, True, tab[m])
        assert added and idxh == n0[b] and abs(chi2h - tab[m]) > 0.02 * tab[m] and m == 8
        slot = H.free_slots(t)[0]
        H.enter_landmark(t, slot, idxh, Cw - 1, pf)
        t.box_plus(dxh)
        href.append(dict(chi2=chi2h, dx=dxh, slot=slot))
    hcases = copy.deepcopy(cases)
    for b in range(len(cases)):
        hcases[b]["frames"][2]["new_idx"] = n0[b] + 3                      # the host loop's clone goes behind the landmark
    fr_h = host_step(ch, hcases, tabs, 2)
    dev = {}
    for name, use_async in (("serial", False), ("pipelined", True)):
        cd = ctx_of(True)
        for f in (0, 1):
            nominal_stage(cd, cases, f)()
            cd.frame_run()
            cd.frame_fetch()
        got = cd.landmark_init_nominal(0, blocks, of)
        nominal_stage(cd, cases, 2, use_async=use_async)()                 # no nominal_get / _set in between
        cd.frame_run()
        fr = cd.frame_fetch()
        dev[name] = dict(got=got, frame=fr, table=cd.nominal_get(), P=[cd.cov_get(b) for b in range(len(cases))])
        cd.close()
    _loop.update(cases=cases, tabs=tabs, href=href, n0=n0, fr_h=fr_h, Ph=[ch.cov_get(b) for b in range(len(cases))], dev=dev)
    ch.close()
    return _loop


@pytest.mark.gpu
def test_in_the_closed_loop():
    """on the store and the table two real frames leave (one pending drop column): equal masks and row counts, values and P to 1e-9"""
    from nominal_helpers import assert_table
    L = closed_loop_runs()
    d = L["dev"]["serial"]
    dxh, acch, rowsh = L["fr_h"]
    dxd, accd, rowsd = d["frame"]
    assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd) and rowsd.min() > 0
    for b, t in enumerate(L["tabs"]):
        g, h = d["got"][b], L["href"][b]
        assert g[0] == [True] and g[1] == [L["n0"][b]] and g[4] == [h["slot"]]
        assert abs(g[2][0] - h["chi2"]) <= 1e-9 * max(1.0, h["chi2"]) and rel_err(g[3][0], h["dx"]) < 1e-9
        assert rel_err(dxd[b], dxh[b]) < 1e-9 and rel_err(d["P"][b], L["Ph"][b]) < 1e-9
        assert_table(d["table"][b], t, 1e-9, "after the frame behind the initialisation")


@pytest.mark.gpu
def test_asynchronous_stage_behind_the_call_sees_the_new_table():
    """pipelined equals serial bit for bit: the stage on the copy stream waits for the table event the call records"""
    L = closed_loop_runs()
    s, p = L["dev"]["serial"], L["dev"]["pipelined"]
    for b in range(len(L["tabs"])):
        assert s["got"][b][:3] == p["got"][b][:3] and np.array_equal(s["got"][b][3][0], p["got"][b][3][0])
        assert np.array_equal(s["P"][b], p["P"][b]) and table_equal(s["table"][b], p["table"][b])
    for x, y in zip(s["frame"], p["frame"]):
        assert np.array_equal(x, y)
