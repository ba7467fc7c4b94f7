"""In-state SLAM landmarks in the device-resident closed loop (include/ingvio_hip.h: ingvio_landmark_stage_nominal).

The landmark update's inputs - extended pose, extrinsics, landmark positions and every Type::idx() - come from the device nominal table
at the moment the rows are formed; only the observations travel.  Stand-alone form against the host-fed stage (bit for bit) and against
the C oracle; the in-frame form against a host reference loop in the reference's order (IngvioFilter.cpp:277-324: MSCKF update ->
boxPlus -> landmark rows at the updated values -> gates -> stacked update -> boxPlus -> marginalisation), harness in
ingvio_amd/closed_loop_lm.py."""
import copy

import numpy as np
import pytest

from conftest import rel_err as rel
from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_lm as clm
from ingvio_amd.closed_loop import LM, SE23, SE3, VEC3, HostTable
from nominal_helpers import assert_table, device_state, same_state
from nominal_helpers import refused as refused_on
from nominal_helpers import table_ctx as fresh

pytestmark = pytest.mark.gpu

L_LOOP = 6


def same_results(o0, o1, cases):
    for f, ((fa, la), (fb, lb)) in enumerate(zip(o0, o1)):
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[2], fb[2]), f
        for i, c in enumerate(cases):                                    # accept flags exist for the frame's features only
            nf = len(c["frames"][f]["delta"]["feat_track"])
            assert np.array_equal(fa[1][i, :nf], fb[1][i, :nf]), (f, i)
        for x, y in zip(la, lb):
            assert np.array_equal(x, y), f


# ---- 1. / 2. the stand-alone form ----------------------------------------------------------------------------------------------
def rot(rng, mag=1.0):
    from oracle import oracle as orc
    return orc.gamma(mag * rng.standard_normal(3), 0).reshape(3, 3)


def spd(n, rng, scale=1.0):
    A = rng.standard_normal((n, n))
    return scale * (A @ A.T / n + 0.1 * np.eye(n))


def make_filter(rng, C, L, hole, outliers=(), untracked=()):
    """a table [pose | bg | ba | ext | C clones | (a free slot) | L landmarks in view of the camera, anchored to different clones] with
    its prior, the observations of the landmarks and the stereo extrinsics"""
    slots = []
    idx = [0]

    def add(kind, size, R=None, p=None, anchor=-1):
        slots.append(dict(kind=kind, idx=idx[0], anchor=anchor, R=np.eye(3) if R is None else R, p=np.zeros(3) if p is None else p,
                          v=0.1 * rng.standard_normal(3) if kind == SE23 else np.zeros(3)))
        idx[0] += size
        return len(slots) - 1
    R_i2w, p_i2w = rot(rng, 0.3), rng.standard_normal(3)
    R_cl2i, p_c2i = rot(rng, 0.05), 0.05 * rng.standard_normal(3)
    v_pose = add(SE23, 9, R_i2w, p_i2w)
    v_bg, v_ba = add(VEC3, 3, p=0.01 * rng.standard_normal(3)), add(VEC3, 3, p=0.01 * rng.standard_normal(3))
    v_ext = add(SE3, 6, R_cl2i, p_c2i)
    clones = [add(SE3, 6, rot(rng, 0.3), rng.standard_normal(3)) for _ in range(C)]
    if hole:
        slots.append(None)
    Rlr, tlr = rot(rng, 0.01), np.array([-0.11, 0.002, 0.001])
    uv, lm = np.zeros((L, 4)), []
    for l in range(L):
        q = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 9.0)])      # in the left camera
        lm.append(add(LM, 3, p=R_i2w @ (R_cl2i @ q + p_c2i) + p_i2w, anchor=clones[int(rng.integers(0, C))]))
        qr = Rlr @ q + tlr
        uv[l] = [q[0] / q[2], q[1] / q[2], qr[0] / qr[2], qr[1] / qr[2]]
        uv[l] += 0.01 * rng.standard_normal(4) * (30.0 if l in outliers else 1.0)
    tracked = np.ones(L, dtype=np.uint8)
    for l in untracked:
        tracked[l] = 0
    table = HostTable(slots, clones, v_ext, v_pose, v_bg, v_ba, [0.0, 0.0, -9.8])
    return dict(table=table, P=spd(idx[0], rng, 1e-3), lm_slots=lm, uv=uv, tracked=tracked, Rlr=Rlr, tlr=tlr)


def standalone_batch(stereo, L=9, C=5):
    """filter 0 plain, 1 not staged (n_lm = 0), 2 with an untracked landmark, 3 with a free slot below the landmarks and a subset staged
    in another order"""
    rng = np.random.default_rng(2100 + L + (1 if stereo else 0))
    flt = [make_filter(rng, C + b, L, hole=(b == 3), outliers=(1, 5), untracked=(2,) if b == 2 else ()) for b in range(4)]
    for f in flt[1:]:
        f["Rlr"], f["tlr"] = flt[0]["Rlr"], flt[0]["tlr"]
    staged = []
    for b, f in enumerate(flt):
        if b == 1:
            staged.append(None)
        elif b == 3:
            order = [4, 0, 7, 2, 5]
            staged.append(dict(lm_var=[f["lm_slots"][l] for l in order], uv=f["uv"][order], tracked=f["tracked"][order]))
        else:
            staged.append(dict(lm_var=f["lm_slots"], uv=f["uv"], tracked=f["tracked"]))
    return flt, staged


def standalone_ctx(flt, with_table=True):
    from ingvio_amd import capi
    n_max = max(f["P"].shape[0] for f in flt) + 6
    ctx = capi.Context(batch=len(flt), n_max=((n_max + 15) // 16) * 16, c_max=max(len(f["table"].clones) for f in flt) + 1, f_max=8, m_max=64)
    for b, f in enumerate(flt):
        ctx.cov_set(b, f["P"])
    if with_table:
        ctx.nominal_create(96)
        ctx.nominal_set(0, [f["table"].as_dict() for f in flt])
    return ctx


# (True, 60, 10): states of 267 ... 285 rows, beyond the fused landmark front (256 rows) - the k_lm_build route
@pytest.mark.parametrize("stereo,L,C", [(True, 9, 5), (False, 9, 5), (True, 60, 10)])
def test_standalone_equals_host_fed_stage_bit_for_bit(stereo, L, C):
    flt, staged = standalone_batch(stereo, L, C)
    B = len(flt)
    thr = clm.CHI2_4 if stereo else clm.CHI2_2
    cd, ch = standalone_ctx(flt), standalone_ctx(flt, with_table=False)
    nom = cd.nominal_get()
    cd.landmark_stage_nominal(0, staged, stereo, 0.02, thr, flt[0]["Rlr"], flt[0]["tlr"])
    cd.landmark_run()
    rd = cd.landmark_fetch()
    ch.landmark_stage(0, clm.staged_frames(nom, staged), stereo, 0.02, thr, flt[0]["Rlr"], flt[0]["tlr"])
    ch.landmark_run()
    rh = ch.landmark_fetch()
    for name, x, y in zip(("dx", "rows", "accept", "gamma", "status"), rd, rh):
        assert np.array_equal(x, y), name
    assert not rd[4].any()
    assert rd[1][1] == 0 and not rd[0][1].any()                          # the filter that staged nothing
    assert rd[1][0] > 0 and rd[1][2] > 0 and rd[1][3] > 0
    assert rd[3][2, 2] == -1.0                                           # the untracked landmark
    for b in range(B):
        assert np.array_equal(cd.cov_get(b), ch.cov_get(b)), b
    got = cd.nominal_get()                                               # the run ended with boxPlus of its dx on the table
    for b, f in enumerate(flt):
        t = copy.deepcopy(f["table"])
        t.box_plus(rd[0][b])
        assert_table(got[b], t, 1e-13, b)
    assert any(rel(got[b]["val"], nom[b]["val"]) > 1e-9 for b in range(B))
    cd.close(); ch.close()


def oracle_update(P0, fr, stereo, noise, thr, Rlr, tlr):
    from oracle import oracle as orc
    per = 4 if stereo else 2
    n = P0.shape[0]
    ie, ix = fr["idx_epose"], fr["idx_ext"]
    rows, res, acc, gam = [], [], [], []
    for l, (il, ia) in enumerate(zip(fr["lm_idx"], fr["anchor_idx"])):
        if not fr["tracked"][l]:
            acc.append(0); gam.append(-1.0); continue
        H, r = orc.landmark_rows_epose(fr["R_i2w"], fr["p_i2w"], fr["R_cl2i"], fr["p_c2i"], fr["pf"][l], fr["uv"][l], stereo, Rlr, tlr)
        Hd = np.zeros((per, n))
        Hd[:, ie:ie + 9] += H[:per, 0:9]; Hd[:, ix:ix + 6] += H[:per, 9:15]; Hd[:, ia:ia + 6] += H[:per, 15:21]; Hd[:, il:il + 3] += H[:per, 21:24]
        S = Hd @ P0 @ Hd.T + noise ** 2 * np.eye(per)
        g = float(r[:per] @ np.linalg.solve(S, r[:per]))
        gam.append(g)
        if g < thr:
            acc.append(1); rows.append(Hd); res.append(r[:per])
        else:
            acc.append(0)
    oc = orc.Cov(P0)
    dx = np.zeros(n)
    if rows:
        dx, _ = oc.ekf_update([0], [n], np.vstack(rows), np.concatenate(res), noise ** 2)
    return oc.P, dx, np.array(acc), np.array(gam), per * int(np.sum(acc))


@pytest.mark.parametrize("stereo,L,C", [(True, 9, 5), (False, 9, 5), (True, 60, 10)])
def test_standalone_against_the_oracle(stereo, L, C):
    flt, staged = standalone_batch(stereo, L, C)
    thr = clm.CHI2_4 if stereo else clm.CHI2_2
    cd = standalone_ctx(flt)
    cd.landmark_stage_nominal(0, staged, stereo, 0.02, thr, flt[0]["Rlr"], flt[0]["tlr"])
    cd.landmark_run()
    dx, rows, acc, gam, st = cd.landmark_fetch()
    assert not st.any()
    frames = clm.staged_frames([f["table"].as_dict() for f in flt], staged)
    seen = set()
    for b, (f, fr) in enumerate(zip(flt, frames)):
        n, nl = f["P"].shape[0], len(fr["lm_idx"])
        Pw, dxw, accw, gamw, mw = oracle_update(f["P"], fr, stereo, 0.02, thr, f["Rlr"], f["tlr"])
        if nl:
            assert np.array_equal(acc[b, :nl], accw), b
            on = gamw >= 0
            assert np.allclose(gam[b, :nl][on], gamw[on], rtol=1e-9, atol=1e-12) and (gam[b, :nl][~on] == -1).all(), b
            seen |= set(accw[on].tolist())
        assert rows[b] == mw, b
        P = cd.cov_get(b)
        assert np.linalg.norm(P - Pw) < 1e-9 * np.linalg.norm(Pw) and np.array_equal(P, P.T), b
        assert np.linalg.norm(dx[b, :n] - dxw) < 1e-8 * max(1e-6, np.linalg.norm(dxw)), b
    assert seen == {0, 1}                                                # both verdicts occurred
    cd.close()


# ---- 3. - 6. the closed loop ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lm_cases():
    return clm.make_lm_loop(24, 13, L=L_LOOP)


def device_frame(ctx, cases, f, opts):
    cl.nominal_stage(ctx, cases, f)()
    clm.lm_stage_call(ctx, cases, f, opts)()
    ctx.frame_run()
    return ctx.frame_fetch(), ctx.landmark_fetch()


def test_closed_loop_device_equals_host_reference(lm_cases):
    cases, opts = lm_cases, clm.lm_opts()
    B, F, L = len(cases), 24, L_LOOP
    ch, cd = cl.loop_ctx(cases, F), fresh(cases)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    refused, accepted = np.zeros(B, dtype=int), np.zeros(B, dtype=int)
    worst_t = worst_p = 0.0
    near = np.inf
    for f in range(len(cases[0]["frames"])):
        (dxh, acch, rowsh), (ldxh, lrowsh, lacch, lgamh, lsth) = clm.host_step_lm(ch, cases, tabs, f, opts)
        (dxd, accd, rowsd), (ldxd, lrowsd, laccd, lgamd, lstd) = device_frame(cd, cases, f, opts)
        # the comparison is not empty: asserted on the HOST REFERENCE LOOP's results
        assert not lsth.any(), f
        trk = np.stack([c["frames"][f]["lm_tracked"] for c in cases]) != 0
        g = lgamh[:, :L][trk]
        near = min(near, float(np.min(np.abs(g - opts["chi2_thr"]) / opts["chi2_thr"])))
        refused += ((lacch[:, :L] == 0) & trk).sum(axis=1)
        accepted += (lacch[:, :L] == 1).sum(axis=1)
        print("frame %2d  reference: msckf rows %s  landmark rows min %d  refused %d  gamma margin %.3e" %
              (f, (int(rowsh.min()), int(rowsh.max())), int(lrowsh.min()), int(((lacch[:, :L] == 0) & trk).sum()), near))
        if f >= 2:
            assert (lrowsh >= 4 * (L - 3)).all(), (f, lrowsh)
            assert rowsh.sum() > 0, f
        # device form against the reference
        assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd), f
        assert np.array_equal(lacch, laccd) and np.array_equal(lrowsh, lrowsd), f
        nom, Ps = device_state(cd, B)
        for b in range(B):
            worst_t = max(worst_t, assert_table(nom[b], tabs[b], 1e-9, (f, b)))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape, (f, b)
            worst_p = max(worst_p, rel(Ps[b], Ph))
            assert rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
    print("worst table value %.3e  worst P %.3e  smallest gamma margin %.3e" % (worst_t, worst_p, near))
    assert (refused >= 1).all() and (accepted >= 1).all(), (refused, accepted)
    assert near > 1e-6, near
    ch.close(); cd.close()


def test_landmark_rows_are_formed_after_the_msckf_boxplus(lm_cases):
    """One frame three ways: the device in-frame form, the host reference loop (rows at the values after the MSCKF update's boxPlus) and
    the host-fed in-frame stage (rows at the values before it).  The device form must follow the reference, and the two orders must be
    told apart by far more than the tolerance."""
    cases, opts = lm_cases, clm.lm_opts()
    B, F, f0 = len(cases), 24, 4
    ch, cp, cd = cl.loop_ctx(cases, F), cl.loop_ctx(cases, F), fresh(cases)
    tabs_h = [copy.deepcopy(c["table"]) for c in cases]
    tabs_p = [copy.deepcopy(c["table"]) for c in cases]
    for f in range(f0):
        clm.host_step_lm(ch, cases, tabs_h, f, opts)
        clm.host_step_lm(cp, cases, tabs_p, f, opts)
        device_frame(cd, cases, f, opts)
    (dxh, _, rowsh), lmh = clm.host_step_lm(ch, cases, tabs_h, f0, opts)
    _, lmp = clm.host_step_lm_prestaged(cp, cases, tabs_p, f0, opts)
    _, lmd = device_frame(cd, cases, f0, opts)
    for b in range(B):
        n = cases[b]["frames"][f0]["new_idx"] + 6
        move = float(np.linalg.norm(dxh[b, 0:9]))                       # the reference's MSCKF correction of the extended pose
        agree, differ = rel(lmd[0][b, :n], lmh[0][b, :n]), rel(lmp[0][b, :n], lmh[0][b, :n])
        print("filter %2d  msckf rows %3d  |dx pose| %.3e  device vs reference %.3e  pre-update vs reference %.3e" %
              (b, rowsh[b], move, agree, differ))
        assert rowsh[b] > 0 and move >= 1e-5, (b, move)
        assert lmh[1][b] > 0
        assert agree <= 1e-9, (b, agree)
        assert differ >= 1e-6, (b, differ)
        assert rel(lmd[0][b, :n], lmp[0][b, :n]) >= 1e-6, b
    ch.close(); cp.close(); cd.close()


def test_pipelined_loop_equals_serial_loop(lm_cases):
    cases, opts = lm_cases, clm.lm_opts()
    B = len(cases)
    res = []
    for pipelined in (False, True):
        ctx = fresh(cases)
        out = clm.device_loop_lm(ctx, cases, list(range(len(cases[0]["frames"]))), opts, pipelined)
        res.append((out, device_state(ctx, B)))
        ctx.close()
    (o0, s0), (o1, s1) = res
    for f, ((fa, la), (fb, lb)) in enumerate(zip(o0, o1)):
        for x, y in zip(fa + la, fb + lb):
            assert np.array_equal(x, y), f
    same_state(s0, s1)
    assert sum(int(la[1].sum()) for _, la in o0) > 0


def test_snapshot_restore_replays_bit_for_bit(lm_cases):
    cases, opts = lm_cases, clm.lm_opts()
    B, F, N = len(cases), 24, 6
    ctx = fresh(cases)
    ctx.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            ctx.restore()
            ctx.tracks_create(F)                                         # the track store is not part of the snapshot
        out = clm.device_loop_lm(ctx, cases, list(range(N)), opts, False)
        runs.append((out, device_state(ctx, B)))
    same_results(runs[0][0], runs[1][0], cases)
    same_state(runs[0][1], runs[1][1], keys=("kind", "idx", "val", "clone_var"))
    ctx.close()


def test_frames_without_a_landmark_stage_run_as_before(lm_cases):
    """a landmark stage belongs to one frame: the frames after it take the plain path of tests/test_gpu_nominal_state.py"""
    cases, opts = lm_cases, clm.lm_opts()
    B, F, N = len(cases), 24, 5
    plain = fresh(cases)
    want = cl.device_loop(plain, cases, list(range(N)), False)
    want_state = device_state(plain, B)
    plain.close()
    ctx = fresh(cases)
    ctx.snapshot()
    device_frame(ctx, cases, 0, opts)
    ctx.restore()
    ctx.tracks_create(F)
    got = cl.device_loop(ctx, cases, list(range(N)), False)
    for f, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), f
        for i, c in enumerate(cases):
            nf = len(c["frames"][f]["delta"]["feat_track"])
            assert np.array_equal(a[1][i, :nf], b[1][i, :nf]), (f, i)
    same_state(want_state, device_state(ctx, B), keys=("kind", "idx", "val", "clone_var"))
    ctx.close()
    # without a restore in between: frame 0 with the stage, frame 1 without, against the host loops of the same order
    ch, cd = cl.loop_ctx(cases, F), fresh(cases)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    clm.host_step_lm(ch, cases, tabs, 0, opts)
    device_frame(cd, cases, 0, opts)
    lm0 = cd.landmark_fetch()
    dxh, acch, rowsh = cl.host_step(ch, cases, tabs, 1)
    cl.nominal_stage(cd, cases, 1)()
    cd.frame_run()
    dxd, accd, rowsd = cd.frame_fetch()
    assert np.array_equal(rowsh, rowsd)
    for x, y in zip(lm0, cd.landmark_fetch()):                           # no landmark update ran in frame 1
        assert np.array_equal(x, y)
    nom, Ps = device_state(cd, B)
    for b in range(B):
        assert_table(nom[b], tabs[b], 1e-9, b)
        assert rel(Ps[b], ch.cov_get(b)) <= 1e-9, b
    ch.close(); cd.close()


def test_refusals_leave_the_state_unchanged(lm_cases):
    from ingvio_amd import capi
    cases, opts = lm_cases[:4], clm.lm_opts()
    B, F, L = len(cases), 24, L_LOOP
    tabs = [c["table"].as_dict() for c in cases]
    ctx = cl.loop_ctx(cases, F)

    def state():
        return device_state(ctx, B), [ctx.n(b) for b in range(B)]

    def refused(fn, code):
        refused_on(ctx, fn, code, sizes=True)

    def stage(frames, in_frame, b0=0):
        return ctx.landmark_stage_nominal_prepare(b0, frames, opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"], opts["t_cl2cr"],
                                                  in_frame=in_frame)
    good = clm.nominal_frames(cases, 0)

    def bad(b, **kw):
        fr = [dict(g) for g in good]
        fr[b].update(kw)
        return fr
    with pytest.raises(capi.IngvioError) as e:                           # no table
        stage(good, False)()
    assert e.value.code == capi.E_ARG
    ctx.nominal_create(48)
    ctx.nominal_set(0, tabs)
    sl, sl2, sl3 = cases[1]["lm_slots"], cases[2]["lm_slots"], cases[3]["lm_slots"]
    refused(stage(bad(1, lm_var=[sl[0], 47] + sl[2:]), False), capi.E_ARG)              # a free slot
    refused(stage(bad(1, lm_var=[sl[0], tabs[1]["v_pose"]] + sl[2:]), False), capi.E_ARG)      # not a landmark
    refused(stage(bad(2, lm_var=[sl2[0], sl2[0]] + sl2[2:]), False), capi.E_ARG)        # a duplicate
    refused(stage(bad(0, lm_var=[cases[0]["lm_slots"][0]] * 65, uv=np.zeros((65, 4)), tracked=np.ones(65, dtype=np.uint8)), False), capi.E_CAPACITY)
    refused(stage(good, True), capi.E_ARG)                               # in-frame without a pending frame from the table
    # a stand-alone stage that has not run: what moves the table or the bookkeeping is refused, as for a pending GNSS epoch
    stage(good, False)()
    refused(cl.nominal_stage(ctx, cases, 0), capi.E_ARG)
    refused(lambda: ctx.nominal_set(0, tabs), capi.E_ARG)
    refused(lambda: ctx.nominal_box_plus(0, np.zeros((B, ctx.ldp))), capi.E_ARG)
    refused(lambda: ctx.nominal_set_gnss(0, [[-1] * 6] * B), capi.E_ARG)
    refused(lambda: ctx.snapshot(), capi.E_ARG)
    refused(lambda: ctx.landmark_run(1, B - 1), capi.E_ARG)              # another range than the staged one
    ctx.landmark_run()
    ctx.landmark_fetch()
    refused(lambda: ctx.landmark_run(), capi.E_ARG)                      # a second run
    ctx.close()

    # a restore abandons either form
    ctx = fresh(cases)
    ctx.snapshot()
    s0 = state()
    stage(good, False)()
    ctx.restore()
    refused(lambda: ctx.landmark_run(0, B), capi.E_ARG)
    cl.nominal_stage(ctx, cases, 0)()
    stage(good, True)()
    ctx.restore()
    ctx.tracks_create(F)
    s1 = state()
    same_state(s0[0], s1[0])
    refused(lambda: ctx.landmark_run(0, B), capi.E_ARG)

    # with a frame staged from the table and not yet run
    cl.nominal_stage(ctx, cases, 0)()
    refused(stage(good, False), capi.E_ARG)                              # the stand-alone form
    refused(stage(good[1:], True, b0=1), capi.E_ARG)                     # the in-frame form is the whole batch's
    refused(stage(good[:B - 1], True), capi.E_ARG)
    refused(stage(bad(3, lm_var=[sl3[1], sl3[1]] + sl3[2:]), True), capi.E_ARG)
    # the host-fed in-frame stage stays refused with a frame from the table
    nom = ctx.nominal_get()
    ctx.landmark_stage(0, clm.table_frames(nom, cases, 0), opts["stereo"], opts["noise"], opts["chi2_thr"], opts["R_cl2cr"], opts["t_cl2cr"],
                       in_frame=True)
    refused(lambda: ctx.frame_run(), capi.E_UNSUPPORTED)
    stage(good, True)()                                                  # replaces it
    refused(lambda: ctx.landmark_run(0, B), capi.E_ARG)                  # the frame's run applies it
    ctx.frame_run()
    got = [(ctx.frame_fetch(), ctx.landmark_fetch())]
    refused(lambda: ctx.frame_run(), capi.E_ARG)                         # consumed with the frame
    refused(stage(good, True), capi.E_ARG)
    for f in (1, 2):
        got.append(device_frame(ctx, cases, f, opts))
    got_state = device_state(ctx, B)
    ctx.close()
    # the valid frames give what they give without the refused calls
    ctx = fresh(cases)
    want = [device_frame(ctx, cases, f, opts) for f in range(3)]
    same_results(want, got, cases)
    same_state(device_state(ctx, B), got_state)
    ctx.close()

    # a table without extrinsics
    ctx = cl.loop_ctx(cases, F)
    ctx.nominal_create(48)
    ctx.nominal_set(0, [dict(t, v_ext=-1) for t in tabs])
    refused(stage(good, False), capi.E_ARG)
    ctx.close()
