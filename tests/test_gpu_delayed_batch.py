"""ingvio_add_variable_delayed_batch (kernels_delayed.hip): StateManager::addVariableDelayed for a batch of filters with several
candidates each, the verdicts taken on the device, against the C oracle called filter by filter and candidate by candidate
(oracle.Cov.add_variable_delayed).  Rows are built as tests/test_landmark_path.py::test_gpu_add_variable_delayed builds them;
tolerances are that test's.  Every test asserts on the oracle's own chi2 that no candidate lies within 2 % of its gate."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from test_landmark_path import spd

NOISE = 0.1
WINDOWS = (3, 5, 8, 11, 11, 12, 16)
STEREO = (True, False, True, False, True, False, True)
SUBSET = {2: (0, 2, 3, 5, 7), 5: (1, 2, 4, 5, 6, 8, 9, 11)}       # filters whose var_old_order is a strict subset of the window


def chi2_check(m):
    from scipy.stats import chi2
    return float(chi2.ppf(0.95, m))


def make_cand(rng, vidx, vsize, m, s, res=None):
    nc = int(np.sum(vsize))
    return (list(vidx), list(vsize), rng.standard_normal((m, nc)), rng.standard_normal((m, s)),
            0.05 * rng.standard_normal(m) if res is None else res, chi2_check(m))


def oracle_run(P0, cands, chi2_mult=1.0, do_chi2=True):
    """the reference's loop for one filter -> (Cov, added[], new_idx[], chi2[], dx[])"""
    c = orc.Cov(P0)
    added, idx, chi2, dxs = [], [], [], []
    for vidx, vsize, H_old, H_new, res, chk in cands:
        m, s = H_new.shape
        if m <= s:
            a, dx, g = False, None, 0.0
        else:
            n0 = c.n
            a, dx, g = c.add_variable_delayed(vidx, vsize, H_old, H_new, res, NOISE, chi2_mult, do_chi2, chk)
            assert abs(g - chi2_mult * chk) > 0.02 * chi2_mult * chk, "a candidate within 2 % of its gate: change the seed"
        added.append(a); idx.append(n0 if a else -1); chi2.append(g); dxs.append(dx if a else None)
    return c, added, idx, chi2, dxs


def compare(ctx, b, got, ref):
    """one filter's results of the batch call against oracle_run's"""
    c, added, idx, chi2, dxs = ref
    ga, gi, gc, gd = got
    assert ga == added and gi == idx, (b, ga, added, gi, idx)
    for j in range(len(added)):
        assert abs(gc[j] - chi2[j]) <= 1e-9 * max(1.0, chi2[j]), (b, j, gc[j], chi2[j])
        if added[j]:
            assert np.linalg.norm(gd[j] - dxs[j]) < 1e-9 * max(1.0, np.linalg.norm(dxs[j])), (b, j)
        else:
            assert gd[j] is None
    assert ctx.n(b) == c.n
    Pg = ctx.cov_get(b)
    assert np.linalg.norm(Pg - c.P) / np.linalg.norm(c.P) < 1e-11, b
    assert np.array_equal(Pg, Pg.T)


def mixed_batch():
    rng = np.random.default_rng(2024)
    priors, blocks = [], []
    for b, (Cw, st) in enumerate(zip(WINDOWS, STEREO)):
        n = 21 + 6 * Cw
        priors.append(spd(n, rng, 1e-2))
        clones = SUBSET.get(b, range(Cw))
        vidx = [21 + 6 * i for i in clones]
        blocks.append([make_cand(rng, vidx, [6] * len(vidx), (4 if st else 2) * Cw, 3)])
    return priors, blocks


def new_ctx(priors, batch=None, m_max=96, extra=16):
    from ingvio_amd import capi
    n = max(P.shape[0] for P in priors)
    ctx = capi.Context(batch=batch or len(priors), n_max=((n + 15) // 16) * 16 + extra, c_max=16, f_max=32, m_max=m_max)
    return ctx


_cache = {}


def mixed_reference():
    """the mixed batch, its oracle results and the device's (one run, shared)"""
    if "mixed" not in _cache:
        priors, blocks = mixed_batch()
        ref = [oracle_run(P, cs) for P, cs in zip(priors, blocks)]
        ctx = new_ctx(priors)
        for b, P in enumerate(priors):
            ctx.cov_set(b, P)
        got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
        Ps = [ctx.cov_get(b) for b in range(len(priors))]
        _cache["mixed"] = (priors, blocks, ref, ctx, got, Ps)
    return _cache["mixed"]


@pytest.mark.gpu
def test_mixed_batch_one_candidate_each():
    priors, blocks, ref, ctx, got, Ps = mixed_reference()
    for b in range(len(priors)):
        assert ref[b][1] == [True] and ref[b][2] == [priors[b].shape[0]]
        compare(ctx, b, got[b], ref[b])
    assert list(ctx.delayed_status) == [0] * len(priors)


@pytest.mark.gpu
def test_verdicts():
    priors, blocks, ref, _, got1, Ps1 = mixed_reference()
    blocks = [list(cs) for cs in blocks]
    v, s1, h1, r1, chk = blocks[1][0][0], blocks[1][0][1], blocks[1][0][2], blocks[1][0][3], blocks[1][0][5]
    blocks[1] = [(v, s1, h1, r1, 50.0 * np.ones(h1.shape[0]), chk)]                              # refused by the gate
    v, s3, h3, r3 = blocks[3][0][:4]
    blocks[3] = [(v, s3, h3[:3], r3[:3], blocks[3][0][4][:3], chi2_check(3))]                    # m == s: skipped
    blocks[4] = []                                                                                # nothing for this filter
    quiet = (1, 3, 4)
    assert oracle_run(priors[1], blocks[1])[1] == [False]
    ctx = new_ctx(priors)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    before = [ctx.cov_get(b) for b in range(len(priors))]
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    for b in range(len(priors)):
        if b in quiet:
            assert got[b][0] == [False] * len(blocks[b]) and got[b][1] == [-1] * len(blocks[b]) and all(d is None for d in got[b][3])
            assert ctx.n(b) == priors[b].shape[0] and np.array_equal(ctx.cov_get(b), before[b])
        else:                                                                                     # bit for bit what the first test got
            assert got[b][:3] == got1[b][:3] and np.array_equal(got[b][3][0], got1[b][3][0])
            assert np.array_equal(ctx.cov_get(b), Ps1[b])
    assert got[1][2][0] > chk and got[3][2] == [0.0]
    # the refused filter alone, the gate off: added
    ref = oracle_run(priors[1], blocks[1], do_chi2=False)
    got = ctx.add_variable_delayed_batch(1, [blocks[1]], NOISE, do_chi2=False)
    assert ref[1] == [True]
    compare(ctx, 1, got[0], ref)
    ctx.close()


@pytest.mark.gpu
def test_sequences():
    rng = np.random.default_rng(77)
    Cs = (6, 9, 11, 4)
    priors, blocks = [], []
    for b, Cw in enumerate(Cs):
        n = 21 + 6 * Cw
        priors.append(spd(n, rng, 1e-2))
        vidx = [21 + 6 * i for i in range(Cw)]
        cands = [make_cand(rng, vidx, [6] * Cw, (4 if b % 2 == 0 else 2) * Cw, 3) for _ in range(3)]
        if b in (1, 2):                                                                           # the middle candidate is refused
            v, s, h, r, _, chk = cands[1]
            cands[1] = (v, s, h, r, 50.0 * np.ones(h.shape[0]), chk)
        if b == 3:
            cands[1] = make_cand(rng, [0], [9], 5, 1)                                             # a GNSS scalar on the extended pose
        blocks.append(cands)
    ref = [oracle_run(P, cs) for P, cs in zip(priors, blocks)]
    assert [r[1] for r in ref] == [[True] * 3, [True, False, True], [True, False, True], [True] * 3]
    n0 = [P.shape[0] for P in priors]
    assert ref[0][2] == [n0[0], n0[0] + 3, n0[0] + 6] and ref[1][2] == [n0[1], -1, n0[1] + 3] and ref[3][2] == [n0[3], n0[3] + 3, n0[3] + 4]
    ctx = new_ctx(priors)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    for b in range(len(priors)):
        compare(ctx, b, got[b], ref[b])
    # the host mirror knows the new sizes: an update on a new landmark's columns is accepted
    for b in (0, 1):
        li = got[b][1][2]
        H = rng.standard_normal((2, 9)); r = 0.01 * rng.standard_normal(2)
        dxo, _ = ref[b][0].ekf_update([21, li], [6, 3], H, r, 0.01)
        dxg, _ = ctx.ekf_update(b, [21, li], [6, 3], H, r, 0.01)
        assert np.linalg.norm(dxg - dxo) < 1e-9 * max(1.0, np.linalg.norm(dxo))
        assert np.linalg.norm(ctx.cov_get(b) - ref[b][0].P) / np.linalg.norm(ref[b][0].P) < 1e-11
    ctx.close()


@pytest.mark.gpu
def test_partial_range():
    rng = np.random.default_rng(31)
    Cw = 5; n = 21 + 6 * Cw
    priors = [spd(n, rng, 1e-2) for _ in range(8)]
    vidx = [21 + 6 * i for i in range(Cw)]
    blocks = [[make_cand(rng, vidx, [6] * Cw, 4 * Cw, 3), make_cand(rng, vidx, [6] * Cw, 2 * Cw, 3)] for _ in range(3)]
    ctx = new_ctx(priors)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    before = [ctx.cov_get(b) for b in range(8)]
    got = ctx.add_variable_delayed_batch(2, blocks, NOISE)
    for i in range(3):
        compare(ctx, 2 + i, got[i], oracle_run(priors[2 + i], blocks[i]))
    for b in (0, 1, 5, 6, 7):
        assert ctx.n(b) == n and np.array_equal(ctx.cov_get(b), before[b])
    ctx.close()


def raw_call(ctx, b0, nb, arr, cap):
    added = np.zeros((max(nb, 1), max(cap, 1)), dtype=np.int32); idx = np.zeros_like(added)
    return ctx.L.ingvio_add_variable_delayed_batch(ctx.h, b0, nb, arr, C.c_double(NOISE), C.c_double(1.0), 1, cap,
                                                   added.ctypes.data_as(C.POINTER(C.c_int)), idx.ctypes.data_as(C.POINTER(C.c_int)), None, None, None)


@pytest.mark.gpu
def test_refusals():
    from ingvio_amd import capi
    rng = np.random.default_rng(5)
    Cw = 4; n = 21 + 6 * Cw
    P0 = spd(n, rng, 1e-2)
    ctx = capi.Context(batch=2, n_max=48, c_max=Cw, f_max=16, m_max=64)                           # room for ONE more 3-vector
    ctx.cov_set(0, P0); ctx.cov_set(1, P0)
    vidx, vsize = [21 + 6 * i for i in range(Cw)], [6] * Cw
    good = make_cand(rng, vidx, vsize, 8, 3)

    def code(blocks, b0=0, nb=None, cap=None, edit=None):
        arr, cc, keep = capi.make_delayed_blocks(blocks)
        if edit:
            edit(arr)
        rc = raw_call(ctx, b0, len(blocks) if nb is None else nb, arr, cc if cap is None else cap)
        assert ctx.n(0) == n and ctx.n(1) == n and np.array_equal(ctx.cov_get(0), P0) and np.array_equal(ctx.cov_get(1), P0)
        return rc
    assert code([[good], [good]], b0=1) == capi.E_ARG                                             # range
    assert code([[good]], edit=lambda a: setattr(a[0], "cand", None)) == capi.E_ARG               # NULL where data is needed
    assert code([[good]], edit=lambda a: setattr(a[0].cand[0], "res", None)) == capi.E_ARG
    assert code([[make_cand(rng, vidx, vsize, 12, 7)]]) == capi.E_ARG                             # s outside 1..6
    assert code([[good]], edit=lambda a: setattr(a[0].cand[0], "ldh", 7)) == capi.E_ARG           # ldh < m
    assert code([[good]], edit=lambda a: setattr(a[0].cand[0], "ldn", 7)) == capi.E_ARG
    assert code([[good, good]], cap=1) == capi.E_ARG                                              # n_cand > cand_cap
    assert code([[make_cand(rng, [21, n - 3], [6, 6], 8, 3)]]) == capi.E_NOT_IN_STATE             # beyond h_n[b]
    assert code([[], [good, good]]) == capi.E_CAPACITY                                            # the first alone would fit
    assert code([[make_cand(rng, vidx, vsize, 70, 3)]]) == capi.E_CAPACITY                        # m > mld
    assert code([[make_cand(rng, [21] * 12, [6] * 12, 8, 3)]]) == capi.E_CAPACITY                 # more columns than the context holds
    ctx.close()
    Cb = 21; nb_ = 21 + 6 * Cb
    Pb = spd(nb_, rng, 1e-2)
    big = capi.Context(batch=1, n_max=224, c_max=30, f_max=16, m_max=64)                          # rows up to 6 * 30
    big.cov_set(0, Pb)
    wide = [21 + 6 * i for i in range(Cb)]
    # (the three LDS bounds nest: the trailing update's S implies the gate's 150 KB, which implies the front's 160 KB, so each case
    # names the FIRST bound it breaks; no input breaks an inner bound alone)
    for cand in (make_cand(rng, vidx, vsize, 150, 3),                                             # S of the trailing update beyond LDS
                 make_cand(rng, [0] + wide[:15], [9] + [6] * 15, 103, 3),                         # S fits, the gate's 150 KB bound does not
                 make_cand(rng, wide, [6] * Cb, 4 * Cb, 3)):                                      # both fit, rows and T beyond the front's LDS
        arr, cc, keep = capi.make_delayed_blocks([[cand]])
        assert raw_call(big, 0, 1, arr, cc) == capi.E_CAPACITY and big.n(0) == nb_ and np.array_equal(big.cov_get(0), Pb)
    big.close()


@pytest.mark.gpu
def test_refused_while_a_nominal_frame_is_pending():
    from ingvio_amd import capi
    from ingvio_amd.closed_loop import make_loop, nominal_stage
    from nominal_helpers import refused, table_ctx
    cases = make_loop(2, 2, F=24, n_landmarks=0)
    ctx = table_ctx(cases)
    rng = np.random.default_rng(9)
    blocks = [[make_cand(rng, [0], [9], 8, 3)] for _ in cases]
    nominal_stage(ctx, cases, 0)()
    refused(ctx, lambda: ctx.add_variable_delayed_batch(0, blocks, NOISE), capi.E_ARG, sizes=True)
    ctx.frame_run()
    ctx.frame_fetch()
    tab0 = ctx.nominal_get()
    n0 = [ctx.n(b) for b in range(2)]
    refs = [oracle_run(ctx.cov_get(b), blocks[b]) for b in range(2)]
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    tab1 = ctx.nominal_get()
    for b in range(2):
        assert got[b][0] == [True] and got[b][1] == [n0[b]]
        compare(ctx, b, got[b], refs[b])
        for key in ("kind", "idx", "anchor", "val", "clone_var"):                                 # the call never touches the table
            assert np.array_equal(tab0[b][key], tab1[b][key])
    ctx.close()


@pytest.mark.gpu
def test_with_the_closed_loop():
    """two frames, the batch initialisation, the landmark entered into the device table, boxPlus, one more frame - against a host
    loop that made the same initialisation through the single-filter ingvio_add_variable_delayed"""
    import copy
    from conftest import rel_err
    from ingvio_amd import capi
    from ingvio_amd.closed_loop import LM, host_step, make_loop, nominal_stage
    from nominal_helpers import assert_table
    F = 24
    cases = make_loop(2, 3, F=F, n_landmarks=0)
    n_max = ((max(c["P"].shape[0] for c in cases) + 9 + 15) // 16) * 16

    def ctx_of():
        ctx = capi.Context(batch=len(cases), n_max=n_max, c_max=12, f_max=F, m_max=64)
        for b, c in enumerate(cases):
            ctx.cov_set(b, c["P"])
        ctx.tracks_create(F)
        return ctx
    ch, cd = ctx_of(), ctx_of()
    cd.nominal_create(48)
    cd.nominal_set(0, [c["table"].as_dict() for c in cases])
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    for f in (0, 1):
        host_step(ch, cases, tabs, f)
        nominal_stage(cd, cases, f)()
        cd.frame_run()
        cd.frame_fetch()
    rng = np.random.default_rng(12)
    blocks = []
    for t in tabs:
        vidx = [t.slots[s]["idx"] for s in t.clones]
        blocks.append([make_cand(rng, vidx, [6] * len(vidx), 4 * len(vidx), 3)])
    n0 = [cd.n(b) for b in range(2)]
    got = cd.add_variable_delayed_batch(0, blocks, NOISE)
    dev = cd.nominal_get()
    dxp = np.zeros((2, cd.ldp))
    for b, t in enumerate(tabs):
        vidx, vsize, H_old, H_new, res, chk = blocks[b][0]
        added, dxh, chi2h, idxh = ch.add_variable_delayed(b, vidx, vsize, H_old, H_new, res, NOISE, 1.0, True, chk)
        assert abs(chi2h - chk) > 0.02 * chk
        assert added and got[b][0] == [True] and got[b][1] == [idxh] == [n0[b]]
        assert abs(got[b][2][0] - chi2h) <= 1e-9 * max(1.0, chi2h) and rel_err(got[b][3][0], dxh) < 1e-9
        pf = t.slots[t.clones[0]]["p"] + rng.normal(size=3) * 3.0
        anchor = t.clones[0]
        assert len(dev[b]["kind"]) == len(t.slots)
        t.slots.append(dict(kind=LM, idx=idxh, anchor=anchor, R=np.eye(3), p=pf.copy(), v=np.zeros(3)))
        row = np.zeros(15); row[0:9] = np.eye(3).reshape(9); row[9:12] = pf
        d = dev[b]
        d["kind"] = np.append(d["kind"], capi.NOM_LANDMARK); d["idx"] = np.append(d["idx"], got[b][1][0])
        d["anchor"] = np.append(d["anchor"], anchor); d["val"] = np.vstack([d["val"], row])
        t.box_plus(dxh)
        dxp[b, :len(got[b][3][0])] = got[b][3][0]
        cases[b]["frames"][2]["new_idx"] = n0[b] + 3                      # the host loop's clone goes behind the landmark
    cd.nominal_set(0, dev)
    cd.nominal_box_plus(0, dxp)
    dxh, acch, rowsh = host_step(ch, cases, tabs, 2)
    nominal_stage(cd, cases, 2)()
    cd.frame_run()
    dxd, accd, rowsd = cd.frame_fetch()
    assert np.array_equal(acch, accd) and np.array_equal(rowsh, rowsd) and rowsd.min() > 0
    dev = cd.nominal_get()
    for b, t in enumerate(tabs):
        assert rel_err(dxd[b], dxh[b]) < 1e-9 and rel_err(cd.cov_get(b), ch.cov_get(b)) < 1e-9
        assert_table(dev[b], t, 1e-9, "after the frame behind the initialisation")
        assert t.slots[t.clones[-1]]["idx"] == n0[b] + 3 - 6 and dev[b]["idx"][dev[b]["clone_var"][-1]] == n0[b] + 3 - 6
    ch.close(); cd.close()


@pytest.mark.gpu
def test_refused_while_a_split_frame_step_is_pending():
    from ingvio_amd import capi, host, synth
    ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
    cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
    ctx.snapshot()
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
    ctx.frame_run_phase(1, restore_prior=True)
    rng = np.random.default_rng(3)
    arr, cap, keep = capi.make_delayed_blocks([[make_cand(rng, [0], [9], 8, 3)] for _ in range(2)])
    before = [(ctx.n(b), ctx.cov_get(b)) for b in range(2)]
    assert raw_call(ctx, 0, 2, arr, cap) == capi.E_ARG
    for b in range(2):
        assert ctx.n(b) == before[b][0] and np.array_equal(ctx.cov_get(b), before[b][1])
    ctx.frame_run_phase(2)
    ctx.frame_fetch()
    n0 = [ctx.n(b) for b in range(2)]
    assert raw_call(ctx, 0, 2, arr, cap) == capi.OK and [ctx.n(b) for b in range(2)] == [n + 3 for n in n0]
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["gnss", "landmarks"])
def test_refused_while_a_stage_from_the_table_is_pending(what):
    """a GNSS epoch / a stand-alone landmark update staged from the nominal table and not yet run: refused as ingvio_nominal_box_plus is"""
    from conftest import load_golden
    from ingvio_amd import capi, synth
    from nominal_helpers import refused, table_ctx
    rng = np.random.default_rng(4)
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
    blocks = [[make_cand(rng, [0], [9], 8, 3)] for _ in cases]
    refused(ctx, lambda: ctx.add_variable_delayed_batch(0, blocks, NOISE), capi.E_ARG, sizes=True)
    if what == "gnss":
        ctx.gnss_run(); ctx.gnss_fetch()
    else:
        ctx.landmark_run(); ctx.landmark_fetch()
    ctx.close()


@pytest.mark.gpu
def test_a_trailing_update_that_is_not_positive_definite_stops_the_sequence():
    """an indefinite prior: the trailing S of the first candidate has a negative pivot.  The variable stays appended
    (addVariableDelayedInvertible ran), dx is zero, the status is E_NOT_PD, the filter's second candidate is not tried and the
    host's n follows the device's; the other filter of the call is what the oracle gives."""
    from ingvio_amd import capi
    rng = np.random.default_rng(8)
    Cw = 5; n = 21 + 6 * Cw
    good = spd(n, rng, 1e-2)
    v = rng.standard_normal(n)
    bad = good - 5.0 * np.outer(v, v) / n                                                         # one large negative eigenvalue
    vidx = [21 + 6 * i for i in range(Cw)]
    blocks = [[make_cand(rng, vidx, [6] * Cw, 4 * Cw, 3) for _ in range(2)] for _ in range(2)]
    Hu = np.linalg.qr(blocks[0][0][3], mode="complete")[0].T[3:] @ blocks[0][0][2]
    assert np.linalg.eigvalsh(Hu @ bad[21:, 21:] @ Hu.T).min() < -1.0                           # S of the lower rows is indefinite
    ctx = new_ctx([good], batch=2)
    ctx.cov_set(0, bad); ctx.cov_set(1, good)
    ref = oracle_run(good, blocks[1], do_chi2=False)
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE, do_chi2=False)
    assert list(ctx.delayed_status) == [capi.E_NOT_PD, capi.OK]
    assert got[0][0] == [True, False] and got[0][1] == [n, -1] and not got[0][3][0].any() and got[0][3][1] is None
    assert ctx.n(0) == n + 3 and np.array_equal(ctx.cov_get(0)[:n, :n], bad)                      # appended, not updated
    assert ref[1] == [True, True]
    compare(ctx, 1, got[1], ref)
    ctx.close()
