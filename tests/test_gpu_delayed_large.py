"""The large form of the delayed-initialisation front (k_delayed_front_large, ingvio_set_delayed_form): [H_old | res | T^T]
in a per-filter workspace, swept through LDS in panels.  Mode 2 against mode 0 and the oracle at small shapes; mode 1 at the shapes the
LDS form cannot take (18 ... 36 clones) against the oracle, for rows the host forms and rows formed from the track store and the table.
Scenarios and oracle results are delayed_large_helpers.py's (their conditions are asserted by tests/test_delayed_large_model.py);
tolerances are those of tests/test_gpu_delayed_batch.py and tests/test_gpu_landmark_init.py."""
import ctypes as C

import numpy as np
import pytest

import delayed_large_helpers as L
import landmark_init_helpers as H
from conftest import rel_err
from test_gpu_delayed_batch import NOISE, compare, make_cand, raw_call
from test_gpu_landmark_init import check_against_oracle, table_equal
from test_landmark_path import spd


def ctx_of(priors, form, batch=None, c_max=36):
    from ingvio_amd import capi
    n = max(P.shape[0] for P in priors)
    ctx = capi.Context(batch=batch or len(priors), n_max=((n + 15) // 16) * 16 + 16, c_max=c_max, f_max=16, m_max=96)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ctx.set_delayed_form(form)
    return ctx


def report(what, ctx, b, got, ref):
    c, added, idx, chi2, dxs = ref
    e_chi = max([abs(g - r) / max(1.0, r) for g, r in zip(got[2], chi2)] + [0.0])
    e_dx = max([np.linalg.norm(g - r) / max(1.0, np.linalg.norm(r)) for g, r, a in zip(got[3], dxs, added) if a and g is not None] + [0.0])
    e_P = np.linalg.norm(ctx.cov_get(b) - c.P) / np.linalg.norm(c.P) if ctx.n(b) == c.n else np.inf
    print("%s filter %d: n=%d chi2 err %.2e dx err %.2e P err %.2e" % (what, b, c.n, e_chi, e_dx, e_P))


_small = {}


def small_runs():
    """the small scenario under mode 0 and under mode 2 (one run each, shared)"""
    if not _small:
        priors, blocks, refs = L.reference("small")
        for form in (0, 2):
            ctx = ctx_of(priors, form, c_max=16)
            got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
            _small[form] = (ctx, got, [ctx.cov_get(b) for b in range(len(priors))], [ctx.n(b) for b in range(len(priors))])
    return _small


@pytest.mark.gpu
def test_every_candidate_in_the_large_form_at_small_shapes():
    """mode 2 against mode 0 and the oracle: 3 ... 16 clones, stereo and mono, non-contiguous column maps, s = 1, 3, 6, m = s + 1, odd m,
    63 / 64 / 65 / 129 columns (a panel is 64), a refused candidate"""
    priors, blocks, refs = L.reference("small")
    runs = small_runs()
    (c0, g0, P0, n0), (c2, g2, P2, n2) = runs[0], runs[2]
    assert n0 == n2
    for b in range(len(priors)):
        report("mode 2", c2, b, g2[b], refs[b][0])
        assert g2[b][0] == g0[b][0] and g2[b][1] == g0[b][1], b                          # added, new_idx
        compare(c0, b, g0[b], refs[b][0])
        compare(c2, b, g2[b], refs[b][0])
    assert list(c2.delayed_status) == [0] * len(priors)
    assert refs[-1][0][1] == [False] and np.array_equal(P2[-1], priors[-1])              # the refused filter: bit-unchanged


@pytest.mark.gpu
def test_quiet_filters_beside_filters_that_ran():
    """refused, skipped (m <= s) and empty filters are bit-unchanged under mode 2; the others get the bits of the full run"""
    priors, blocks, refs = L.reference("small")
    _, g2, P2, _ = small_runs()[2]
    blocks = [list(cs) for cs in blocks]
    v, s3, h3, r3 = blocks[3][0][:4]
    blocks[3] = [(v, s3, h3[:3], r3[:3], blocks[3][0][4][:3], 7.8)]                      # m == s: skipped
    blocks[4] = []
    quiet = (3, 4, len(priors) - 1)
    ctx = ctx_of(priors, 2, c_max=16)
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    for b in range(len(priors)):
        if b in quiet:
            assert got[b][0] == [False] * len(blocks[b]) and got[b][1] == [-1] * len(blocks[b]) and all(d is None for d in got[b][3])
            assert ctx.n(b) == priors[b].shape[0] and np.array_equal(ctx.cov_get(b), priors[b])
        else:
            assert got[b][:3] == g2[b][:3] and np.array_equal(got[b][3][0], g2[b][3][0]) and np.array_equal(ctx.cov_get(b), P2[b])
    assert got[3][2] == [0.0] and got[-1][2][0] > blocks[-1][0][5]
    ctx.close()


@pytest.mark.gpu
def test_shapes_the_lds_form_cannot_take():
    """mode 1: stereo 18 (the first that does not fit), 27 and 36 clones (m = 144, nc = 216, GNSS scalars behind the clones), mono 27 and
    36; per filter a refused candidate, then an accepted one.  Mode 0 refuses the same call, and again after mode 1"""
    from ingvio_amd import capi
    priors, blocks, refs = L.reference("large")
    ctx = ctx_of(priors, 0)
    arr, cap, keep = capi.make_delayed_blocks(blocks)
    assert raw_call(ctx, 0, len(priors), arr, cap) == capi.E_CAPACITY
    ctx.set_delayed_form(1)
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    for b in range(len(priors)):
        report("mode 1", ctx, b, got[b], refs[b][0])
        assert refs[b][0][1] == [False, True]
        compare(ctx, b, got[b], refs[b][0])
    assert list(ctx.delayed_status) == [0] * len(priors)
    ctx.set_delayed_form(0)
    before = [ctx.cov_get(b) for b in range(len(priors))]
    assert raw_call(ctx, 0, len(priors), arr, cap) == capi.E_CAPACITY
    assert all(np.array_equal(ctx.cov_get(b), before[b]) for b in range(len(priors)))
    ctx.close()


@pytest.mark.gpu
def test_a_round_that_mixes_the_forms():
    """an 11-clone filter (LDS form, bit-identical to mode 0), a 27-clone filter (large form), an empty filter, a refused one"""
    priors, blocks, refs = L.reference("mixed_forms")
    c0 = ctx_of(priors, 0)
    g0 = c0.add_variable_delayed_batch(0, blocks[:1], NOISE)
    ctx = ctx_of(priors, 1)
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    assert got[0][:3] == g0[0][:3] and np.array_equal(got[0][3][0], g0[0][3][0]) and np.array_equal(ctx.cov_get(0), c0.cov_get(0))
    for b in (0, 1):
        report("mixed", ctx, b, got[b], refs[b][0])
        assert refs[b][0][1] == [True]
        compare(ctx, b, got[b], refs[b][0])
    assert got[2] == ([], [], [], []) and got[3][0] == [False] and got[3][1] == [-1] and refs[3][0][1] == [False]
    assert abs(got[3][2][0] - refs[3][0][3][0]) <= 1e-9 * refs[3][0][3][0]
    for b in (2, 3):
        assert ctx.n(b) == priors[b].shape[0] and np.array_equal(ctx.cov_get(b), priors[b])
    c0.close(); ctx.close()


@pytest.mark.gpu
def test_sequences_at_27_clones():
    priors, blocks, refs = L.reference("sequence")
    ctx = ctx_of(priors, 1)
    got = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    for b in range(len(priors)):
        report("sequence", ctx, b, got[b], refs[b][0])
        n0 = priors[b].shape[0]
        assert refs[b][0][1] == [True, False, True] and refs[b][0][2] == [n0, -1, n0 + 3]
        compare(ctx, b, got[b], refs[b][0])
    ctx.close()


@pytest.mark.gpu
def test_partial_range():
    priors, blocks, refs = L.reference("partial")
    ctx = ctx_of(priors, 1)
    got = ctx.add_variable_delayed_batch(1, blocks, NOISE)
    for i in range(2):
        report("partial", ctx, 1 + i, got[i], refs[i][0])
        compare(ctx, 1 + i, got[i], refs[i][0])
    for b in (0, 3):
        assert ctx.n(b) == priors[b].shape[0] and np.array_equal(ctx.cov_get(b), priors[b])
    ctx.close()


@pytest.mark.gpu
def test_single_filter_call_at_27_clones():
    """ingvio_add_variable_delayed beyond its gate bound: refused under mode 0, a one-filter call of the batch path under mode 1"""
    from ingvio_amd import capi
    priors, blocks, refs = L.reference("mixed_forms")
    vidx, vsize, H_old, H_new, res, chk = blocks[1][0]
    ctx = ctx_of(priors, 0)
    with pytest.raises(capi.IngvioError) as e:
        ctx.add_variable_delayed(1, vidx, vsize, H_old, H_new, res, NOISE, 1.0, True, chk)
    assert e.value.code == capi.E_CAPACITY and ctx.n(1) == priors[1].shape[0] and np.array_equal(ctx.cov_get(1), priors[1])
    ctx.set_delayed_form(1)
    added, dx, chi2, idx = ctx.add_variable_delayed(1, vidx, vsize, H_old, H_new, res, NOISE, 1.0, True, chk)
    report("single", ctx, 1, ([added], [idx], [chi2], [dx]), refs[1][0])
    compare(ctx, 1, ([added], [idx], [chi2], [dx]), refs[1][0])
    vidx, vsize, H_old, H_new, res, chk = blocks[3][0]                                   # refused by the gate: nothing changes
    added, dx, chi2, idx = ctx.add_variable_delayed(3, vidx, vsize, H_old, H_new, res, NOISE, 1.0, True, chk)
    assert not added and dx is None and abs(chi2 - refs[3][0][3][0]) <= 1e-9 * chi2
    assert ctx.n(3) == priors[3].shape[0] and np.array_equal(ctx.cov_get(3), priors[3])
    ctx.close()


def assert_oracle_table(dev, t, what):
    from ingvio_amd import capi
    for i, s in enumerate(t.slots):
        if s is None:
            assert i >= len(dev["kind"]) or dev["kind"][i] == capi.NOM_NONE, (what, i)
            continue
        assert dev["idx"][i] == s["idx"] and dev["anchor"][i] == s["anchor"], (what, i)
        assert rel_err(dev["val"][i][0:9].reshape(3, 3), s["R"]) < 1e-9 and rel_err(dev["val"][i][9:12], s["p"]) < 1e-9, (what, i)
    assert list(dev["clone_var"]) == list(t.clones), what


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [True, False])
def test_rows_formed_from_the_table(stereo):
    """ingvio_landmark_init_nominal under mode 1: stereo 20 and 27 clones (one pending drop column), mono 35.  The rows against
    feat_all_obs_rows (1e-11 of max|H|), a mask with gaps whose anchor does not observe, then good / refused / good against the round
    trip nominal_get -> numpy rows -> oracle add_variable_delayed -> host boxPlus: the third candidate is formed at the moved poses,
    the landmarks' records and the retracted table are the oracle's"""
    from ingvio_amd import capi
    scn = L.lm_scenario(stereo)
    o = H.opts_frame(stereo)
    ctx = L.lm_ctx(scn, form=0)
    blocks = H.blocks_of(scn, [list(L.LM_TRACKS)] * len(scn))
    s0 = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(len(scn))])
    with pytest.raises(capi.IngvioError) as e:                                           # mode 0: refused, nothing changes
        ctx.landmark_init_nominal(0, blocks, o)
    assert e.value.code == capi.E_CAPACITY
    ctx.set_delayed_form(1)
    for b, f in enumerate(scn):
        for tr in (H.T_GOOD, H.T_GAP):
            Hx, Hf, r, _ = L.reference_rows(f, f["table"], tr)
            g_old, g_new, g_r = ctx.debug_landmark_init_rows(b, (tr, f["anchor"][tr], f["pf"][tr]), o, f["Cw"], f["drop"])
            assert g_old.shape == Hx.shape and g_new.shape == Hf.shape, (b, tr, g_old.shape, Hx.shape)
            s = np.abs(Hx).max()
            err = max(np.abs(g_old - Hx).max(), np.abs(g_new - Hf).max(), np.abs(g_r - r).max())
            print("rows stereo=%d window=%d track=%d m=%d err/max|H|=%.2e" % (stereo, f["Cw"], tr, Hx.shape[0], err / s))
            assert err <= 1e-11 * s, (b, tr, err / s)
    s1 = (ctx.nominal_get(), [ctx.cov_get(b) for b in range(len(scn))])
    for b in range(len(scn)):
        assert table_equal(s0[0][b], s1[0][b]) and np.array_equal(s0[1][b], s1[1][b])
    gap = ctx.landmark_init_nominal(0, H.blocks_of(scn, [[H.T_GAP]] * len(scn)), o)      # a mask with gaps, the anchor does not observe
    for b, f in enumerate(scn):
        ref = H.oracle_sequence(f, [H.T_GAP])
        assert ref["added"] == [True]
        check_against_oracle(ctx, b, gap[b], ref, "gaps")
        assert_oracle_table(ctx.nominal_get()[b], ref["table"], "gaps")
    ctx.close()
    ctx = L.lm_ctx(scn, form=1)
    got = ctx.landmark_init_nominal(0, blocks, o)
    assert list(ctx.delayed_status) == [0] * len(scn)
    dev = ctx.nominal_get()
    for b, f in enumerate(scn):
        ref = H.oracle_sequence(f, L.LM_TRACKS)
        up = H.oracle_sequence(f, L.LM_TRACKS, reform=False)
        print("sequence stereo=%d window=%d chi2 %s oracle %s" % (stereo, f["Cw"], got[b][2], ref["chi2"]))
        check_against_oracle(ctx, b, got[b], ref, "sequence")
        free = H.free_slots(f["table"], L.V_MAX)
        assert got[b][4] == [free[0], -1, free[2]]
        assert dev[b]["kind"][free[0]] == capi.NOM_LANDMARK and dev[b]["kind"][free[1]] == capi.NOM_NONE and dev[b]["kind"][free[2]] == capi.NOM_LANDMARK
        assert_oracle_table(dev[b], ref["table"], "sequence")
        move = abs(up["chi2"][2] - ref["chi2"][2]) / max(1.0, ref["chi2"][2])           # rows taken up front are a different result
        assert move > 1e-6 and abs(got[b][2][2] - up["chi2"][2]) / max(1.0, ref["chi2"][2]) > 0.5 * move
    ctx.close()


@pytest.mark.gpu
def test_the_setting():
    """bad values and pending states are refused with the mode unchanged; snapshot -> call -> restore -> call gives the same bits"""
    from ingvio_amd import capi, host, synth
    from ingvio_amd.closed_loop import make_loop, nominal_stage
    from nominal_helpers import table_ctx
    priors, blocks, refs = L.reference("sequence")
    ctx = ctx_of(priors, 0)
    arr, cap, keep = capi.make_delayed_blocks(blocks)
    for bad in (-1, 3, 7):
        assert ctx.L.ingvio_set_delayed_form(ctx.h, bad) == capi.E_ARG
    assert ctx.L.ingvio_set_delayed_form(None, 1) == capi.E_ARG
    assert raw_call(ctx, 0, 2, arr, cap) == capi.E_CAPACITY                              # still mode 0
    ctx.set_delayed_form(1)
    ctx.snapshot()
    g1 = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    P1 = [ctx.cov_get(b) for b in range(2)]
    ctx.restore()
    assert [ctx.n(b) for b in range(2)] == [P.shape[0] for P in priors]
    g2 = ctx.add_variable_delayed_batch(0, blocks, NOISE)
    for b in range(2):
        assert g1[b][:3] == g2[b][:3] and np.array_equal(ctx.cov_get(b), P1[b])
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(g1[b][3], g2[b][3]))
    ctx.close()
    # a split frame step pending
    ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
    cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
    ctx.snapshot()
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
    ctx.frame_run_phase(1, restore_prior=True)
    assert ctx.L.ingvio_set_delayed_form(ctx.h, 1) == capi.E_ARG
    ctx.frame_run_phase(2)
    ctx.frame_fetch()
    ctx.set_delayed_form(1)
    ctx.close()
    # a frame staged from the table that has not run
    cases = make_loop(2, 2, F=24, n_landmarks=0)
    ctx = table_ctx(cases)
    nominal_stage(ctx, cases, 0)()
    assert ctx.L.ingvio_set_delayed_form(ctx.h, 1) == capi.E_ARG
    ctx.frame_run()
    ctx.frame_fetch()
    ctx.set_delayed_form(1)
    ctx.close()


@pytest.mark.gpu
def test_refusals_that_remain():
    """under mode 1 the trailing update's S at m = 150, m > mld, columns beyond the context and too few free table slots still return
    INGVIO_E_CAPACITY and leave P, n and the table unchanged"""
    from ingvio_amd import capi
    rng = np.random.default_rng(5)
    Cw = 4; n = 21 + 6 * Cw
    P0 = spd(n, rng, 1e-2)
    ctx = capi.Context(batch=1, n_max=48, c_max=Cw, f_max=16, m_max=64)
    ctx.cov_set(0, P0)
    ctx.set_delayed_form(1)
    vidx, vsize = [21 + 6 * i for i in range(Cw)], [6] * Cw
    for cand in (make_cand(rng, vidx, vsize, 70, 3),                                     # m > mld
                 make_cand(rng, [21] * 12, [6] * 12, 8, 3)):                             # more columns than the context holds
        arr, cc, keep = capi.make_delayed_blocks([[cand]])
        assert raw_call(ctx, 0, 1, arr, cc) == capi.E_CAPACITY and ctx.n(0) == n and np.array_equal(ctx.cov_get(0), P0)
    arr, cc, keep = capi.make_delayed_blocks([[make_cand(rng, vidx, vsize, 8, 3), make_cand(rng, vidx, vsize, 8, 3)]])
    assert raw_call(ctx, 0, 1, arr, cc) == capi.E_CAPACITY and ctx.n(0) == n and np.array_equal(ctx.cov_get(0), P0)      # n + sum s > n_max
    ctx.close()
    Cb = 21; nb_ = 21 + 6 * Cb
    Pb = spd(nb_, rng, 1e-2)
    big = capi.Context(batch=1, n_max=224, c_max=30, f_max=16, m_max=64)
    big.cov_set(0, Pb)
    big.set_delayed_form(1)
    arr, cc, keep = capi.make_delayed_blocks([[make_cand(rng, vidx, vsize, 150, 3)]])   # S of the trailing update beyond LDS
    assert raw_call(big, 0, 1, arr, cc) == capi.E_CAPACITY and big.n(0) == nb_ and np.array_equal(big.cov_get(0), Pb)
    big.close()
    # rows from the table: fewer free slots than candidates
    scn = L.lm_scenario(False)
    o = H.opts_frame(False)
    ctx = L.lm_ctx(scn, form=1)
    free = len(H.free_slots(scn[0]["table"], L.V_MAX))
    tracks = [H.T_GOOD] * (free + 1)
    s0 = (ctx.nominal_get(), ctx.cov_get(0), ctx.n(0))
    with pytest.raises(capi.IngvioError) as e:
        ctx.landmark_init_nominal(0, H.blocks_of(scn, [tracks]), o)
    assert e.value.code == capi.E_CAPACITY
    assert table_equal(s0[0][0], ctx.nominal_get()[0]) and np.array_equal(s0[1], ctx.cov_get(0)) and s0[2] == ctx.n(0)
    ctx.close()
