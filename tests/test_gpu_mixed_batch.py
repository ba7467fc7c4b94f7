"""Batched frame step with per-filter IMU settings: every filter of one stage call may carry its own step count k and its own IMU /
clock noise (sigma[4], sigma_cb, sigma_rw).

k_propagate reads them from the filters' parameter blocks when a launch mixes them (k_propagate<SPLIT, true>) and keeps them scalar
kernel arguments when every filter shares them.  Each filter of a mixed batch must match the oracle with its own settings and be
bit-identical to the same filter in a uniform batch of the same size; this holds for the host-formed and the device-formed
(track store) transitions, partial stages, ingvio_frame_set_imu_noise, the asynchronous pipeline, consecutive frames and the split
frame step.  Refusals still change nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rel_err
from test_gpu_imu_steps import (TC, TF, TIGHT, assert_matches_oracle, fill_store, host_case, oracle_frame, perm_of, raw_stage, run_fetch,
                                settings, track_ctx, track_delta, with_k)

pytestmark = pytest.mark.gpu

KMIX = (1, 7, 10, 11, 20, 64)
NOISE_F = ((1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.0, 2.5, 1.0), (1.0, 1.0, 0.25), (0.5, 3.0, 4.0), (1.5, 0.5, 2.0))


@functools.lru_cache(maxsize=None)
def _case(orc, seed, k, C=11, F=40, n_lm=0, ld=256):
    return host_case(orc, seed, k, C=C, F=F, n_landmarks=n_lm, ld=ld)


def with_noise(step, f):
    """the step with sigma / sigma_cb / sigma_rw scaled by f = (f_sigma, f_cb, f_rw)"""
    sig, scb, srw = settings(step)
    return dict(step, sigma=[f[0] * x for x in sig], sigma_cb=f[1] * scb, sigma_rw=f[2] * srw)


def noise_row(step):
    sig, scb, srw = settings(step)
    return list(sig) + [scb, srw]


def stage_run(ctx, priors, steps, frames, noise=None, restore=True):
    """cov_set + snapshot + ONE whole-batch ingvio_frame_stage (the first step's noise), then ingvio_frame_set_imu_noise (optional),
    run and fetch"""
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ctx.snapshot()
    sigma, scb, srw = settings(steps[0])
    ctx.frame_stage(0, steps, frames, sigma, 1, scb, srw)
    if noise is not None:
        ctx.frame_set_imu_noise(0, noise)
    return run_fetch(ctx, len(priors)) if restore else None


def assert_same(a, b, what):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y), what
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert np.array_equal(x, y), (what, i, rel_err(x, y))


# ---- 1. mixed k in one stage call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,big", [(6, False), (66, False), (3, True)])
def test_mixed_k_frame_path(orc, nb, big):
    """k = 1, 7, 10, 11, 20, 64 across the filters of one ingvio_frame_stage: k_propagate<true, true> (6 filters), <false, true>
    (66 filters) and two row tiles (N = 333).  Every filter matches the oracle at its own k, and is bit-identical to the same filter
    in a uniform batch of the same size at that k."""
    from ingvio_amd import capi
    n_lm, n_max = (80, 336) if big else (0, 256)
    seeds = [300 + b % 6 for b in range(nb)]
    ks = [7, 64, 11] if big else [KMIX[(b + b // 6) % 6] for b in range(nb)]
    cases = [_case(orc, seeds[b], ks[b], n_lm=n_lm, ld=n_max) for b in range(nb)]
    priors = [c[0] for c in cases]
    ctx = capi.Context(batch=nb, n_max=n_max, c_max=11, f_max=40, m_max=64)
    res = stage_run(ctx, priors, [c[1] for c in cases], [c[2] for c in cases])
    for b in range(nb):
        assert_matches_oracle(orc, res, b, *cases[b], n_max, 40)
    for k in sorted(set(ks)):
        uni = [_case(orc, seeds[b], k, n_lm=n_lm, ld=n_max) for b in range(nb)]
        ru = stage_run(ctx, priors, [c[1] for c in uni], [c[2] for c in uni])
        for b in range(nb):
            if ks[b] == k:
                assert np.array_equal(res[3][b], ru[3][b]) and np.array_equal(res[0][b], ru[0][b]), (k, b)
                assert np.array_equal(res[1][b], ru[1][b]) and res[2][b] == ru[2][b]
    ctx.close()


# ---- 2. per-filter noise --------------------------------------------------------------------------------------------------------
def test_per_filter_noise_set_and_partial_stages(orc):
    """Different sigma[4], sigma_cb and sigma_rw per filter (GNSS clock states present, so the clock recursion sees them), with a k mix:
    (a) one whole-batch stage + ingvio_frame_set_imu_noise, (b) one partial stage per filter on a fresh context, (c) a whole-batch
    stage, then partial stages that change some filters' k and noise.  All three equal the oracle per filter and each other."""
    from ingvio_amd import capi
    nb = 6
    ks = [10, 10, 12, 10, 7, 12]
    cases = [_case(orc, 320 + b, ks[b], C=TC, F=TF, ld=64) for b in range(nb)]
    assert all(np.asarray(c[1]["gnss_idx"]).max() >= 0 for c in cases)
    priors, frames = [c[0] for c in cases], [c[2] for c in cases]
    steps = [with_noise(cases[b][1], NOISE_F[b]) for b in range(nb)]
    ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    ra = stage_run(ctx, priors, [c[1] for c in cases], frames, noise=[noise_row(s) for s in steps])
    for b in range(nb):
        oc, dxo, acco = oracle_frame(orc, priors[b], steps[b], frames[b], 64)
        assert np.array_equal(ra[1][b, :TF], acco) and rel_err(ra[3][b], oc.P) <= TIGHT, (b, rel_err(ra[3][b], oc.P))
        assert rel_err(ra[0][b, :len(dxo)], dxo) <= 1e-9
        if NOISE_F[b] != (1.0, 1.0, 1.0):          # the noise mattered
            oc0, _, _ = oracle_frame(orc, priors[b], cases[b][1], frames[b], 64)
            assert rel_err(oc0.P, oc.P) > 1e-8, b
    ctx.close()
    ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ctx.snapshot()
    for b in (3, 0, 5, 1, 4, 2):                    # (b) the first stage is partial: it gives every filter its settings first
        sg, scb, srw = settings(steps[b])
        ctx.frame_stage(b, [steps[b]], [frames[b]], sg, 1, scb, srw)
    assert_same(run_fetch(ctx, nb), ra, "partial stages")
    sg, scb, srw = settings(cases[0][1])            # (c) whole batch at other settings, then partial stages
    other = [_case(orc, 320 + b, 11, C=TC, F=TF, ld=64)[1] for b in range(nb)]
    ctx.frame_stage(0, other, frames, sg, 1, 2.0 * scb, srw)
    for b0, nb1 in ((0, 2), (2, 3), (5, 1)):
        sg, scb, srw = settings(steps[b0])
        assert raw_stage(ctx, b0, steps[b0:b0 + nb1], frames[b0:b0 + nb1], frames[0], sigma=sg, scb=scb, srw=srw) == capi.OK
        ctx.frame_set_imu_noise(b0, [noise_row(s) for s in steps[b0:b0 + nb1]])
    assert_same(run_fetch(ctx, nb), ra, "whole batch, then partial stages")
    ctx.close()


@pytest.mark.parametrize("second", ["subset", "none"])
@pytest.mark.parametrize("tracks", [False, True], ids=["flattened", "track_store"])
def test_restage_with_other_clock_indices_ends_the_strip_restore(orc, tracks, second):
    """Stage with all five clock states, run twice from the prior (the second run restores only the strips the first one wrote, which
    the staged clock-state indices name), then stage the same frame with another set of indices - a subset, or none with enable_gnss
    = 0 - and run from the prior again: bit-identical to a fresh context that staged the second set once and ran once.  The
    covariance is not read between the runs (that alone ends the strip restore)."""
    nb = 3
    cases = [_case(orc, 360 + b, (10, 7, 12)[b], C=TC, F=TF, ld=64) for b in range(nb)]
    priors, frames = [c[0] for c in cases], [c[2] for c in cases]
    steps_a = [c[1] for c in cases]
    assert all(np.asarray(s["gnss_idx"]).min() >= 0 and s["marg_idx"] >= 0 for s in steps_a)
    keep = (1, 0, 1, 0, 0) if second == "subset" else (0,) * 5
    enable_b = 1 if second == "subset" else 0
    steps_b = [dict(s, gnss_idx=[g if on else -1 for g, on in zip(s["gnss_idx"], keep)]) for s in steps_a]
    sigma, scb, srw = settings(steps_a[0])

    def stage(ctx, steps, enable, fill):
        if not tracks:
            ctx.frame_stage(0, steps, frames, sigma, enable, scb, srw)
            return
        for s in range(TC) if fill else (None,):        # the window's columns first; the re-stage is a delta without a new column
            deltas = [track_delta(frames[b], b, s, feats=s in (None, TC - 1)) for b in range(nb)]
            ctx.frame_stage_tracks_prepare(0, steps, deltas, frames[0], sigma, enable, scb, srw)()

    def fresh():
        ctx = track_ctx(nb)
        for b, P in enumerate(priors):
            ctx.cov_set(b, P)
        ctx.snapshot()
        return ctx

    ctx = fresh()
    stage(ctx, steps_a, 1, True)
    ctx.frame_run(restore_prior=True)
    ctx.frame_run(restore_prior=True)
    stage(ctx, steps_b, enable_b, False)
    got = run_fetch(ctx, nb)
    ctx.close()
    ref = fresh()
    stage(ref, steps_b, enable_b, True)
    want = run_fetch(ref, nb)
    stage(ref, steps_a, 1, False)
    first = run_fetch(ref, nb)
    ref.close()
    assert_same(got, want, (tracks, second))
    assert not all(np.array_equal(x, y) for x, y in zip(want[3], first[3])), "the clock-state indices did not matter"


# ---- 3. track store -------------------------------------------------------------------------------------------------------------
def test_track_store_mixed_k(orc):
    """ingvio_frame_stage_tracks with k = 1, 17, 51, 64 in one call: k_imu_steps forms each filter's Phi / G at its own slot; the
    posterior equals that of the same frames through ingvio_frame_stage with host-formed transitions, and the oracle's."""
    ks = (17, 1, 64, 51)
    nb = len(ks)
    cases = [_case(orc, 340 + b, ks[b], C=TC, F=TF, ld=64) for b in range(nb)]
    priors = [c[0] for c in cases]
    ref = track_ctx(nb)
    r0 = stage_run(ref, priors, [c[1] for c in cases], [c[2] for c in cases])
    ref.close()
    ctx = track_ctx(nb)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ctx.snapshot()
    fill_store(ctx, cases)
    r1 = run_fetch(ctx, nb)
    assert np.array_equal(r1[1], r0[1]) and np.array_equal(r1[2], r0[2])
    for b in range(nb):
        assert rel_err(r1[3][b], r0[3][b]) <= TIGHT and rel_err(r1[0][b], r0[0][b]) <= 1e-9, (b, rel_err(r1[3][b], r0[3][b]))
        oc, dxo, acco = oracle_frame(orc, *cases[b][:3], 64)
        assert np.array_equal(r1[1][b, :TF], acco) and rel_err(r1[3][b], oc.P) <= TIGHT
    ctx.close()


# ---- 4. asynchronous pipeline ---------------------------------------------------------------------------------------------------
def test_async_pipeline_with_noise(orc):
    """run(i); stage_async(i + 1); set_imu_noise(i + 1); fetch(i) over three frames with another k / noise mix each: every frame is
    bit-identical to staging it synchronously (the frame in flight keeps its own noise)."""
    from ingvio_amd import capi
    nb = 8
    mixes = [[(10, 11, 9, 10, 20, 1, 10, 7)[(b + i) % 8] for b in range(nb)] for i in range(3)]
    inputs = []
    for i in range(3):
        cs = [_case(orc, 360 + b, mixes[i][b], C=TC, F=TF, ld=64) for b in range(nb)]
        noise = [noise_row(with_noise(cs[b][1], NOISE_F[(b + 2 * i) % 6])) for b in range(nb)]
        inputs.append(([c[1] for c in cs], [c[2] for c in cs], noise))
    priors = [_case(orc, 360 + b, 10, C=TC, F=TF, ld=64)[0] for b in range(nb)]
    ref = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    want = [stage_run(ref, priors, *inputs[i]) for i in range(3)]
    ref.close()
    ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ctx.snapshot()
    sg, scb, srw = settings(inputs[0][0][0])
    calls = [ctx.frame_stage_prepare(0, st, fr, sg, 1, scb, srw, use_async=i > 0) for i, (st, fr, _) in enumerate(inputs)]
    calls[0]()
    ctx.frame_set_imu_noise(0, inputs[0][2])
    for i in range(3):
        ctx.frame_run(restore_prior=True)
        if i < 2:
            calls[i + 1]()
            ctx.frame_set_imu_noise(0, inputs[i + 1][2])
        dx, acc, rows = ctx.frame_fetch()
        got = (dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b) for b in range(nb)])
        assert_same(got, want[i], "frame %d" % i)
    ctx.close()


# ---- 5. consecutive frames ------------------------------------------------------------------------------------------------------
def test_jittering_k_over_frames_without_restore(orc):
    """Six frames without restore, k of every filter jittering in 9 .. 12 from frame to frame: every filter is bit-identical, frame by
    frame, to that filter in a same-size batch run at its k; after the last frame it matches the oracle's sequence of frame updates."""
    from ingvio_amd import capi
    nb, nf = 8, 6
    rng = np.random.default_rng(11)
    kj = rng.integers(9, 13, size=(nf, nb))
    kj[0, :] = [9, 10, 11, 12, 9, 10, 11, 12]
    seeds = [380 + b for b in range(nb)]
    priors = [_case(orc, s, 10, C=TC, F=TF, ld=64)[0] for s in seeds]
    ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    uni = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ocs = [orc.Cov(P, ld=64) for P in priors]
    for j in range(nf):
        cs = [_case(orc, seeds[b], int(kj[j, b]), C=TC, F=TF, ld=64) for b in range(nb)]
        before = [ctx.cov_get(b) for b in range(nb)]
        sg, scb, srw = settings(cs[0][1])
        ctx.frame_stage(0, [c[1] for c in cs], [c[2] for c in cs], sg, 1, scb, srw)
        ctx.frame_run(restore_prior=False)
        dx, acc, _ = ctx.frame_fetch()
        after = [ctx.cov_get(b) for b in range(nb)]
        for k in sorted(set(kj[j].tolist())):
            cu = [_case(orc, seeds[b], k, C=TC, F=TF, ld=64) for b in range(nb)]
            for b, P in enumerate(before):
                uni.cov_set(b, P)
            uni.frame_stage(0, [c[1] for c in cu], [c[2] for c in cu], sg, 1, scb, srw)
            uni.frame_run(restore_prior=False)
            dxu, accu, _ = uni.frame_fetch()
            for b in range(nb):
                if kj[j, b] == k:
                    assert np.array_equal(uni.cov_get(b), after[b]) and np.array_equal(dxu[b], dx[b]) and np.array_equal(accu[b], acc[b]), (j, b, k)
        for b in range(nb):
            orc.frame_update(ocs[b], cs[b][1], cs[b][2], max_accept=0, compress_rule=1)
    for b in range(nb):
        P = ctx.cov_get(b)
        assert P.shape == ocs[b].P.shape and rel_err(P, ocs[b].P) <= 1e-6, (b, rel_err(P, ocs[b].P))
    ctx.close(); uni.close()


# ---- 6. split frame step --------------------------------------------------------------------------------------------------------
def test_frame_parts_mixed_batch(orc):
    """ingvio_set_frame_parts(2) over a batch with mixed k and noise (each slice launches its own filters' blocks): bit-identical to
    parts = 1, over two frames (the second without restore)."""
    from ingvio_amd import capi
    nb = 32
    cs = [_case(orc, 400 + b % 8, (10, 11, 9, 12, 10, 30, 10, 1)[b % 8], C=TC, F=TF, ld=64) for b in range(nb)]
    noise = [noise_row(with_noise(cs[b][1], NOISE_F[b % 6])) for b in range(nb)]
    out = []
    for parts in (1, 2):
        ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
        ctx.set_frame_parts(parts)
        r = [stage_run(ctx, [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], noise=noise)]
        ctx.frame_run(restore_prior=False)
        dx, acc, rows = ctx.frame_fetch()
        r.append((dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b) for b in range(nb)]))
        out.append(r)
        ctx.close()
    assert_same(out[1][0], out[0][0], "frame 1")
    assert_same(out[1][1], out[0][1], "frame 2")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_k", [0, 65])
def test_one_bad_k_among_valid_ones_changes_nothing(orc, bad_k):
    """One filter with k = 0 / 65 among valid, different ones: ingvio_frame_stage and ingvio_frame_stage_tracks refuse the call with
    INGVIO_E_ARG; the covariance is unchanged and the next valid stage + run equals that of a context that never saw the call (the
    refused track deltas would have dropped a window slot, erased a track and appended a junk column)."""
    from ingvio_amd import capi
    nb = 3
    ks = [9, 12, 10]
    cases = [_case(orc, 420 + b, ks[b], C=TC, F=TF, ld=64) for b in range(nb)]
    priors, steps, frames = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    bad_ctx, ref_ctx = track_ctx(nb), track_ctx(nb)
    for ctx in (bad_ctx, ref_ctx):
        for b, P in enumerate(priors):
            ctx.cov_set(b, P)
        ctx.snapshot()
        fill_store(ctx, cases, upto=TC - 1)
    before = [bad_ctx.cov_get(b) for b in range(nb)]
    bad = [dict(s) for s in steps]
    bad[1] = with_k(steps[1], max(bad_k, 1), None)
    sa = (capi.FrameStep * nb)(); keep = []
    for i in range(nb):
        s, kp = capi.make_step(bad[i]); keep.append(kp)
        if i == 1:
            s.k = bad_k
        sa[i] = s
    fa = (capi.MsckfFrame * nb)()
    for i in range(nb):
        f, kp = capi.make_frame(frames[i]); keep.append(kp); fa[i] = f
    o, chi2 = capi.make_opts(frames[0], 0, 1, 0)
    sg, scb, srw = settings(steps[0])
    sgd = capi.f64(sg)
    assert bad_ctx.L.ingvio_frame_stage(bad_ctx.h, 0, nb, sa, fa, C.byref(o), capi._d(sgd), 1, C.c_double(scb), C.c_double(srw)) == capi.E_ARG
    ta = (capi.FrameStepRaw * nb)()
    for i in range(nb):
        s, kp = capi.make_step_raw(bad[i]); keep.append(kp)
        if i == 1:
            s.k = bad_k
        ta[i] = s
    deltas = [track_delta(frames[b], b, TC - 1, feats=True, drop=[0], free=[int(perm_of(b)[0])]) for b in range(nb)]
    for d in deltas:
        d["obs_uv"] = np.full_like(d["obs_uv"], 5.0)
    tf = (capi.TrackFrame * nb)()
    for i in range(nb):
        f, kp = capi.make_track_frame(deltas[i]); keep.append(kp); tf[i] = f
    assert bad_ctx.L.ingvio_frame_stage_tracks(bad_ctx.h, 0, nb, ta, tf, C.byref(o), capi._d(sgd), 1, C.c_double(scb), C.c_double(srw), 0) == capi.E_ARG
    for b in range(nb):
        assert np.array_equal(bad_ctx.cov_get(b), before[b]), b
    res = []
    for ctx in (bad_ctx, ref_ctx):
        ctx.frame_stage_tracks_prepare(0, steps, [track_delta(frames[b], b, TC - 1, feats=True) for b in range(nb)], frames[0], sg, 1, scb, srw)()
        res.append(run_fetch(ctx, nb))
    assert_same(res[0], res[1], "after the refused stages")
    for b in range(nb):
        assert_matches_oracle(orc, res[0], b, *cases[b], 64, TF)
    bad_ctx.close(); ref_ctx.close()


def test_set_imu_noise_refusals(orc):
    """ingvio_frame_set_imu_noise: nothing staged, a bad range, NULL, a value that is not finite, a split step pending: INGVIO_E_ARG;
    a refused call changes nothing."""
    from ingvio_amd import capi
    nb = 2
    cases = [_case(orc, 440 + b, (10, 12)[b], C=TC, F=TF, ld=64) for b in range(nb)]
    priors, steps, frames = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    good = capi.f64(np.array([noise_row(s) for s in steps]))
    L = ctx.L
    assert L.ingvio_frame_set_imu_noise(ctx.h, 0, nb, capi._d(good)) == capi.E_ARG            # nothing staged
    want = stage_run(ctx, priors, steps, frames)
    for b0, n in ((-1, 1), (0, 0), (1, 2), (2, 1), (0, 3)):
        assert L.ingvio_frame_set_imu_noise(ctx.h, b0, n, capi._d(good)) == capi.E_ARG, (b0, n)
    assert L.ingvio_frame_set_imu_noise(ctx.h, 0, nb, None) == capi.E_ARG
    for v in (np.nan, np.inf, -np.inf):
        badv = good.copy()
        badv[1, 4] = v
        assert L.ingvio_frame_set_imu_noise(ctx.h, 0, nb, capi._d(badv)) == capi.E_ARG, v
    assert_same(run_fetch(ctx, nb), want, "after refused calls")
    ctx.frame_run_phase(1, restore_prior=True)
    assert L.ingvio_frame_set_imu_noise(ctx.h, 0, nb, capi._d(good)) == capi.E_ARG              # split step pending
    ctx.frame_run_phase(2)
    ctx.frame_fetch()
    ctx.close()
