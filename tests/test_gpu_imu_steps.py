"""IMU propagation over every step count the C ABI accepts (1 <= k <= KMAX = 64).

k_propagate stages its steps in chunks of PROP_KCH = 10: k = 10 (what every other test and the bench use) is exactly one chunk.  Here
the fused propagation, the frame path and the track store's device-formed transition run at 1 .. 64 steps against the C oracle, on
both template variants of k_propagate (<= 64 / > 64 filters per launch), one and two row tiles, with and without the GNSS clock
states; and the entry points must refuse k = 0 / 65 and partial stages whose per-context settings (k, sigma, sigma_cb, sigma_rw)
disagree with the frame already staged, without changing anything."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
SIG = [0.004, 0.08, 0.0002, 0.008]
SCB, SRW = 0.2, 0.2
KS = (1, 2, 3, 4, 5, 9, 10, 11, 13, 14, 19, 20, 21, 31, 40, 63, 64)
# (n, clock-state indices GPS GLO GAL BDS drift): none / all five / drift with two biases absent
LAYOUTS = [(27, [-1] * 5), (87, [21, 22, 23, 24, 25]), (87, [40, -1, 66, -1, 30]), (256, [25, -1, 200, -1, 255])]


def spd(rng, n):
    A = rng.standard_normal((n, n))
    return A @ A.T / n + 0.05 * np.eye(n)


def realistic_steps(orc, rng, k):
    """k (Phi, G, dt) of oracle.imu_transition along the synthetic circle with noisy samples and biases."""
    from ingvio_amd import synth
    t = rng.uniform(0.0, 10.0)
    R, p, v = synth.true_pose(t)
    bg, ba, g = rng.normal(0.0, 2e-3, 3), rng.normal(0.0, 2e-2, 3), np.array([0.0, 0.0, -9.81])
    Phis, Gs, dts = np.zeros((k, 15, 15)), np.zeros((k, 15, 12)), np.zeros(k)
    for s in range(k):
        dt = 0.005 * rng.uniform(0.8, 1.2)
        gyro, acc = synth.true_imu(t + dt)
        R, p, v, Phis[s], Gs[s] = orc.imu_transition(R, p, v, bg, ba, gyro + rng.normal(0.0, 0.02, 3), acc + rng.normal(0.0, 0.2, 3), g, dt)
        dts[s] = dt
        t += dt
    return Phis, Gs, dts


def stress_steps(rng, k):
    return np.eye(15) + 0.02 * rng.standard_normal((k, 15, 15)), rng.uniform(-1, 1, (k, 15, 12)), rng.uniform(0.004, 0.006, k)


def check_fused(orc, ctx, b0, layouts, k, rng, stress=()):
    """One ingvio_propagate_fused call over filters [b0, b0 + len(layouts)) vs k stepwise oracle propagations per filter."""
    nb = len(layouts)
    Phis, Gs, dts, gis, refs = np.zeros((nb, k, 15, 15)), np.zeros((nb, k, 15, 12)), np.zeros((nb, k)), np.zeros((nb, 5), dtype=np.int32), []
    for i, (n, gi) in enumerate(layouts):
        Phis[i], Gs[i], dts[i] = stress_steps(rng, k) if i in stress else realistic_steps(orc, rng, k)
        gis[i] = gi
        P0 = spd(rng, n)
        ctx.cov_set(b0 + i, P0)
        oc = orc.Cov(P0, ld=n + 8)
        for s in range(k):
            oc.propagate(Phis[i, s], Gs[i, s], dts[i, s], SIG, 1, gi, SCB, SRW)
        refs.append(oc.P)
    ctx.propagate(b0, Phis, Gs, dts, SIG, 1, gis, SCB, SRW, fused=True)
    for i in range(nb):
        P = ctx.cov_get(b0 + i)
        assert rel_err(P, refs[i]) <= TIGHT, (k, nb, layouts[i][0], i in stress, rel_err(P, refs[i]))
        assert np.array_equal(P, P.T), (k, nb, i)


@pytest.fixture(scope="module")
def ctx65():
    from ingvio_amd import capi
    c = capi.Context(batch=65, n_max=256, c_max=11, f_max=16, m_max=16)
    yield c
    c.close()


@pytest.mark.parametrize("k", KS)
def test_fused_propagation_vs_stepwise_oracle(orc, ctx65, k):
    """k_propagate<true> (nb 1 / 4: the pinned-slab upload, 5: the staged one) and k_propagate<false> (65 filters) at every chunk
    shape: 1 and 2 steps, a last chunk of 1, 3, 4 or 5 steps (the two-wave split is off below 4), whole multiples of 10."""
    i = KS.index(k)
    rng = np.random.default_rng(7000 + k)
    nb = (1, 4, 5)[i % 3]
    lay = [LAYOUTS[(i + j) % 4] for j in range(nb)]
    check_fused(orc, ctx65, i % 7, lay, k, rng, stress=(nb - 1,) if nb > 1 else ((0,) if i % 2 else ()))
    lay65 = [LAYOUTS[j % 3] if j % 13 else LAYOUTS[(j // 13) % 4] for j in range(65)]
    check_fused(orc, ctx65, 0, lay65, k, rng, stress=(5, 64))


@pytest.mark.parametrize("k", (1, 11, 21, 64))
def test_fused_propagation_two_row_tiles(orc, k):
    """n = 257 / 400 in a context with n_max = 512: two row tiles, clock states on both sides of row 256."""
    from ingvio_amd import capi
    ctx = capi.Context(batch=2, n_max=512, c_max=11, f_max=16, m_max=16)
    rng = np.random.default_rng(7100 + k)
    check_fused(orc, ctx, 0, [(257, [21, 256, 130, 22, 23]), (400, [399, -1, 257, -1, 40])], k, rng, stress=(1,))
    check_fused(orc, ctx, 1, [(257, [256, 21, -1, -1, 100])], k, rng)
    ctx.close()


# ---- frame path -----------------------------------------------------------------------------------------------------------------
def host_case(orc, seed, k, C=11, F=40, n_landmarks=0, ld=512):
    """synth.build_case on the ORACLE's covariance: the prior, the measured frame's k steps (Phi / G of oracle.imu_transition) and
    its raw samples; the prior does not depend on k."""
    from ingvio_amd import synth
    flt, step, frame, info = synth.build_case(lambda P: orc.Cov(P, ld=ld), orc.imu_transition, seed=seed, F=F, C=C, n_gnss=6,
                                              n_landmarks=n_landmarks, k=k)
    assert len(step["dt"]) == k and step["raw"]["imu"].shape == (k, 7)
    return flt.cov.P, step, frame, info


def oracle_frame(orc, prior, step, frame, ld):
    oc = orc.Cov(prior, ld=ld)
    dxo, acco, _, _ = orc.frame_update(oc, step, frame, max_accept=0, compress_rule=1)
    return oc, dxo, acco


def settings(step):
    """(sigma, sigma_cb, sigma_rw) of a synth step: what the oracle's frame update propagates with"""
    return step["sigma"], step["sigma_cb"], step["sigma_rw"]


def stage_and_run(ctx, priors, steps, frames):
    for b, P in enumerate(priors):
        ctx.cov_set(b, P)
    ctx.snapshot()
    sigma, scb, srw = settings(steps[0])
    ctx.frame_stage(0, steps, frames, sigma, 1, scb, srw)
    ctx.frame_run(restore_prior=True)
    dx, acc, rows = ctx.frame_fetch()
    return dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b) for b in range(len(priors))]


def assert_matches_oracle(orc, res, b, prior, step, frame, info, ld, F):
    dx, acc, rows, Ps = res
    oc, dxo, acco = oracle_frame(orc, prior, step, frame, ld)
    P = Ps[b]
    assert P.shape[0] == oc.n and rows[b] == 6 * len(frame["clone_idx"]) and np.array_equal(acc[b, :F], acco), (b, rows[b], acc[b, :F].sum(), acco.sum())
    assert np.array_equal(acco == 0, info["outlier"])
    assert rel_err(P, oc.P) <= TIGHT and rel_err(dx[b, :len(dxo)], dxo) <= 1e-9, (b, rel_err(P, oc.P), rel_err(dx[b, :len(dxo)], dxo))
    assert np.array_equal(P, P.T) and np.diag(P).min() > 0


@pytest.mark.parametrize("k,big", [(1, False), (11, False), (21, False), (64, False), (11, True), (64, True)])
def test_frame_path_vs_oracle(orc, k, big):
    """ingvio_frame_stage + ingvio_frame_run(restore_prior) with host-formed Phi at k steps: n_max = 256 propagates and clones in one
    launch from the snapshot; n_max = 336 (N = 333) takes two row tiles and a separate k_augment."""
    from ingvio_amd import capi
    C, F, nb = 11, 40, 2
    n_lm, n_max = (80, 336) if big else (0, 256)
    cases = [host_case(orc, 60 + b, k, C=C, F=F, n_landmarks=n_lm, ld=n_max) for b in range(nb)]
    assert cases[0][3]["N_update"] == (333 if big else 93)
    ctx = capi.Context(batch=nb, n_max=n_max, c_max=C, f_max=F, m_max=64)
    res = stage_and_run(ctx, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    for b in range(nb):
        prior, step, frame, info = cases[b]
        assert_matches_oracle(orc, res, b, prior, step, frame, info, n_max, F)
    ctx.frame_run(restore_prior=True)                        # repeatable: bit-identical
    for b in range(nb):
        assert np.array_equal(ctx.cov_get(b), res[3][b])
    ctx.close()


# ---- track store: Phi / G formed on the device (k_imu_steps) --------------------------------------------------------------------
TC, TF, TT = 4, 24, 32


def track_ctx(nb):
    from ingvio_amd import capi
    ctx = capi.Context(batch=nb, n_max=64, c_max=TC, f_max=TF, m_max=64)
    ctx.tracks_create(TT)
    return ctx


def perm_of(b):
    return np.random.default_rng(50 + b).permutation(TT)[:TF].astype(np.int32)


def track_delta(frame, b, slot=None, feats=False, **extra):
    """window slot `slot` of the frame as the new column (every feature is observed by every clone), the update's features with it"""
    perm = perm_of(b)
    d = dict(clone_idx=frame["clone_idx"], clone_R=frame["clone_R"], clone_p=frame["clone_p"], feat_track=[], feat_anchor=[], feat_dof=[])
    if slot is not None:
        d.update(append=slot, obs_track=perm, obs_uv=np.ascontiguousarray(np.asarray(frame["uv"])[:, slot]))
    if feats:
        d.update(feat_track=perm, feat_anchor=frame["anchor"], feat_dof=frame["dof"], pf_track=perm, pf=frame["pf"])
    d.update(extra)
    return d


def stage_tracks(ctx, b0, steps, deltas, frame0):
    sigma, scb, srw = settings(steps[0])
    ctx.frame_stage_tracks_prepare(b0, steps, deltas, frame0, sigma, 1, scb, srw)()


def fill_store(ctx, cases, upto=TC):
    """columns 0 .. upto-1 of every filter's window; the last one carries the update's features"""
    steps, frames = [c[1] for c in cases], [c[2] for c in cases]
    for s in range(upto):
        stage_tracks(ctx, 0, steps, [track_delta(frames[b], b, s, feats=s == TC - 1) for b in range(len(cases))], frames[0])


def run_fetch(ctx, nb):
    ctx.frame_run(restore_prior=True)
    dx, acc, rows = ctx.frame_fetch()
    return dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b) for b in range(nb)]


@pytest.mark.parametrize("k", (1, 10, 16, 17, 21, 32, 50, 51, 64))
def test_track_store_transition_vs_host_transition(orc, k):
    """ingvio_frame_stage_tracks forms Phi / G from the raw samples on the device in chunks of 16 samples; the same frame through
    ingvio_frame_stage with oracle.imu_transition's Phi / G gives the same posterior (device sin / cos: 1-2 ulp off the host's)."""
    nb = 2
    cases = [host_case(orc, 80 + b, k, C=TC, F=TF, ld=64) for b in range(nb)]
    priors = [c[0] for c in cases]
    ref = track_ctx(nb)
    r0 = stage_and_run(ref, priors, [c[1] for c in cases], [c[2] for c in cases])
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
        prior, step, frame, info = cases[b]
        oc, dxo, acco = oracle_frame(orc, prior, step, frame, 64)
        assert np.array_equal(r1[1][b, :TF], acco) and rel_err(r1[3][b], oc.P) <= TIGHT
        assert np.array_equal(r1[3][b], r1[3][b].T)
    ctx.close()


# ---- contract edges -------------------------------------------------------------------------------------------------------------
def raw_stage(ctx, b0, steps, frames, frame0, k=None, tracks=False, sigma=None, scb=None, srw=None):
    """ingvio_frame_stage(_tracks) with the step count of every filter overridden to k; returns the status code"""
    from ingvio_amd import capi
    nb = len(steps)
    sa = ((capi.FrameStepRaw if tracks else capi.FrameStep) * nb)()
    fa = ((capi.TrackFrame if tracks else capi.MsckfFrame) * nb)()
    keep = []
    for i in range(nb):
        s, k1 = (capi.make_step_raw if tracks else capi.make_step)(steps[i])
        f, k2 = (capi.make_track_frame if tracks else capi.make_frame)(frames[i])
        if k is not None:
            s.k = k
        sa[i] = s; fa[i] = f; keep.append((k1, k2))
    o, chi2 = capi.make_opts(frame0, 0, 1, 0)
    s0 = settings(steps[0])
    sg = capi.f64(s0[0] if sigma is None else sigma)
    scb, srw = s0[1] if scb is None else scb, s0[2] if srw is None else srw
    if tracks:
        return ctx.L.ingvio_frame_stage_tracks(ctx.h, b0, nb, sa, fa, C.byref(o), capi._d(sg), 1, C.c_double(scb), C.c_double(srw), 0)
    return ctx.L.ingvio_frame_stage(ctx.h, b0, nb, sa, fa, C.byref(o), capi._d(sg), 1, C.c_double(scb), C.c_double(srw))


def with_k(step, k, rng):
    """the step with k samples: k <= len(step) a prefix, else the last one repeated (valid memory behind every pointer)"""
    idx = [min(s, len(step["dt"]) - 1) for s in range(max(k, 1))]
    out = dict(step, Phi=[step["Phi"][s] for s in idx], G=[step["G"][s] for s in idx], dt=[step["dt"][s] for s in idx])
    out["raw"] = dict(step["raw"], imu=np.asarray(step["raw"]["imu"])[idx])
    return out


def test_step_count_out_of_range_is_refused_and_changes_nothing(orc):
    """k = 0 and k = 65 through ingvio_propagate_fused, ingvio_frame_stage and ingvio_frame_stage_tracks: INGVIO_E_ARG, the covariance
    bit-identical, and the next valid stage + run equal to that of a context that never saw the bad call (for the track store this
    is how its contents are seen: the refused deltas drop a window slot, erase a track and append a junk column)."""
    from ingvio_amd import capi
    nb = 2
    cases = [host_case(orc, 90 + b, 12, C=TC, F=TF, ld=64) for b in range(nb)]
    priors, steps, frames = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    rng = np.random.default_rng(3)
    bad_ctx, ref_ctx = track_ctx(nb), track_ctx(nb)
    for ctx in (bad_ctx, ref_ctx):
        for b, P in enumerate(priors):
            ctx.cov_set(b, P)
        ctx.snapshot()
        fill_store(ctx, cases, upto=TC - 1)
    before = [bad_ctx.cov_get(b) for b in range(nb)]
    # ingvio_propagate_fused
    L = bad_ctx.L
    for k in (0, 65):
        Phi = capi.f64(np.tile(np.eye(15), (nb, 65, 1, 1))); G = capi.f64(np.ones((nb, 65, 15, 12))); dt = capi.f64(np.full((nb, 65), 0.005))
        gi = capi.i32(np.array([c[1]["gnss_idx"] for c in cases]))
        sig, scb, srw = settings(steps[0])
        rc = L.ingvio_propagate_fused(bad_ctx.h, 0, nb, k, capi._d(Phi), capi._d(G), capi._d(dt), capi._d(capi.f64(sig)), 1, capi._i(gi),
                                      C.c_double(scb), C.c_double(srw))
        assert rc == capi.E_ARG, (k, rc)
        bad = [with_k(s, max(k, 1), rng) for s in steps]
        assert raw_stage(bad_ctx, 0, bad, frames, frames[0], k=k) == capi.E_ARG, k
        deltas = [track_delta(frames[b], b, TC - 1, feats=True, drop=[0], free=[int(perm_of(b)[0])]) for b in range(nb)]
        for d in deltas:
            d["obs_uv"] = np.full_like(d["obs_uv"], 5.0)
        assert raw_stage(bad_ctx, 0, bad, deltas, frames[0], k=k, tracks=True) == capi.E_ARG, k
        for b in range(nb):
            assert np.array_equal(bad_ctx.cov_get(b), before[b]), (k, b)
    # the next valid stage: the store's last column with the update's features, then the run
    res = []
    for ctx in (bad_ctx, ref_ctx):
        stage_tracks(ctx, 0, steps, [track_delta(frames[b], b, TC - 1, feats=True) for b in range(nb)], frames[0])
        res.append(run_fetch(ctx, nb))
    for a, r in zip(res[0][:3], res[1][:3]):
        assert np.array_equal(a, r)
    for b in range(nb):
        assert np.array_equal(res[0][3][b], res[1][3][b])
        assert_matches_oracle(orc, res[0], b, *cases[b], 64, TF)
    # ... and through ingvio_frame_stage / ingvio_propagate_fused
    res = [stage_and_run(ctx, priors, steps, frames) for ctx in (bad_ctx, ref_ctx)]
    for b in range(nb):
        assert np.array_equal(res[0][3][b], res[1][3][b]) and np.array_equal(res[0][0][b], res[1][0][b])
    for ctx in (bad_ctx, ref_ctx):
        ctx.cov_set(0, priors[0])
        sig, scb, srw = settings(steps[0])
        ctx.propagate(0, np.stack(steps[0]["Phi"]), np.stack(steps[0]["G"]), steps[0]["dt"], sig, 1, [steps[0]["gnss_idx"]], scb, srw, fused=True)
    assert np.array_equal(bad_ctx.cov_get(0), ref_ctx.cov_get(0))
    bad_ctx.close(); ref_ctx.close()


SECOND_HALF = {            # what the second half-batch stage changes: k, or a factor on sigma / sigma_cb / sigma_rw
    "k": (12, 1.0, 1.0, 1.0),
    "sigma": (10, 2.0, 1.0, 1.0),
    "sigma_cb": (10, 1.0, 2.5, 1.0),
    "sigma_rw": (10, 1.0, 1.0, 0.25),
}


@pytest.mark.parametrize("tracks", [False, True])
@pytest.mark.parametrize("what", list(SECOND_HALF))
def test_half_batch_stages_with_different_settings(orc, what, tracks):
    """A full-batch stage at k = 10, then half-batch stages of the same frames: filters 0-1 with the same settings, filters 2-3 with
    another k (the same prior and window, 12 IMU steps) or sigma / sigma_cb / sigma_rw.  Either every filter's posterior is the
    oracle's with its own settings, or the second stage is refused with INGVIO_E_ARG and the run gives every filter the frame
    staged before it.  A silently wrong posterior fails."""
    from ingvio_amd import capi
    nb, half = 4, 2
    k2, f_sig, f_cb, f_rw = SECOND_HALF[what]
    ca = [host_case(orc, 100 + b, 10, C=TC, F=TF, ld=64) for b in range(nb)]
    cb = [host_case(orc, 100 + b, k2, C=TC, F=TF, ld=64) for b in range(nb)]
    for b in range(nb):
        assert np.array_equal(ca[b][0], cb[b][0])           # the same prior, another IMU interval
    sig, scb, srw = settings(ca[0][1])
    second = [dict(cb[b][1], sigma=[f_sig * x for x in sig], sigma_cb=f_cb * scb, sigma_rw=f_rw * srw) for b in range(nb)]
    ctx = track_ctx(nb)
    for b in range(nb):
        ctx.cov_set(b, ca[b][0])
    ctx.snapshot()
    sa, fa = [c[1] for c in ca], [c[2] for c in ca]
    if tracks:
        fill_store(ctx, ca)
        stage_tracks(ctx, 0, sa[:half], [track_delta(fa[b], b, feats=True) for b in range(half)], fa[0])
        rc = raw_stage(ctx, half, second[half:], [track_delta(fa[b], b, feats=True) for b in range(half, nb)], fa[0], tracks=True)
    else:
        ctx.frame_stage(0, sa, fa, sig, 1, scb, srw)
        ctx.frame_stage(0, sa[:half], fa[:half], sig, 1, scb, srw)
        rc = raw_stage(ctx, half, second[half:], fa[half:], fa[0])
    assert rc in (capi.OK, capi.E_ARG), rc
    dx, acc, rows, Ps = run_fetch(ctx, nb)
    for b in range(nb):
        step = second[b] if rc == capi.OK and b >= half else sa[b]
        oc, dxo, acco = oracle_frame(orc, ca[b][0], step, fa[b], 64)
        assert np.array_equal(acc[b, :TF], acco), (what, b, rc)
        assert rel_err(Ps[b], oc.P) <= TIGHT, (what, tracks, b, rc, rel_err(Ps[b], oc.P))
        assert rel_err(dx[b, :len(dxo)], dxo) <= 1e-9
    ctx.close()
