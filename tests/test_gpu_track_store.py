"""The device-resident track store against a host model (track_store_model.py), read back with the parity hooks
ingvio_debug_tracks_read / ingvio_debug_staged_frame: k_tracks_apply and k_tracks_gather (kernels_tracks.hip) and the packing of
frame_stage_tracks_impl (capi.hip) at the shapes the ABI accepts and the rest of the suite does not reach - more tracks than the 256
threads of a workgroup (several stride passes, track numbers up to 65535), windows up to 36 clones (mask bits 32..35, rows closing up
across bit 31 / 32), sub-ranges of the batch, every ordering inside one delta, the worst-case delta the stage buffer is sized for,
refused deltas, and stages pipelined under a running frame.

The store is integers and copied doubles: masks, points, anchors, dofs, clone tables and counts are compared with array_equal,
measurements bit for bit wherever the mask bit is set (closing a row up leaves stale values in the vacated columns and the gather
copies whole rows; the kernels read set bits only)."""
import numpy as np
import pytest

from test_track_store import build, rel, run_reference
from track_store_model import TrackStoreModel, assert_frame_equal, assert_store_equal, bits_of, same_bits

pytestmark = pytest.mark.gpu

E_CAPACITY = -2
SPECIAL = [0, 1, 255, 256, 257, 65534, 65535]                          # both sides of the stride and the ends of the 16-bit track field
STAGED_KEYS = ("n_clones", "n_feat", "clone_idx", "clone_R", "clone_p", "anchor", "dof", "obs_mask", "pf", "uv")


def stage_ctx(batch, C, F):
    """a context that is only staged into: no covariance is set, nothing runs"""
    from ingvio_amd import capi
    N = 21 + 6 + 6 * C
    return capi.Context(batch=batch, n_max=((N + 15) // 16) * 16, c_max=C, f_max=F, m_max=64)


def frame_opts():
    from ingvio_amd import synth
    Rlr, tlr = synth.t_cl2cr()
    return dict(stereo=1, R_cl2cr=Rlr, t_cl2cr=tlr, noise=synth.PARAMS["visual_noise"], chi2_table=synth.chi2_table())


def raw_step(seed, k=2):
    rng = np.random.default_rng(seed)
    imu = np.concatenate([rng.normal(0.0, 0.1, (k, 3)), rng.normal(0.0, 0.5, (k, 3)) + np.array([0.0, 0.0, 9.8]), np.full((k, 1), 0.005)], axis=1)
    return dict(raw=dict(imu=imu, R=np.eye(3), p=np.zeros(3), v=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), gravity=np.array([0.0, 0.0, -9.8])),
                sigma=[1e-3, 1e-2, 1e-5, 1e-4], marg_idx=-1)


def clone_table(rng, n):
    return dict(clone_idx=rng.permutation(21 + 6 * np.arange(n)).astype(np.int32), clone_R=rng.normal(size=(n, 9)), clone_p=rng.normal(size=(n, 3)))


def full(d):
    out = dict(clone_idx=[], clone_R=np.zeros((0, 9)), clone_p=np.zeros((0, 3)), feat_track=[], feat_anchor=[], feat_dof=[])
    out.update(d)
    return out


def stage(ctx, deltas, steps, opts, b0=0, use_async=False):
    ctx.frame_stage_tracks_prepare(b0, steps, [full(d) for d in deltas], opts, steps[0]["sigma"], 1, 0.2, 0.2, use_async=use_async,
                                   max_accept=0, compress_rule=1)()


def flat(model):
    return model.mask(), model.uv(), model.pf()


def check(ctx, b, model, d, what):
    """filter b's store and staged frame against the model, after delta d"""
    d = full(d)
    assert_store_equal(ctx.debug_tracks_read(b), flat(model), ctx.c_max, what)
    want = model.gather(d["feat_track"], d["feat_anchor"], d["feat_dof"], d.get("feat_sel"), ctx.f_max)
    want.update(n_clones=len(d["clone_idx"]), clone_idx=d["clone_idx"], clone_R=d["clone_R"], clone_p=d["clone_p"])
    assert_frame_equal(ctx.debug_staged_frame(b), want, ctx.c_max, what, have=want["have"])


def same_store(a, b):
    """every word of two read-backs, stale columns included"""
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def same_staged(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint64) if np.asarray(a[k]).dtype == np.float64 else a[k],
                              np.asarray(b[k]).view(np.uint64) if np.asarray(b[k]).dtype == np.float64 else b[k]) for k in STAGED_KEYS)


# ---- a. random delta sequences ----------------------------------------------------------------------------------------------------
def sequence(seed, T, C, f_max, pool, n_extra, observe_all):
    """One filter's deltas, each with a feature list and a clone table, and the tracks the test looks at by name.  By construction:
    the window filled to C; C + 1 steady-state frames (drop slot 0, append at C - 1: every bit travels down to slot 0); a delta that
    observes every track; a drop of slot 0, a middle slot and the top slot; a drop with an append to the vacated top slot; a track
    freed and observed in one delta; a free of a track never used; an empty delta; points for freed tracks; n_extra random ones."""
    rng = np.random.default_rng(seed)
    pool = np.asarray(pool)
    shadow = TrackStoreModel(T, C)                                       # the generator's bookkeeping: which tracks hold what
    out, marks, used = [], {}, set()
    max_obs = min(len(pool), 200)

    def emit(empty=False, **d):
        i = len(out)
        F = min([0, f_max, 1, f_max - 1][i] if i < 4 else int(rng.integers(0, f_max + 1)), len(pool))
        ncl = C if i % 3 == 0 else int(rng.integers(1, C + 1))
        if empty:
            F, ncl = 0, 0
        an = rng.integers(0, max(ncl, 1), size=F); do = rng.integers(0, 256, size=F)
        if F:
            an[-1] = ncl - 1; do[-1] = 255; do[0] = 0                  # the byte limits of the feature word
        d.update(feat_track=rng.choice(pool, size=F, replace=False).astype(np.int32),      # every track once, in no order
                 feat_anchor=an.astype(np.int32), feat_dof=do.astype(np.int32),
                 feat_sel=rng.integers(0, 2 ** 64, size=F, dtype=np.uint64) if i % 2 else None, **clone_table(rng, ncl))
        shadow.apply(d); used.update(int(t) for t in d.get("obs_track", []))
        out.append(d)

    def some(nmax, exclude=()):
        cand = np.setdiff1d(pool, np.asarray(exclude, dtype=pool.dtype)) if len(exclude) else pool
        return rng.choice(cand, size=min(int(rng.integers(0, nmax + 1)), len(cand)), replace=False)

    def column(slot, tracks=None, pts=None, **more):
        tr = some(max_obs) if tracks is None else np.asarray(tracks)
        pt = some(30) if pts is None else np.asarray(pts)
        return dict(append=slot, obs_track=tr, obs_uv=rng.normal(size=(len(tr), 4)), pf_track=pt, pf=rng.normal(size=(len(pt), 3)), **more)

    for s in range(C):                                                   # the window fills up
        more = {}
        if s == 1:
            marks["never"] = int([t for t in pool if int(t) not in used][0])
            more["free"] = [marks["never"]]                              # a free of a track that was never used
        elif s % 3 == 0 and s:
            more["free"] = some(4)
        emit(**column(s, **more))
    for _ in range(C + 1):                                               # steady state: a drop and an append to the vacated top slot
        emit(**column(C - 1, drop=[0]))
    if observe_all:
        emit(**column(C - 1, tracks=rng.permutation(T), pts=rng.permutation(T), drop=[0]))
    pt = some(30)
    emit(drop=[0, C // 2, C - 1], pf_track=pt, pf=rng.normal(size=(len(pt), 3)))      # slot 0, a middle slot and the top slot, no new column
    held = sorted(t for t, r in shadow.obs.items() if len(r) >= 1)
    assert len(held) >= 2
    t, u = (int(x) for x in rng.choice(held, size=2, replace=False))
    tr = rng.permutation(np.concatenate([some(max_obs, exclude=[t]), [t]]))
    emit(**column(C - 3, tracks=tr, free=[t]))                           # freed and observed in one delta: only the new bit is left
    assert sorted(shadow.obs[t]) == [C - 3]
    marks["reobserved"] = (len(out) - 1, t, C - 3)
    emit(empty=True, append=-1)
    emit(**column(C - 2, tracks=some(max_obs, exclude=[u]), pts=[u], free=[u]))      # a point for a track freed in the same delta
    assert shadow.obs[u] == {}
    marks["freed_point"] = (len(out) - 1, u)
    emit(**column(C - 1, pts=[u, marks["never"]]))                       # ... and for tracks freed earlier
    n = C
    for _ in range(n_extra):
        if n == C:
            k = int(rng.integers(1, 3))
            n -= k
            emit(**column(n, drop=np.sort(rng.choice(C, size=k, replace=False)), free=some(3)))
        else:
            emit(**column(n))
        n += 1
    return out, marks


@pytest.mark.parametrize("T,C,F,n_extra,observe_all", [(300, 11, 40, 11, True),        # two stride passes, the second partial
                                                       (513, 36, 64, 1, True),         # three passes, mask bits up to 35
                                                       (65536, 4, 24, 0, False)])      # the whole 16-bit track field
def test_random_delta_sequences_equal_the_host_model(T, C, F, n_extra, observe_all):
    nb = 3
    ctx = stage_ctx(nb, C, F)
    ctx.tracks_create(T)
    opts = frame_opts()
    seqs = []
    for b in range(nb):
        pool = np.arange(T) if T <= 1024 else np.unique(np.concatenate([SPECIAL, np.random.default_rng(b).choice(T, size=40, replace=False)]))
        seqs.append(sequence(1000 * C + b, T, C, F, pool, n_extra, observe_all))
    assert len({len(s[0]) for s in seqs}) == 1
    models = [TrackStoreModel(T, C) for _ in range(nb)]
    steps = [raw_step(b) for b in range(nb)]
    top = 0
    for i in range(len(seqs[0][0])):
        ds = [seqs[b][0][i] for b in range(nb)]
        stage(ctx, ds, steps, opts)
        for b in range(nb):
            models[b].apply(ds[b])
            check(ctx, b, models[b], ds[b], (i, b))
            marks = seqs[b][1]
            if i == marks["reobserved"][0]:
                _, t, slot = marks["reobserved"]
                assert int(ctx.debug_tracks_read(b)[0][t]) == 1 << slot
            if i == marks["freed_point"][0]:
                u = marks["freed_point"][1]
                mask, _, pf = ctx.debug_tracks_read(b)
                assert int(mask[u]) == 0 and same_bits(pf[u], ds[b]["pf"][0])
            top |= int(np.bitwise_or.reduce(models[b].mask()))
    assert top == (1 << C) - 1                                           # every mask bit of the window has been set on the way
    if observe_all:
        assert any(len(d.get("obs_track", [])) == T for d in seqs[0][0])
    ctx.close()


# ---- b. the gather beyond one stride pass ----------------------------------------------------------------------------------------
def test_gather_of_more_features_than_threads():
    nb, T, C, F = 2, 400, 11, 300
    ctx = stage_ctx(nb, C, F)
    ctx.tracks_create(T)
    opts = frame_opts()
    steps = [raw_step(b) for b in range(nb)]
    rngs = [np.random.default_rng(40 + b) for b in range(nb)]
    models = [TrackStoreModel(T, C) for _ in range(nb)]

    def go(ds):
        stage(ctx, ds, steps, opts)
        for b in range(nb):
            models[b].apply(ds[b])
            check(ctx, b, models[b], ds[b], b)

    def column(r, s):
        tr = r.choice(T, size=260, replace=False)
        return dict(append=s, obs_track=tr, obs_uv=r.normal(size=(260, 4)), pf_track=tr[:150], pf=r.normal(size=(150, 3)))

    for s in range(C):
        go([column(r, s) for r in rngs])
    for n_feat in (300, 257, 1):                                         # a later, smaller frame zeroes the mask rows the earlier one filled
        go([dict(feat_track=r.choice(T, size=n_feat, replace=False).astype(np.int32), feat_anchor=r.integers(0, C, size=n_feat).astype(np.int32),
                 feat_dof=r.integers(0, 256, size=n_feat).astype(np.int32),
                 feat_sel=r.integers(0, 2 ** 64, size=n_feat, dtype=np.uint64) if n_feat == 257 else None, **clone_table(r, C)) for r in rngs])
        if n_feat == 300:
            assert all(ctx.debug_staged_frame(b)["obs_mask"][257:].any() for b in range(nb))
    ctx.close()


# ---- real windows: the flattened frame of test_track_store.build as deltas ----------------------------------------------------------
def window_deltas(case, tracks, C):
    """the case's flattened frame column by column; the last delta carries the feature list and the points"""
    fr = case[2]
    has = bits_of(fr["obs_mask"], C)
    uv = np.array(fr["uv"])
    table = dict(clone_idx=fr["clone_idx"], clone_R=fr["clone_R"], clone_p=fr["clone_p"])
    out = []
    for s in range(C):
        js = np.flatnonzero(has[:, s])
        out.append(dict(append=s, obs_track=tracks[js], obs_uv=uv[js, s].reshape(-1, 4), **table))
    out[-1].update(feat_track=tracks, feat_anchor=fr["anchor"], feat_dof=fr["dof"], pf_track=tracks, pf=fr["pf"])
    return out


def track_numbers(nb, T, F, seed):
    return [np.random.default_rng(seed + b).permutation(T)[:F].astype(np.int32) for b in range(nb)]


def run_and_fetch(ctx, nb):
    ctx.frame_run(restore_prior=True)
    dx, acc, rows = ctx.frame_fetch()
    return dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b) for b in range(nb)]


def same_results(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and all(np.array_equal(p, q) for p, q in zip(a[3], b[3]))


# ---- c. the two ways of staging leave the same frame -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,F", [(11, 40), (36, 48)])
def test_both_ways_of_staging_leave_the_same_frame(C, F):
    nb, T = 2, 300
    ctx, cases = build(nb, C, F, 500 + C)
    steps = [c[1] for c in cases]
    ctx.frame_stage(0, steps, [c[2] for c in cases], steps[0]["sigma"], 1, 0.2, 0.2)
    flattened = [ctx.debug_staged_frame(b) for b in range(nb)]
    for b in range(nb):                                                  # the hook reads what ingvio_frame_stage was given
        fr = cases[b][2]
        assert_frame_equal(flattened[b], dict(fr, n_feat=F, n_clones=C), C, b)
    ctx.tracks_create(T)
    tracks = track_numbers(nb, T, F, 60)
    deltas = [window_deltas(cases[b], tracks[b], C) for b in range(nb)]
    for s in range(C):
        stage(ctx, [deltas[b][s] for b in range(nb)], steps, cases[0][2])
    for b in range(nb):
        got = ctx.debug_staged_frame(b)
        assert got["obs_mask"][:F].any()
        assert_frame_equal(got, flattened[b], C, b)
    ctx.close()


# ---- d. sub-ranges of the batch ----------------------------------------------------------------------------------------------------
def test_sub_ranges_touch_their_own_filters_only():
    nb, C, F, T = 5, 11, 40, 300
    ctx, cases = build(nb, C, F, 600)
    ctx.snapshot()
    ctx.tracks_create(T)
    steps = [c[1] for c in cases]
    opts = cases[0][2]
    tracks = track_numbers(nb, T, F, 70)
    deltas = [window_deltas(cases[b], tracks[b], C) for b in range(nb)]
    steady = [dict(deltas[b][C - 1], drop=[C - 1]) for b in range(nb)]     # the newest slot leaves and comes back with the same column
    models = [TrackStoreModel(T, C) for _ in range(nb)]

    def part(ds, b0, n):
        stage(ctx, ds[b0:b0 + n], steps[b0:b0 + n], opts, b0=b0)
        for b in range(b0, b0 + n):
            models[b].apply(ds[b])
            check(ctx, b, models[b], ds[b], (b0, n, b))

    def read_all():
        return [(ctx.debug_tracks_read(b), ctx.debug_staged_frame(b)) for b in range(nb)]

    for s in range(C - 1):
        part([deltas[b][s] for b in range(nb)], 0, nb)
    last = [deltas[b][C - 1] for b in range(nb)]
    before = read_all()
    part(last, 2, 2)
    after = read_all()
    for b in (0, 1, 4):                                                  # every word, stale columns included
        assert same_store(before[b][0], after[b][0]) and same_staged(before[b][1], after[b][1]), b
    for b in (2, 3):
        assert not same_store(before[b][0], after[b][0])
    part(last, 0, 2); part(last, 4, 1)
    for b0, n in ((0, 2), (2, 2), (4, 1)):
        part(steady, b0, n)
    in_parts = read_all()
    res_parts = run_and_fetch(ctx, nb)
    assert res_parts[1][:, :F].sum() > nb * F // 2
    # the same deltas, every one as a whole-batch call
    ctx.tracks_create(T)
    models = [TrackStoreModel(T, C) for _ in range(nb)]
    for s in range(C):
        part([deltas[b][s] for b in range(nb)], 0, nb)
    part(steady, 0, nb)
    whole = read_all()
    for b in range(nb):
        assert_store_equal(in_parts[b][0], whole[b][0], C, b)
        assert_frame_equal(in_parts[b][1], whole[b][1], C, b)
    assert same_results(res_parts, run_and_fetch(ctx, nb))              # the same arithmetic on the same inputs
    ctx.close()


# ---- e. the large window fed from the store --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [33, 36])
@pytest.mark.parametrize("stereo", [True, False])
def test_large_window_from_the_track_store_equals_the_staged_frame(C, stereo):
    """test_frame_from_the_track_store_equals_the_staged_frame at the large-window classes (kernels_bigwin.hip, 243-column state), with
    its bounds: 1e-11 on the covariance and 1e-9 on dx for the device's sin / cos in Phi and G."""
    nb, F, T = 2, 48, 300
    ctx, cases = build(nb, C, F, 800 + C, stereo=stereo)
    kw = dict(max_accept=0, compress_rule=1)
    dx0, acc0, rows0, P0 = run_reference(ctx, cases, **kw)
    assert acc0[:, :F].sum() > nb * F // 2
    ctx.tracks_create(T)
    steps = [c[1] for c in cases]
    tracks = track_numbers(nb, T, F, 90)
    deltas = [window_deltas(cases[b], tracks[b], C) for b in range(nb)]
    for s in range(C):
        stage(ctx, [deltas[b][s] for b in range(nb)], steps, cases[0][2])
    dx1, acc1, rows1, P1 = run_and_fetch(ctx, nb)
    assert np.array_equal(acc1, acc0) and np.array_equal(rows1, rows0)
    for b in range(nb):
        print("C %d stereo %d filter %d: rel P %.3e rel dx %.3e" % (C, stereo, b, rel(P1[b], P0[b]), rel(dx1[b], dx0[b])))
    for b in range(nb):
        assert rel(P1[b], P0[b]) < 1e-11 and rel(dx1[b], dx0[b]) < 1e-9, (b, rel(P1[b], P0[b]), rel(dx1[b], dx0[b]))
    ctx.close()


# ---- f. the worst-case delta --------------------------------------------------------------------------------------------------------
def test_worst_case_delta_fits_the_stage():
    from ingvio_amd import capi
    nb, T, C, F = 3, 300, 11, 40
    ctx = stage_ctx(nb, C, F)
    ctx.tracks_create(T)
    opts = frame_opts()
    rngs = [np.random.default_rng(20 + b) for b in range(nb)]
    models = [TrackStoreModel(T, C) for _ in range(nb)]

    def go(ds, steps):
        stage(ctx, ds, steps, opts)
        for b in range(nb):
            models[b].apply(ds[b])
            check(ctx, b, models[b], ds[b], b)

    for s in range(C):
        go([dict(append=s, obs_track=r.choice(T, size=200, replace=False), obs_uv=r.normal(size=(200, 4))) for r in rngs], [raw_step(b) for b in range(nb)])
    # what stage_cap is sized for: every slot leaves, every track is erased, observed and gets a point, f_max features with a selection,
    # the full clone table and 64 IMU samples - on every filter
    worst = [dict(drop=np.arange(C), free=r.permutation(T), append=0, obs_track=r.permutation(T), obs_uv=r.normal(size=(T, 4)),
                  pf_track=r.permutation(T), pf=r.normal(size=(T, 3)), feat_track=r.choice(T, size=F, replace=False).astype(np.int32),
                  feat_anchor=r.integers(0, C, size=F).astype(np.int32), feat_dof=r.integers(0, 256, size=F).astype(np.int32),
                  feat_sel=r.integers(0, 2 ** 64, size=F, dtype=np.uint64), **clone_table(r, C)) for r in rngs]
    long_steps = [raw_step(b, k=64) for b in range(nb)]
    go(worst, long_steps)
    for b in range(nb):
        assert np.array_equal(models[b].mask(), np.ones(T, dtype=np.uint64))
    before = [ctx.debug_tracks_read(b) for b in range(nb)]
    over = dict(worst[1], obs_track=np.concatenate([worst[1]["obs_track"], [0]]), obs_uv=np.zeros((T + 1, 4)))
    with pytest.raises(capi.IngvioError) as e:
        stage(ctx, [worst[0], over, worst[2]], long_steps, opts)
    assert e.value.code == E_CAPACITY
    for b in range(nb):
        assert same_store(before[b], ctx.debug_tracks_read(b)), b
    ctx.close()


# ---- g. refusals change nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_async", [False, True])
def test_refused_deltas_change_nothing(use_async):
    from ingvio_amd import capi
    nb, C, F, T = 3, 6, 8, 16

    def fresh():
        ctx, cases = build(nb, C, F, 77)
        ctx.snapshot()
        ctx.tracks_create(T)
        steps = [c[1] for c in cases]
        tracks = track_numbers(nb, T, F, 80)
        deltas = [window_deltas(cases[b], tracks[b], C) for b in range(nb)]
        for s in range(C):
            stage(ctx, [deltas[b][s] for b in range(nb)], steps, cases[0][2])
        steady = [dict(deltas[b][C - 1], drop=[C - 1]) for b in range(nb)]      # leaves the store where it was
        return ctx, cases, steps, tracks, steady

    def good(ctx, cases, steps, steady):
        stage(ctx, steady, steps, cases[0][2], use_async=use_async)
        return run_and_fetch(ctx, nb)

    ctx0, cases0, steps0, _, steady0 = fresh()
    want = good(ctx0, cases0, steps0, steady0)
    assert want[1][:, :F].sum() > 0
    ctx0.close()

    ctx, cases, steps, tracks, steady = fresh()
    table = dict(clone_idx=cases[1][2]["clone_idx"], clone_R=cases[1][2]["clone_R"], clone_p=cases[1][2]["clone_p"])
    one = np.zeros((1, 4))

    def valid(b):                                                        # would change masks, measurements and points if it were applied
        return dict(steady[b], drop=[0], free=[int(tracks[b][1])], obs_track=tracks[b][:3], obs_uv=np.ones((3, 4)), pf_track=tracks[b][:1], pf=np.ones((1, 3)))

    bad = [dict(free=[T]),
           dict(pf_track=[-1], pf=np.zeros((1, 3))),
           dict(append=0, obs_track=[T], obs_uv=one),
           dict(drop=[C]),
           dict(drop=[2, 2]),
           dict(append=C, obs_track=[0], obs_uv=one),
           dict(obs_track=[0], obs_uv=one),                              # observations without a slot
           dict(feat_track=[T], feat_anchor=[0], feat_dof=[1]),
           dict(feat_track=[0], feat_anchor=[C], feat_dof=[1]),          # anchor = n_clones
           dict(feat_track=[0], feat_anchor=[0], feat_dof=[256])]
    for i, d in enumerate(bad):
        before = [(ctx.debug_tracks_read(b), ctx.debug_staged_frame(b)) for b in range(nb)]
        with pytest.raises(capi.IngvioError):
            stage(ctx, [valid(0), dict(table, **d), valid(2)], steps, cases[0][2], use_async=use_async)
        for b in range(nb):
            assert same_store(before[b][0], ctx.debug_tracks_read(b)), (i, b)
            assert same_staged(before[b][1], ctx.debug_staged_frame(b)), (i, b)
        assert same_results(good(ctx, cases, steps, steady), want), i
    ctx.close()


# ---- h. ingvio_tracks_create on a context that has a store -----------------------------------------------------------------------
def test_tracks_create_again_gives_an_empty_store():
    from ingvio_amd import capi
    nb, T, C, F = 2, 300, 11, 40
    ctx = stage_ctx(nb, C, F)
    with pytest.raises(capi.IngvioError):                                # no store yet
        ctx.debug_tracks_read(0)
    ctx.tracks_create(T)
    opts = frame_opts()
    steps = [raw_step(b) for b in range(nb)]
    r = np.random.default_rng(5)
    fill = [dict(append=3, obs_track=r.permutation(T), obs_uv=r.normal(size=(T, 4)), pf_track=r.permutation(T), pf=r.normal(size=(T, 3))) for _ in range(nb)]
    stage(ctx, fill, steps, opts)
    assert all(ctx.debug_tracks_read(b)[0].all() for b in range(nb))
    for b in (-1, nb):
        with pytest.raises(capi.IngvioError):
            ctx.debug_tracks_read(b)
        with pytest.raises(capi.IngvioError):
            ctx.debug_staged_frame(b)
    ctx.tracks_create(T)                                                 # the same size: cleared in place
    for b in range(nb):
        mask, uv, pf = ctx.debug_tracks_read(b)
        assert mask.shape == (T,) and not mask.any() and not pf.any()
    stage(ctx, fill, steps, opts)
    ctx.tracks_create(64)                                                # another size: a new, empty store
    for b in range(nb):
        mask, uv, pf = ctx.debug_tracks_read(b)
        assert mask.shape == (64,) and uv.shape == (64, C, 4) and pf.shape == (64, 3)
        assert not mask.any() and not pf.any() and not uv.any()
    with pytest.raises(capi.IngvioError):                                # the old size's track numbers are gone with it
        stage(ctx, [dict(append=0, obs_track=[64], obs_uv=np.zeros((1, 4)))] * nb, steps, opts)
    model = TrackStoreModel(64, C)
    d = dict(append=C - 1, obs_track=[63, 0], obs_uv=r.normal(size=(2, 4)))
    stage(ctx, [d] * nb, steps, opts)
    model.apply(d)
    for b in range(nb):
        check(ctx, b, model, d, b)
    ctx.close()


# ---- i. stages pipelined under the running frame ---------------------------------------------------------------------------------
def test_pipelined_stages_leave_the_serial_sequence_of_stores():
    nb, C, F, T, n_frames = 3, 11, 40, 300, 7

    def prepare():
        ctx, cases = build(nb, C, F, 700)
        ctx.snapshot()
        ctx.tracks_create(T)
        steps = [c[1] for c in cases]
        tracks = track_numbers(nb, T, F, 30)
        deltas = [window_deltas(cases[b], tracks[b], C) for b in range(nb)]
        for s in range(C):
            stage(ctx, [deltas[b][s] for b in range(nb)], steps, cases[0][2])
        return ctx, cases, steps, tracks, deltas

    ctx, cases, steps, tracks, deltas = prepare()
    models = [TrackStoreModel(T, C) for _ in range(nb)]
    for b in range(nb):
        for d in deltas[b]:
            models[b].apply(d)
    # steady-state frames: slot 0 leaves, a new column arrives at the top; the update uses the tracks that still hold four observations,
    # anchored at their oldest one (the caller's bookkeeping, here read off the model)
    frames, stores = [], []
    for i in range(n_frames):
        ds = []
        for b in range(nb):
            r = np.random.default_rng(100 * i + b)
            last = deltas[b][C - 1]
            d = dict(drop=[0], append=C - 1, obs_track=last["obs_track"], obs_uv=last["obs_uv"] + 1e-4 * r.normal(size=last["obs_uv"].shape),
                     clone_idx=last["clone_idx"], clone_R=last["clone_R"], clone_p=last["clone_p"])
            models[b].apply(d)
            use = [t for t in tracks[b] if len(models[b].obs[int(t)]) >= 4]
            d.update(feat_track=np.array(use, dtype=np.int32), feat_anchor=np.array([min(models[b].obs[int(t)]) for t in use], dtype=np.int32),
                     feat_dof=np.array([len(models[b].obs[int(t)]) - 1 for t in use], dtype=np.int32))
            ds.append(d)
        frames.append(ds)
        stores.append([flat(m) for m in models])
    assert len(frames[-1][0]["feat_track"]) > 0

    def read():
        return [ctx.debug_tracks_read(b) for b in range(nb)]

    piped = []
    stage(ctx, frames[0], steps, cases[0][2], use_async=True)
    piped.append(read())
    for i in range(n_frames - 1):                                        # run(i); stage_async(i + 1); fetch(i)
        ctx.frame_run(restore_prior=True)
        stage(ctx, frames[i + 1], steps, cases[0][2], use_async=True)
        piped.append(read())
        ctx.frame_fetch()
    ctx.close()
    ctx, cases, steps, _, _ = prepare()
    serial = []
    for i in range(n_frames):
        stage(ctx, frames[i], steps, cases[0][2])
        serial.append(read())
        ctx.frame_run(restore_prior=True)
        ctx.frame_fetch()
    ctx.close()
    for i in range(n_frames):
        for b in range(nb):
            assert_store_equal(piped[i][b], stores[i][b], C, ("pipelined", i, b))
            assert_store_equal(serial[i][b], stores[i][b], C, ("serial", i, b))
            assert_store_equal(piped[i][b], serial[i][b], C, ("pipelined / serial", i, b))
