"""ingvio_tracks_maintain (k_tracks_maintain, kernels_tracks.hip): the MSCKF anchor change and the invalid-feature erase on
the device-resident track store, against the host model of ingvio_amd/closed_loop_maintain.py evaluated on the values read back from
the device (ingvio_nominal_get, ingvio_debug_tracks_read, ingvio_debug_tracks_flags).

Verdicts are compared with equality - the test's depths keep clear of the thresholds except where they sit on them exactly - and depths
to 1e-14 |p_f - p_a|: three products and three sums on identical inputs differ by at most ~1.3e-15 of that with FMA contraction."""
import copy

import numpy as np
import pytest

from ingvio_amd.closed_loop_maintain import (ERASED, ERASED_INVALID, ERASED_MOVE, ERASED_UNTRIANGULATED, KEEP, MIN_DEPTH, MOVED, Anchors,
                                             depth_at, host_landmarks, host_maintain, make_table)
from ingvio_amd.closed_loop_update import HostStore, host_table_of
from test_gpu_track_store import frame_opts, full, raw_step, same_bits

pytestmark = pytest.mark.gpu

T_MAX = 300
LEAVING = -7                                                             # a table slot that no longer exists: the anchor that left


def make_ctx(tables, c_max):
    from ingvio_amd import capi
    n_hi = max(n for _, n, _ in tables)
    ctx = capi.Context(batch=len(tables), n_max=((n_hi + 6 + 15) // 16) * 16, c_max=c_max, f_max=16, m_max=64)
    rng = np.random.default_rng(77)
    for b, (t, n, _) in enumerate(tables):
        A = rng.normal(size=(n, n))
        ctx.cov_set(b, 1e-3 * (A @ A.T / n + 0.1 * np.eye(n)))
    ctx.nominal_create(40)
    ctx.nominal_set(0, [t.as_dict() for t, _, _ in tables])
    ctx.tracks_create(T_MAX)
    return ctx


def stage(ctx, deltas, b0=0):
    """the deltas on the store through ingvio_frame_stage_tracks (host-fed values: the table plays no part, nothing runs)"""
    steps = [raw_step(b0 + i) for i in range(len(deltas))]
    ctx.frame_stage_tracks_prepare(b0, steps, [full(d) for d in deltas], frame_opts(), steps[0]["sigma"], 1, 0.2, 0.2, max_accept=0, compress_rule=1)()


def device_state(ctx):
    """everything the call must leave alone, bit for bit: per filter (mask, uv, pf, flags), the tables, P, n"""
    st = [ctx.debug_tracks_read(b) + (ctx.debug_tracks_flags(b),) for b in range(ctx.batch)]
    return st, ctx.nominal_get(), [ctx.cov_get(b) for b in range(ctx.batch)], [ctx.n(b) for b in range(ctx.batch)]


def same_store(a, b, but=()):
    keep = np.ones(len(a[0]), dtype=bool)
    keep[list(but)] = False
    return (np.array_equal(a[0][keep], b[0][keep]) and same_bits(a[1][keep], b[1][keep]) and same_bits(a[2][keep], b[2][keep]) and
            np.array_equal(a[3][keep], b[3][keep]))


def same_nominal(a, b):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("kind", "idx", "anchor", "clone_var")) and \
        all(same_bits(x["val"], y["val"]) for x, y in zip(a, b))


def same_rest(s0, s1):
    return same_nominal(s0[1], s1[1]) and all(p.shape == q.shape and same_bits(p, q) for p, q in zip(s0[2], s1[2])) and s0[3] == s1[3]


def host_expect(nom, store, entries, move_min_depth):
    """host_maintain on the read-back values; entries: (track, window position, move) - a moved entry names the newest clone.
    -> ({track: (verdict, depth)}, the model store after the step)"""
    t = host_table_of(nom)
    mask, _, pf, has = store
    hs = HostStore(len(mask), 1)
    hs.mask[:] = mask
    hs.points = {int(k): pf[k].copy() for k in np.flatnonzero(has)}
    an = Anchors({tr: (LEAVING if mv else t.clones[pos]) for tr, pos, mv in entries})
    return host_maintain(t, hs, an, [LEAVING], move_min_depth), hs, t


def check_call(ctx, b0, lists, move_min_depth, begin_end=False):
    """one call over filters b0 .. against the model, and what it must leave alone; -> verdict counts"""
    from ingvio_amd import capi
    s0 = device_state(ctx)
    blocks = [dict(tracks=[capi.maintain_word(*e) for e in es]) for es in lists]
    if begin_end:
        ctx.tracks_maintain_begin(b0, blocks, move_min_depth, MIN_DEPTH)
        ctx.odom_begin(0, ctx.batch); ctx.odom_end()                   # (other work between the halves)
        out = ctx.tracks_maintain_end()
    else:
        out = ctx.tracks_maintain(b0, blocks, move_min_depth, MIN_DEPTH)
    s1 = device_state(ctx)
    assert same_rest(s0, s1)
    counts = np.zeros(5, dtype=int)
    for b in range(ctx.batch):
        if not b0 <= b < b0 + len(lists) or not lists[b - b0]:
            assert same_store(s0[0][b], s1[0][b]), b                     # an untouched filter, or one with an empty list
            continue
        es, o = lists[b - b0], out[b - b0]
        want, hs, t = host_expect(s0[1][b], s0[0][b], es, move_min_depth)
        gone = []
        for j, (tr, pos, mv) in enumerate(es):
            v, d = want[tr]
            assert o["verdict"][j] == v, (b, j, tr, pos, mv, o["verdict"][j], v, o["depth"][j], d)
            counts[v] += 1
            if d is None:
                assert o["depth"][j] == 0.0
            elif np.isfinite(d):
                a = t.slots[t.clones[pos]]
                assert abs(o["depth"][j] - d) <= 1e-14 * np.linalg.norm(s0[0][b][2][tr] - a["p"]), (b, j, o["depth"][j], d)
            else:
                assert np.isnan(o["depth"][j]) == np.isnan(d) and (np.isnan(d) or o["depth"][j] == d)
            if v in ERASED:
                gone.append(tr)
        m1, _, pf1, has1 = s1[0][b]
        assert not m1[gone].any() and not has1[gone].any()
        assert np.array_equal(m1, hs.mask) and set(np.flatnonzero(has1)) == set(hs.points)
        assert same_bits(pf1, s0[0][b][2])                               # an erased track's point stays where it was: only the flag goes
        assert same_store(s0[0][b], s1[0][b], but=gone)
    return counts


def seed_delta(rng, table, n_pts, special=None):
    """tracks 0 .. n_pts - 1 get a point (depths of 0.5 .. 9 m on either side of the window's clones), every track an observation"""
    cl = [table.slots[s] for s in table.clones]
    pts = np.zeros((n_pts, 3))
    for k in range(n_pts):
        a = cl[k % len(cl)]
        z = rng.uniform(0.5, 9.0) * (-1.0 if k % 3 == 0 else 1.0)
        pts[k] = a["R"] @ np.array([rng.normal(), rng.normal(), z]) + a["p"]
    for k, p in (special or {}).items():
        pts[k] = p
    return dict(append=0, obs_track=list(range(T_MAX)), obs_uv=rng.normal(size=(T_MAX, 4)), pf_track=list(range(n_pts)), pf=pts)


def entries_of(rng, tracks, C):
    """(track, window position, move): positions 0, last and between; a moved track names the newest clone"""
    out = []
    for j, tr in enumerate(tracks):
        mv = j % 4 == 1
        out.append((int(tr), C - 1 if mv or j % 3 == 0 else (0 if j % 3 == 1 else int(rng.integers(0, C))), int(mv)))
    return out


@pytest.mark.parametrize("c_max,move_min_depth", [(12, 0.3), (12, 0.0), (20, 0.0)])
def test_one_call_equals_the_host_model(c_max, move_min_depth):
    """3 filters (windows 5, c_max, 7), t_max = 300: list lengths 1, 0 and 255, then a partial range with 256 and 257 through _begin /
    _end beside an untouched filter, then 300; anchor_pos 0 and last; an identity anchor with p_f.z exactly 0.3, 0.2, 0.0 and the next
    double above each, as kept and as moved tracks; tracks without a point, kept and moved; a freed and re-pointed track; NaN and
    infinities in a point"""
    rng = np.random.default_rng(11 + c_max)
    tables = [make_table(rng, 5, identity_ends=True), make_table(rng, c_max), make_table(rng, 7)]
    ctx = make_ctx(tables, c_max)
    zs = [0.3, np.nextafter(0.3, 1.0), 0.2, np.nextafter(0.2, 1.0), 0.0, np.nextafter(0.0, 1.0)]
    special = {k: np.array([0.4, -0.7, z]) for k, z in enumerate(zs + zs)}            # tracks 0..5 kept, 6..11 moved, at the identity
    special.update({12: np.array([np.nan, 0.0, 1.0]), 13: np.array([0.0, 0.0, np.inf]), 14: np.array([0.0, 0.0, -np.inf]), 15: np.array([1.0, np.nan, np.nan])})
    n_pts = 280                                                          # tracks 280 .. 299 never get a point
    stage(ctx, [seed_delta(rng, t, n_pts, special if b == 0 else None) for b, (t, _, _) in enumerate(tables)])
    stage(ctx, [dict(free=[20, 21, 22], pf_track=[21], pf=np.array([[0.1, 0.2, 5.0]]))] * 3)
    stage(ctx, [dict(pf_track=[22], pf=np.array([[0.1, 0.2, -5.0]]))] * 3)
    has = ctx.debug_tracks_flags(0)
    assert has[:20].all() and not has[20] and has[21] and has[22] and has[23:n_pts].all() and not has[n_pts:].any()
    ident = [(k, 0, 0) for k in range(6)] + [(k, 4, 1) for k in range(6, 12)] + [(k, 4 if k % 2 else 0, k % 2) for k in range(12, 16)]
    first = ident + entries_of(rng, list(range(16, 251)) + [285, 286, 287, 288], 5)
    assert len(first) == 255
    total = check_call(ctx, 0, [first, [], [(7, 6, 1)]], move_min_depth)
    # the exact thresholds at the identity anchor: <= erases, the next double above does not
    h0 = ctx.debug_tracks_flags(0)
    alive = [bool(h0[k]) for k in range(12)]
    assert alive[:6] == [True, True, False, True, False, False]          # kept: 0.3, 0.3+ stay; 0.2 goes, 0.2+ stays; 0.0, 0.0+ go
    assert alive[6:] == ([False, True, False, False, False, False] if move_min_depth == 0.3 else [True, True, False, True, False, False])
    assert h0[12] and h0[13] and not h0[14] and h0[15]                   # NaN keeps (NaN <= x is false), +inf keeps, -inf erases
    total += check_call(ctx, 1, [entries_of(rng, range(256), c_max), entries_of(rng, list(range(43, 300)), 7)], move_min_depth, begin_end=True)
    stage(ctx, [seed_delta(rng, tables[0][0], n_pts)], b0=0)
    total += check_call(ctx, 0, [entries_of(rng, rng.permutation(T_MAX), 5)], move_min_depth)
    assert total.min() >= 3, total                                       # every verdict occurred
    ctx.close()


def test_a_following_frame_drops_an_erased_track_or_restarts_it():
    """after an erasure: a stage that lists the track gathers an empty mask (the update drops it as it drops a failed triangulation), a
    stage that appends to it leaves a track of that one observation and no point"""
    from ingvio_amd import capi
    rng = np.random.default_rng(5)
    tables = [make_table(rng, 5, identity_ends=True)]
    ctx = make_ctx(tables, 12)
    pts = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 3.0], [0.0, 0.0, -2.0]])
    stage(ctx, [dict(append=0, obs_track=[0, 1, 2], obs_uv=rng.normal(size=(3, 4)), pf_track=[0, 1, 2], pf=pts)])
    stage(ctx, [dict(append=1, obs_track=[0, 1, 2], obs_uv=rng.normal(size=(3, 4)))])
    out = ctx.tracks_maintain(0, [dict(tracks=[capi.maintain_word(t, 0, 0) for t in range(3)])])
    assert list(out[0]["verdict"]) == [ERASED_INVALID, KEEP, ERASED_INVALID]
    cl = tables[0][0]
    ct = dict(clone_idx=[cl.slots[s]["idx"] for s in cl.clones[:3]], clone_R=np.stack([np.eye(3).reshape(9)] * 3), clone_p=np.zeros((3, 3)))
    uv2 = rng.normal(size=(2, 4))
    stage(ctx, [dict(ct, append=2, obs_track=[1, 2], obs_uv=uv2, feat_track=[0, 1, 2], feat_anchor=[0, 0, 2], feat_dof=[2, 2, 0])])
    sf = ctx.debug_staged_frame(0)
    assert list(sf["obs_mask"][:3]) == [0, 7, 4]                         # listed and erased: nothing; kept: three; restarted: the new one
    mask, uv, _ = ctx.debug_tracks_read(0)
    has = ctx.debug_tracks_flags(0)
    assert list(mask[:3]) == [0, 7, 4] and list(has[:3]) == [0, 1, 0] and np.array_equal(uv[2, 2], uv2[1])
    ctx.close()


def test_landmark_list_is_report_only():
    """in-state landmarks by table slot: the verdicts of the host model on the read-back table, the table, the store and P unchanged"""
    rng = np.random.default_rng(9)
    tables = [make_table(rng, 5, n_lm=7), make_table(rng, 6, n_lm=0), make_table(rng, 8, n_lm=12)]
    for t, _, lms in tables[:1]:                                         # one landmark exactly on the threshold of an identity anchor, one above
        a = t.slots[t.slots[lms[0]]["anchor"]]
        a["R"], a["p"] = np.eye(3), np.zeros(3)
        t.slots[lms[0]]["p"] = np.array([1.0, 2.0, MIN_DEPTH])
        t.slots[lms[5]]["p"] = np.array([1.0, 2.0, np.nextafter(MIN_DEPTH, 1.0)])
    ctx = make_ctx(tables, 12)
    s0 = device_state(ctx)
    out = ctx.tracks_maintain(0, [dict(lm_slot=lms[::-1]) for _, _, lms in tables])
    s1 = device_state(ctx)
    assert same_rest(s0, s1) and all(same_store(a, b) for a, b in zip(s0[0], s1[0]))
    seen = set()
    for b, (_, _, lms) in enumerate(tables):
        want = host_landmarks(host_table_of(s0[1][b]), lms[::-1])
        assert list(out[b]["lm_verdict"]) == want, b
        seen |= set(want)
    assert seen == {KEEP, ERASED_INVALID}
    assert out[0]["lm_verdict"][-1] == ERASED_INVALID and out[0]["lm_verdict"][1] == KEEP
    ctx.close()


def test_every_refusal_changes_nothing():
    """each refusal with its code, then the state bit for bit that of a context that was never refused anything"""
    from ingvio_amd import capi
    rng = np.random.default_rng(21)
    tables = [make_table(rng, 5, n_lm=2), make_table(rng, 6, n_lm=2)]
    w = capi.maintain_word

    def fresh():
        ctx = make_ctx(copy.deepcopy(tables), 12)
        stage(ctx, [seed_delta(np.random.default_rng(3), t, 200) for t, _, _ in tables])
        return ctx

    def good(ctx):
        return ctx.tracks_maintain(0, [dict(tracks=[w(t, t % 5, 0) for t in range(0, 250, 3)], lm_slot=tables[b][2]) for b in range(2)])

    def no(ctx, code, fn):
        with pytest.raises(capi.IngvioError) as e:
            fn()
        assert e.value.code == code, (e.value.code, code, str(e.value))
    ctx = fresh()
    s0 = device_state(ctx)
    ok = [dict(tracks=[w(1, 0, 0)])] * 2
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(2, ok[:1]))                                              # a bad range
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(1, ok))
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(0, [dict(tracks=[w(t, 0, 0) for t in range(T_MAX)] + [w(0, 0, 0)])]))      # longer than t_max
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(0, ok, list_cap=0))                                      # longer than list_cap
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(0, [dict(tracks=[w(T_MAX, 0, 0)])]))                      # a track out of range
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(0, [dict(tracks=[w(4, 0, 0), w(5, 1, 0), w(4, 2, 1)])]))  # named twice
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(0, [dict(tracks=[w(4, 0, 0) | (1 << 25)])]))             # bits above move
    no(ctx, capi.E_NOT_IN_STATE, lambda: ctx.tracks_maintain(0, [dict(tracks=[w(4, 5, 0)])]))                # beyond the window (5 clones)
    no(ctx, capi.E_NOT_IN_STATE, lambda: ctx.tracks_maintain(1, [dict(tracks=[w(4, 6, 1)])]))
    no(ctx, capi.E_NOT_IN_STATE, lambda: ctx.tracks_maintain(0, [dict(lm_slot=[tables[0][0].clones[0]])]))   # no landmark
    no(ctx, capi.E_NOT_IN_STATE, lambda: ctx.tracks_maintain(0, [dict(lm_slot=[39])]))                       # a free slot
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain(0, [dict(lm_slot=tables[0][2])], lm_cap=1))
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain_end())                                                   # _end without _begin
    ctx.tracks_maintain_begin(0, [dict(), dict()])                                                           # every list empty: pending all the same
    no(ctx, capi.E_ARG, lambda: ctx.tracks_maintain_begin(0, ok))                                            # _begin while one is pending
    assert [len(o["verdict"]) + len(o["lm_verdict"]) for o in ctx.tracks_maintain_end()] == [0, 0]
    # NULL where data is needed: straight at the export
    o = capi.MaintainOpts(); o.move_min_depth = 0.0; o.min_depth = 0.2; o.list_cap = 4; o.lm_cap = 4
    blk = (capi.MaintainBlock * 1)(); blk[0].n_tracks = 1
    assert ctx.L.ingvio_tracks_maintain_begin(ctx.h, 0, 1, blk, None) == capi.E_ARG
    assert ctx.L.ingvio_tracks_maintain_begin(ctx.h, 0, 1, None, capi.C.byref(o)) == capi.E_ARG
    assert ctx.L.ingvio_tracks_maintain_begin(ctx.h, 0, 1, blk, capi.C.byref(o)) == capi.E_ARG
    one = capi.i32([w(1, 0, 0)]); blk[0].tracks = capi._i(one)
    assert ctx.L.ingvio_tracks_maintain(ctx.h, 0, 1, blk, capi.C.byref(o), None, None, None) == capi.E_ARG
    s1 = device_state(ctx)
    assert same_rest(s0, s1) and all(same_store(a, b) for a, b in zip(s0[0], s1[0]))
    res = good(ctx)
    s2 = device_state(ctx)
    ctx.close()
    # without a table, without a store
    c2 = capi.Context(batch=1, n_max=64, c_max=12, f_max=16, m_max=64)
    no(c2, capi.E_ARG, lambda: c2.tracks_maintain(0, ok[:1]))
    c2.nominal_create(8)
    no(c2, capi.E_ARG, lambda: c2.tracks_maintain(0, ok[:1]))
    c2.close()
    ctx = fresh()
    res2 = good(ctx)
    s3 = device_state(ctx)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(res, res2) for k in ("verdict", "lm_verdict")) and all(same_bits(a["depth"], b["depth"]) for a, b in zip(res, res2))
    assert same_rest(s2, s3) and all(same_store(a, b) for a, b in zip(s2[0], s3[0]))
    ctx.close()


# ---- the call in the two-update closed loops ----------------------------------------------------------------------------------------
F = 24


def loop_cases(mode):
    from ingvio_amd.closed_loop_maintain import add_decoys
    from ingvio_amd.closed_loop_update import make_keyframe_loop, make_update_loop
    if mode == "sw":
        return add_decoys(make_update_loop(6, 9, F, first_tri=True, windows=(5, 6, 7, 8)), F, mode)
    return add_decoys(make_keyframe_loop(4, 6, F, first_tri=True, windows=(5, 6, 7, 8)), F, mode)


def loop_ctx_of(cases, table):
    from ingvio_amd import capi
    from ingvio_amd.closed_loop_maintain import DECOYS
    n_max = max(c["P"].shape[0] for c in cases) + 18                     # (the key-frame window grows by two clones before two leave)
    ctx = capi.Context(batch=len(cases), n_max=((n_max + 15) // 16) * 16, c_max=12, f_max=F, m_max=64)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c["P"])
    ctx.tracks_create(F + DECOYS)
    if table:
        ctx.nominal_create(48)
        ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    return ctx


def device_loop(ctx, cases, frames, free_running, pipelined):
    from ingvio_amd.closed_loop import DeviceLoop
    from ingvio_amd.closed_loop_maintain import Book, decoy_form
    from ingvio_amd.closed_loop_update import two_update_entries, update_stage
    out = {}
    out["books"] = books = [Book(c) for c in cases]
    form = decoy_form(cases, books, out, free_running)
    return DeviceLoop(ctx, cases, two_update_entries(frames), form, pipelined, update_stage=update_stage), out


@pytest.mark.parametrize("mode", ["sw", "kf"])
def test_loops_synchronous_form_equals_host_loop_and_free_running_form(mode):
    """mode sw: 6 filters x 9 camera frames, windows 5 .. 8, k in {1, 9, 10, 33}, the sliding-window thresholds; mode kf: 4 filters x 6
    camera frames in the key-frame cadence, ingvio_nominal_tail dropping two clones behind every other frame, the key-frame thresholds.
    The synchronous call in the serial device loop against the host loop in the reference's order, in every frame: verdicts equal,
    depths to 1e-7 m, accept masks, rows, flags and points of both updates equal, dx, table and P to 1e-9.  The free-running form in the
    pipelined loop (_begin behind run(i), _end behind run(i + 1)) against the synchronous one: verdicts and accept masks equal in every
    frame, dx to 1e-9, the final table, P and store flags, and - in a serial loop with the same order of calls - table and P of every frame
    to 1e-9.  A snapshot restored replays the free-running loop.
    Track REAL is listed by every first update: accepted in camera frame POISON_FRAME, erased behind it (its point overwritten by the
    second update's delta), it drops out of the next two first updates as accepted = 0 in every form, while (sliding-window loop) the loop
    without maintenance accepts it there and every OTHER feature of that update comes out bit for bit the same; the host's bookkeeping of masks
    and anchors (Book) equals the device's masks in every frame, also when the verdicts arrive behind the next stage."""
    from conftest import rel_err as rel
    from ingvio_amd.closed_loop_maintain import Book, DECOYS, MOVE_MIN_DEPTH, POISON_FRAME, REAL, decoy_points
    from ingvio_amd.closed_loop_update import device_loop_update, host_step_update, host_tail_drop, staged_clones
    from nominal_helpers import assert_table
    from test_gpu_nominal_first_tri import assert_loop_frame, listed
    cases = loop_cases(mode)
    nb, nfr = len(cases), len(cases[0]["frames"])
    cd, ch = loop_ctx_of(cases, True), loop_ctx_of(cases, False)
    loop, sync = device_loop(cd, cases, range(nfr), False, False)
    staged = {}
    loop.staged_hook = lambda lp, i: staged.__setitem__(i, staged_clones(lp.ctx))
    loop.start()
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    hcases = copy.deepcopy(cases)                                        # the host loop's own inputs: erased tracks enter the next delta's free_tracks
    books, stores, points = [Book(c) for c in cases], [HostStore(F + DECOYS, 12) for _ in cases], [dict() for _ in cases]
    serial, counts, states = [], np.zeros(5, dtype=int), []
    for f in range(nfr):
        d1, d2 = loop.frame(2 * f), loop.frame(2 * f + 1)
        serial.append((d1, d2))
        for bk in books:
            bk.staged()
        host = host_step_update(ch, hcases, tabs, f, points, stores=stores, staged=(staged[2 * f], staged[2 * f + 1]))
        if mode == "kf":
            host_tail_drop(ch, hcases, tabs, f)
        assert_loop_frame(cases, f, host, (d1, d2), nb)
        n1 = listed(cases, f)[0]
        if n1:
            assert 2 * d1[1][:, :n1].sum(axis=1).min() >= n1, f           # in every filter half of the listed features pass the gate
        nom, Ps = cd.nominal_get(), [cd.cov_get(b) for b in range(nb)]
        states.append((nom, Ps))
        for b, (c, t, bk, st) in enumerate(zip(cases, tabs, books, stores)):
            fr = c["frames"][f]
            decoy_points(st, fr)
            leaving = bk.leave(fr)
            assert bk.ints.clones == t.clones, (f, b)
            want = host_maintain(t, st, bk.an, leaving, MOVE_MIN_DEPTH[mode])
            tracks, verdicts, depths = sync[f][b]
            assert sorted(want) == tracks and [want[tr][0] for tr in tracks] == verdicts, (f, b, want, verdicts)
            assert all(want[tr][1] is None or abs(want[tr][1] - d) <= 1e-7 for tr, d in zip(tracks, depths)), (f, b)
            counts += np.bincount(verdicts, minlength=5)
            assert_table(nom[b], t, 1e-9, (f, b))
            Ph = ch.cov_get(b)
            assert Ph.shape == Ps[b].shape and rel(Ps[b], Ph) <= 1e-9, (f, b, rel(Ps[b], Ph))
            has = cd.debug_tracks_flags(b)
            assert {tr for tr in bk.tracked if has[tr]} == {tr for tr in st.points if tr in bk.tracked}, (f, b)
            mask = cd.debug_tracks_read(b)[0]
            assert not mask[[tr for tr in tracks if want[tr][0] in ERASED]].any()
            dbk = sync["books"][b]                                       # the device loop's own bookkeeping: anchors and masks as the device has them
            assert dbk.an.slot == bk.an.slot and [int(mask[tr]) for tr in dbk.tracked] == [dbk.mask(tr) for tr in dbk.tracked], (f, b)
            if f + 1 < nfr:
                hcases[b]["frames"][f + 1]["delta"]["free"] = list(hcases[b]["frames"][f + 1]["delta"].get("free", [])) + \
                    [tr for tr in tracks if tr < F and want[tr][0] in ERASED]
            if f == POISON_FRAME:
                assert want[REAL][0] == ERASED_INVALID, (b, want[REAL])
    assert counts.min() >= 3, counts
    # the erased track in the following updates' lists, against the loop that is never maintained
    j, g = cases[0]["frames"][POISON_FRAME + 1]["delta"]["feat_track"].index(REAL), POISON_FRAME + 1
    n1 = listed(cases, g)[0]
    others = [q for q in range(n1) if q != j]
    assert serial[POISON_FRAME][0][1][:, j].all()                                                # accepted before
    for h in (g, g + 1):
        assert not serial[h][0][1][:, j].any() and not (serial[h][0][4][:, j] == 1).any(), h    # erased: refused for want of observations, accepted = 0
    assert serial[g + 2][0][1][:, j].sum() >= nb - 1                                             # three observations again
    if mode == "sw":                                                     # (the plain two-update driver has no tail: the sliding-window loop only)
        cp = loop_ctx_of(cases, True)
        plain = device_loop_update(cp, cases, list(range(g + 1)), False)
        cp.close()
        assert plain[g][0][1][:, j].sum() >= nb - 1                      # accepted there when nothing erases it
        for k in (1, 3, 4):                                              # accept masks, points and flags of every other feature: untouched
            assert np.array_equal(serial[g][0][k][:, others], plain[g][0][k][:, others]), k
    state = cd.nominal_get(), [cd.cov_get(b) for b in range(nb)], [cd.debug_tracks_read(b) + (cd.debug_tracks_flags(b),) for b in range(nb)]
    ch.close(); cd.close()
    # the free-running form, pipelined; then the same loop again from the snapshot
    cf = loop_ctx_of(cases, True)
    cf.snapshot()
    runs = []
    for rep in range(2):
        if rep:
            cf.restore()
            cf.tracks_create(F + DECOYS)                                 # the track store, flags included, is no part of the snapshot
        loop, free = device_loop(cf, cases, range(nfr), True, True)
        runs.append((loop.run(), free))
    for f in range(nfr):
        for rep in range(2):
            out, free = runs[rep]
            assert [(t, v) for t, v, _ in free[f]] == [(t, v) for t, v, _ in sync[f]], (f, rep)
            for x, y, n in zip((out[2 * f], out[2 * f + 1]), serial[f], listed(cases, f)):
                assert np.array_equal(x[1][:, :n], y[1][:, :n]) and np.array_equal(x[2], y[2]), (f, rep)
                assert max([rel(x[0][b], y[0][b]) for b in range(nb) if y[2][b] > 0] + [0.0]) <= 1e-9, (f, rep)      # (no rows: dx is not written)
    for rep in range(2):
        for b, bk in enumerate(runs[rep][1]["books"]):                   # the lagged bookkeeping ends where the device's masks are
            mask = (cf.debug_tracks_read(b)[0] if rep else None)
            assert bk.an.slot == sync["books"][b].an.slot and (mask is None or [int(mask[tr]) for tr in bk.tracked] == [bk.mask(tr) for tr in bk.tracked]), (rep, b)
    # the same order of calls in a serial loop: table and P behind every camera frame
    cs = loop_ctx_of(cases, True)
    loop, _ = device_loop(cs, cases, range(nfr), True, False)
    loop.start()
    for f in range(nfr):
        loop.frame(2 * f), loop.frame(2 * f + 1)
        for b, nm in enumerate(cs.nominal_get()):
            assert list(nm["idx"]) == list(states[f][0][b]["idx"]) and rel(nm["val"], states[f][0][b]["val"]) <= 1e-9, (f, b)
            assert rel(cs.cov_get(b), states[f][1][b]) <= 1e-9, (f, b)
    cs.close()
    nom = cf.nominal_get()
    for b in range(nb):
        assert list(nom[b]["kind"]) == list(state[0][b]["kind"]) and list(nom[b]["idx"]) == list(state[0][b]["idx"])
        assert rel(nom[b]["val"], state[0][b]["val"]) <= 1e-9 and rel(cf.cov_get(b), state[1][b]) <= 1e-9
        m, _, _, has = state[2][b]
        assert np.array_equal(cf.debug_tracks_read(b)[0], m) and np.array_equal(cf.debug_tracks_flags(b), has)
    cf.close()


def test_device_triangulated_points_set_the_flag_and_a_pending_table_stage_refuses():
    """three camera frames of the sliding-window loop: the tracks whose points the device triangulated (none was handed over) carry the
    flag, and a call that lists them equals the host model on the read-back values; with a frame staged from the table and not yet run
    the call is refused and changes nothing, after the run it is taken"""
    from ingvio_amd import capi
    from ingvio_amd.closed_loop import nominal_stage
    cases = loop_cases("sw")
    ctx = loop_ctx_of(cases, True)
    loop, _ = device_loop(ctx, cases, range(3), False, False)
    out = loop.run()
    won = 0
    for b in range(ctx.batch):
        has = ctx.debug_tracks_flags(b)
        tri = {int(t) for j, t in enumerate(cases[b]["frames"][2]["upd"]["feat_track"]) if out[5][4][b, j] == 1}
        assert tri and all(has[t] for t in tri), b
        won += len(tri)
    n_cl = [len(nm["clone_var"]) for nm in ctx.nominal_get()]
    lists = [[(t, n_cl[b] - 1 if t % 2 else 0, t % 2) for t in range(F)] for b in range(ctx.batch)]
    counts = check_call(ctx, 0, lists, 0.0)
    assert counts[KEEP] + counts[MOVED] >= won and counts[ERASED_UNTRIANGULATED] > 0
    nominal_stage(ctx, cases, 3)()
    s0 = device_state(ctx)
    with pytest.raises(capi.IngvioError) as e:
        ctx.tracks_maintain(0, [dict(tracks=[capi.maintain_word(0, 0, 0)])])
    assert e.value.code == capi.E_ARG
    with pytest.raises(capi.IngvioError) as e:
        ctx.tracks_maintain_begin(0, [dict(tracks=[capi.maintain_word(0, 0, 0)])])
    assert e.value.code == capi.E_ARG
    s1 = device_state(ctx)
    assert same_rest(s0, s1) and all(same_store(a, b) for a, b in zip(s0[0], s1[0]))
    ctx.frame_run()
    ctx.frame_fetch()
    ctx.tracks_maintain(0, [dict(tracks=[capi.maintain_word(0, 0, 0)])])
    ctx.close()


def test_refused_between_the_halves_of_a_split_step():
    """a split frame step pending: INGVIO_E_ARG from both entry points, store, table, P and n as they were; taken behind the second half"""
    from ingvio_amd import capi, host, synth
    ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
    cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
    rng = np.random.default_rng(4)
    tables = [make_table(rng, 5), make_table(rng, 6)]
    ctx.tracks_create(T_MAX); ctx.nominal_create(40)
    ctx.nominal_set(0, [t.as_dict() for t, _, _ in tables])
    stage(ctx, [seed_delta(rng, t, 100) for t, _, _ in tables])
    ctx.snapshot()
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
    ctx.frame_run_phase(1, restore_prior=True)
    store = lambda: [ctx.debug_tracks_read(b) + (ctx.debug_tracks_flags(b),) for b in range(2)]
    s0, nom0, n0 = store(), ctx.nominal_get(), [ctx.n(b) for b in range(2)]
    blocks = [dict(tracks=[capi.maintain_word(t, 0, 0) for t in range(100)])] * 2
    for fn in (lambda: ctx.tracks_maintain(0, blocks), lambda: ctx.tracks_maintain_begin(0, blocks)):
        with pytest.raises(capi.IngvioError) as e:
            fn()
        assert e.value.code == capi.E_ARG and "split" in str(e.value)
    assert all(same_store(a, b) for a, b in zip(s0, store())) and same_nominal(nom0, ctx.nominal_get()) and n0 == [ctx.n(b) for b in range(2)]
    ctx.frame_run_phase(2)
    ctx.frame_fetch()
    out = ctx.tracks_maintain(0, blocks)
    assert all(len(o["verdict"]) == 100 for o in out) and sum(int((o["verdict"] == ERASED_INVALID).sum()) for o in out) > 0
    ctx.close()


def test_a_loop_without_the_new_exports_computes_what_it_computed_before():
    """the pipelined two-update loop that never calls ingvio_tracks_maintain, against the arrays the library recorded before the point
    flag existed (tests/golden/maintain_non_user_loop.npz): dx, accept masks, rows, points and flags of every entry, the final P,
    table and track store, bit for bit"""
    from conftest import load_golden
    from ingvio_amd.closed_loop_maintain import non_user_arrays
    want, got = load_golden("maintain_non_user_loop"), non_user_arrays()
    assert sorted(want.keys()) == sorted(got) and len(got) > 40
    for k in got:
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), k
    assert sum(int(got[k].sum()) for k in got if k.endswith("_rows")) > 0
