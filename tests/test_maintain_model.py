"""The host model of the MSCKF anchor change and the invalid-feature erase (ingvio_amd/closed_loop_maintain.py) against
oracle/stream_filter.py's change_anchor + erase_invalid on the same features, in both modes' thresholds, and the conditions the decoy
scenario of the GPU loops has to meet, checked on the oracle alone: the tables follow the oracle's IMU integration of the loops' inputs
without any update, which is the true trajectory to the IMU noise.  No update runs here, so the condition that half of each frame's
listed features still pass the gate is not checked in this file: tests/test_gpu_tracks_maintain.py asserts it on the real gate."""
import copy

import numpy as np
import pytest

from ingvio_amd.closed_loop import host_propagate
from ingvio_amd.closed_loop_maintain import (DECOYS, ERASED, ERASED_INVALID, ERASED_MOVE, ERASED_UNTRIANGULATED, INVALID, KEEP, MIN_DEPTH,
                                             MOVE_MIN_DEPTH, MOVED, Anchors, Book, add_decoys, decoy_points, depth_at, host_maintain,
                                             maintain_words, make_table)
from ingvio_amd.closed_loop_update import HostStore, make_keyframe_loop, make_update_loop

F = 24


def oracle_verdicts(table, points, anchors, leaving, move_min_depth):
    """change_anchor + erase_invalid of oracle/stream_filter.py on a map of MSCKF features built from the same table, points and
    anchors; -> {track: verdict}"""
    from oracle import stream_filter as sf
    flt = object.__new__(sf.Filter)
    var = {}
    for q, sl in enumerate(table.clones):
        v = sf.Var("se3", 6)
        v.R, v.p = table.slots[sl]["R"].copy(), table.slots[sl]["p"].copy()
        var[sl] = (q, v)
    flt.sw = {float(q): v for q, v in var.values()}
    flt.map, flt.landmarks = {}, {}
    for t, sl in anchors.items():
        fi = sf.Feature()
        fi.id, fi.anchor, fi.is_tri = t, var[sl][1], t in points
        if t in points:
            fi.pf = np.array(points[t])
        flt.map[t] = fi
    tri = {t: fi.is_tri for t, fi in flt.map.items()}
    tr = {}
    flt.change_anchor([float(var[sl][0]) for sl in leaving], move_min_depth, tr)
    flt.erase_invalid(tr)
    out = {}
    for t in anchors:
        if t in tr["anchor_erased"]:
            out[t] = ERASED_MOVE if tri[t] else ERASED_UNTRIANGULATED
        elif t in tr["invalid_erased"]:
            out[t] = ERASED_INVALID
        else:
            out[t] = MOVED if t in tr["anchor_moved"] else KEEP
    return out, {t: (None if fi.anchor is None else next(sl for sl, (_, v) in var.items() if v is fi.anchor)) for t, fi in flt.map.items()}


@pytest.mark.parametrize("mode", ["sw", "kf"])
def test_host_model_equals_the_oracle_on_random_maps(mode):
    """random windows, points on both sides of both thresholds, anchors on every clone, one or two clones leaving, features with and
    without a point: verdicts and the surviving features' anchors equal"""
    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(20):
        C = int(rng.integers(3, 10))
        table, _, _ = make_table(rng, C)
        leaving = [table.clones[q] for q in sorted(rng.choice(C - 1, size=1 + trial % 2, replace=False))]
        store, an = HostStore(60, 1), Anchors()
        for t in range(60):
            an.slot[t] = table.clones[int(rng.integers(0, C))]
            if t % 5:
                a = table.slots[table.clones[int(rng.integers(0, C))]]
                store.points[t] = a["R"] @ np.array([rng.normal(), rng.normal(), rng.uniform(-2.0, 3.0)]) + a["p"]
        store.mask[:] = 1
        want, anchors_after = oracle_verdicts(table, store.points, dict(an.slot), leaving, MOVE_MIN_DEPTH[mode])
        got = host_maintain(table, store, an, leaving, MOVE_MIN_DEPTH[mode])
        assert {t: v for t, (v, _) in got.items()} == want
        assert an.slot == {t: s for t, s in anchors_after.items()}
        assert all((store.mask[t] == 0) == (v in ERASED) and ((t in store.points) == (t % 5 != 0 and v not in ERASED)) for t, v in want.items())
        seen |= set(want.values())
    assert seen == {KEEP, MOVED, ERASED_UNTRIANGULATED, ERASED_MOVE, ERASED_INVALID}


def play(cases, mode):
    """the decoy loop on host tables alone: per frame the new clone (oracle IMU integration), the step on the oracle and on the host
    model before the clones leave, the words of the call; -> [(f, b, track, verdict, depths compared)]"""
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    books, stores = [Book(c) for c in cases], [HostStore(F + DECOYS, 12) for _ in cases]
    rows = []
    for f in range(len(cases[0]["frames"])):
        host_propagate(cases, tabs, f, marg=False)
        for b, (c, t, bk, st) in enumerate(zip(cases, tabs, books, stores)):
            fr = c["frames"][f]
            bk.staged()
            assert bk.ints.clones == t.clones
            st.apply(fr["delta"])
            decoy_points(st, fr)
            leaving = [t.clones[q] for q in fr["decoy"]["leave_pos"]]
            near = []
            for tr, sl in bk.an.slot.items():                            # every depth the two steps may compare with a threshold
                if tr in st.points:
                    s = t.clones[-1] if sl in leaving else sl          # (a moved track is tested at its new anchor both times)
                    near.append(depth_at(t.slots[s]["R"], t.slots[s]["p"], st.points[tr]))
            want, _ = oracle_verdicts(t, st.points, dict(bk.an.slot), leaving, MOVE_MIN_DEPTH[mode])
            got = host_maintain(t, st, bk.an, leaving, MOVE_MIN_DEPTH[mode])
            assert {k: v for k, (v, _) in got.items()} == want, (f, b)
            for s in leaving:
                t.marginalize(t.slots[s]["idx"])
            assert bk.leave(fr) == leaving and bk.ints.clones == t.clones
            tracks, words = maintain_words(t.clones, Anchors(dict(bk.an.slot)), [])
            assert all((w >> 16) & 0xff < len(t.clones) for w in words)
            rows += [(f, b, tr, v, near) for tr, v in want.items()]
    return rows


@pytest.mark.parametrize("mode,nb,nfr", [("sw", 6, 9), ("kf", 4, 6)])
def test_decoy_scenario_meets_its_conditions(mode, nb, nfr):
    """every verdict class at least 3 times per loop and once per filter; no compared depth within 1 m of a threshold (the GPU tests
    exempt nothing: the filters' poses differ from these by centimetres); the restarted track is erased and observed again"""
    if mode == "sw":
        cases = make_update_loop(nb, nfr, F, first_tri=True, windows=(5, 6, 7, 8))
    else:
        cases = make_keyframe_loop(nb, nfr, F, first_tri=True, windows=(5, 6, 7, 8))
    add_decoys(cases, F, mode)
    rows = play(cases, mode)
    for v in (KEEP, MOVED, ERASED_UNTRIANGULATED, ERASED_MOVE, ERASED_INVALID):
        hits = [r for r in rows if r[3] == v]
        assert len(hits) >= 3 and {r[1] for r in hits} == set(range(nb)), (v, len(hits))
    for f, b, tr, v, near in rows:
        for d in near:
            assert min(abs(d - MIN_DEPTH), abs(d - MOVE_MIN_DEPTH[mode])) > 1.0, (f, b, tr, d)
    for b, c in enumerate(cases):
        gone = [f for f, bb, tr, v, _ in rows if bb == b and tr == F + INVALID and v == ERASED_INVALID]
        assert len(gone) >= 2 and gone[0] == 0
        assert all(F + INVALID in c["frames"][f]["delta"]["obs_track"] for f in range(1, nfr))      # observed again under the same number
        assert any(v == KEEP for f, bb, tr, v, _ in rows if bb == b and tr == F + INVALID and gone[0] < f < gone[1])
