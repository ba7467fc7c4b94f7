"""The call order of the two-update closed loop (ingvio_amd/closed_loop_update.py), pinned without a GPU as
tests/test_closed_loop_schedule.py pins the other forms: a stand-in for capi.Context records the method names while the device loop
alternates the two kinds of frame from the table over three camera frames, and the host reference step runs one camera frame."""
import copy

import numpy as np
import pytest

from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_update as cu


class Recorder:
    """stands in for capi.Context: logs the name of every method called on it; a *_prepare method hands back a callable that logs the
    name of the stage it issues; fetches return zeros of the right shapes, the track store is empty"""

    def __init__(self, cases, F=24, c_max=12):
        self.log = []
        self.batch, self.f_max, self.c_max = len(cases), F, c_max
        self.ldp = max(c["P"].shape[0] for c in cases) + 16
        self.tables = []
        for c in cases:                                                  # the start tables with frame 0's clone appended: what a run leaves
            t = copy.deepcopy(c["table"])
            t.append_clone(c["frames"][0]["new_idx"])
            d = t.as_dict()
            self.tables.append(dict(d, kind=np.array(d["kind"]), idx=np.array(d["idx"]), anchor=np.array(d["anchor"])))

    def result(self, name):
        B, n, F = self.batch, self.ldp, self.f_max
        if name in ("frame_fetch", "frame_fetch_end"):
            return np.zeros((B, n)), np.zeros((B, F), dtype=np.int32), np.zeros(B, dtype=np.int32)
        if name == "frame_fetch_tri":
            return np.zeros((B, F, 3)), np.zeros((B, F), dtype=np.int32)
        if name == "msckf_update_tri":
            return (np.zeros((B, n)), np.zeros((B, F), dtype=np.int32), np.zeros((B, F)), np.zeros(B, dtype=np.int32), np.zeros((B, F, 3)),
                    np.zeros((B, F), dtype=np.int32))
        if name == "debug_tracks_read":
            return np.zeros(F, dtype=np.uint64), np.zeros((F, self.c_max, 4)), np.zeros((F, 3))
        if name == "nominal_get":
            return copy.deepcopy(self.tables)
        return None

    def __getattr__(self, name):
        def call(*args, **kw):
            self.log.append(name)
            if name.endswith("_prepare"):
                return lambda: self.log.append(name[:-len("_prepare")])
            return self.result(name)
        return call


B, FRAMES = 8, 4
STAGE = ["frame_stage_tracks_nominal_prepare", "frame_stage_tracks_nominal"]
USTAGE = ["update_stage_tracks_nominal_prepare", "update_stage_tracks_nominal"]
HOST = ["frame_stage_tracks_prepare", "frame_stage_tracks", "frame_run", "frame_fetch"]


@pytest.fixture(scope="module")
def cases():
    return cu.make_update_loop(B, FRAMES)


def run(cases, pipelined, **kw):
    r = Recorder(cases)
    cu.device_loop_update(r, cases, [0, 1, 2], pipelined, **kw)
    return r.log


def test_serial_two_update_loop(cases):
    assert run(cases, False) == 3 * (STAGE + ["frame_run", "frame_fetch"] + USTAGE + ["frame_run", "frame_fetch", "frame_fetch_tri"])
    assert run(cases, False, sync_every_call=True) == 3 * (STAGE + ["sync", "frame_run", "sync", "frame_fetch"]
                                                          + USTAGE + ["sync", "frame_run", "sync", "frame_fetch", "frame_fetch_tri"])


def test_pipelined_two_update_loop(cases):
    """run(i); ustage(i); fetch_begin(i); run_u(i); fetch_end(i); stage(i + 1); fetch_begin(u_i); run(i + 1); fetch_end(u_i); fetch_tri(u_i)"""
    step = ["frame_fetch_begin", "frame_run", "frame_fetch_end"]
    assert run(cases, True) == (STAGE + ["frame_run"] + USTAGE + step
                                + 2 * (STAGE + step + ["frame_fetch_tri"] + USTAGE + step)
                                + ["frame_fetch", "frame_fetch_tri"])


def test_entries_and_plain_forms_unchanged(cases):
    e = cu.two_update_entries([4, 5])
    assert [x if isinstance(x, int) else ("u", x.f, x.tri) for x in e] == [4, ("u", 4, True), 5, ("u", 5, True)]
    # a loop without update-only entries calls what it called before
    r = Recorder(cases)
    cl.DeviceLoop(r, cases, [0, 1], None, True).run()
    assert r.log == STAGE + ["frame_run"] + STAGE + ["frame_fetch_begin", "frame_run", "frame_fetch_end", "frame_fetch"]


def test_round_trip_form(cases):
    """as tools/closed_loop_bench.py --two-updates drives it: the plain loop, every stage prepared, the second update through the host"""
    r = Recorder(cases)
    loop = cl.DeviceLoop(r, cases, [0, 0, 0], cu.UpdateRoundTrip(cases, [0], 12), True, collect=False).prepare()
    r.log.clear()
    loop.run()
    S, RT = STAGE[1:], ["nominal_get", "msckf_update_tri", "marginalize", "nominal_set"]
    assert r.log == S + ["frame_run"] + 2 * (["frame_fetch_begin"] + RT + S + ["frame_run", "frame_fetch_end"]) + ["frame_fetch_begin"] + RT + ["frame_fetch_end"]


def test_host_reference_step(cases):
    r = Recorder(cases)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    cu.host_step_update(r, cases, tabs, 0, [dict() for _ in cases])
    assert r.log == HOST + B * ["debug_tracks_read"] + ["msckf_update_tri"] + B * ["marginalize"]


def test_scenario_shape(cases):
    """what the GPU comparison relies on: the first update marginalises nothing, the second lists a count that is no multiple of four
    over three or four selected slots that hold observations, its anchor among them, and no point of its tracks is handed over"""
    for c in cases:
        W = len(c["table"].clones) + 1
        for f, fr in enumerate(c["frames"]):
            u, d = fr["upd"], fr["delta"]
            assert fr["marg"] == -1 and fr["marg_upd"] >= 0
            assert not set(d.get("pf_track", [])) & set(range(cu.N_LOST, 24))
            nobs = min(f + 1, W - 1)
            if nobs < 3:
                assert not u["feat_track"] and not d["feat_track"]
                continue
            assert len(u["feat_track"]) % 4 and len(u["feat_track"]) == 24 - cu.N_LOST
            sel = [s for s in range(64) if (int(u["feat_sel"][0]) >> s) & 1]
            assert 3 <= len(sel) <= 4 and min(sel) >= W - nobs and max(sel) == W - 1 == u["feat_anchor"][0]
