"""The call order of the closed loop whose first updates triangulate on the device (ingvio_frame_stage_tracks_nominal_tri; ingvio_amd/
closed_loop*.py), pinned without a GPU with the recording stand-in of tests/test_closed_loop_schedule.py (in the form
tests/test_update_form_schedule.py gives it: it also answers the triangulating fetches): the positions of stage, run and
fetch_begin / fetch_tri / fetch_end, serial and pipelined, and the host reference step of one camera frame."""
import copy

import numpy as np
import pytest

from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_update as cu
from test_update_form_schedule import Recorder as UpdateRecorder


class Recorder(UpdateRecorder):
    def result(self, name):
        if name == "triangulate":
            return np.zeros((self.batch, self.f_max, 3)), np.zeros((self.batch, self.f_max), dtype=np.int32)
        return super().result(name)


B, FRAMES = 6, 4
TSTAGE = ["frame_stage_tracks_nominal_tri_prepare", "frame_stage_tracks_nominal_tri"]
USTAGE = ["update_stage_tracks_nominal_prepare", "update_stage_tracks_nominal"]
HOST = ["frame_stage_tracks_prepare", "frame_stage_tracks", "frame_run", "frame_fetch"]


@pytest.fixture(scope="module")
def cases():
    return cu.make_update_loop(B, FRAMES, first_tri=True)


def run(cases, pipelined, **kw):
    r = Recorder(cases)
    out = cu.device_loop_update(r, cases, [0, 1, 2], pipelined, **kw)
    assert all(len(first) == 5 and len(second) == 5 for first, second in out)      # (dx, accept, rows, pf, tri_ok) of both kinds of entry
    return r.log


def test_serial_loop(cases):
    assert run(cases, False) == 3 * (TSTAGE + ["frame_run", "frame_fetch", "frame_fetch_tri"] + USTAGE + ["frame_run", "frame_fetch", "frame_fetch_tri"])
    assert run(cases, False, sync_every_call=True) == 3 * (TSTAGE + ["sync", "frame_run", "sync", "frame_fetch", "frame_fetch_tri"]
                                                          + USTAGE + ["sync", "frame_run", "sync", "frame_fetch", "frame_fetch_tri"])


def test_pipelined_loop(cases):
    """fetch_tri of either kind of entry follows the fetch_end of that entry, which follows the run of the next one"""
    step = ["frame_fetch_begin", "frame_run", "frame_fetch_end", "frame_fetch_tri"]
    assert run(cases, True) == (TSTAGE + ["frame_run"] + USTAGE + step
                                + 2 * (TSTAGE + step + USTAGE + step)
                                + ["frame_fetch", "frame_fetch_tri"])


def test_loops_without_first_tri_call_what_they_called(cases):
    plain = cu.make_update_loop(B, FRAMES)
    r = Recorder(plain)
    cl.DeviceLoop(r, plain, [0, 1], None, True).run()
    S = ["frame_stage_tracks_nominal_prepare", "frame_stage_tracks_nominal"]
    assert r.log == S + ["frame_run"] + S + ["frame_fetch_begin", "frame_run", "frame_fetch_end", "frame_fetch"]


def test_host_reference_step(cases):
    """frames 0 and 1 list nothing (nothing to triangulate), frame 2 does: the host-fed triangulation comes in front of the stage"""
    r = Recorder(cases)
    tabs = [copy.deepcopy(c["table"]) for c in cases]
    stores = [cu.HostStore(24, 12) for _ in cases]
    points = [dict() for _ in cases]
    tail = B * ["debug_tracks_read"] + ["msckf_update_tri"] + B * ["marginalize"]
    for f in range(3):
        r.log.clear()
        first, second = cu.host_step_update(r, cases, tabs, f, points, stores=stores)
        assert len(first) == 5
        assert r.log == (["triangulate"] if f == 2 else []) + HOST + tail, f


def test_scenario_shape(cases):
    """no point is handed over; from the third frame on the first update lists the lost tracks, the far track and, where it holds one
    or two observations, the restarted one"""
    for c in cases:
        assert c["first_tri"]
        for f, fr in enumerate(c["frames"]):
            d = fr["delta"]
            assert "pf_track" not in d and "pf" not in d
            if f < 2:
                assert not d["feat_track"]
                continue
            want = list(range(cu.N_LOST)) + ([cu.N_LOST] if f >= 3 else []) + ([23] if f % 3 != 1 else []) + [cu.far_track(24)]
            assert list(d["feat_track"]) == want and len(d["feat_anchor"]) == len(want) == len(d["feat_dof"])
