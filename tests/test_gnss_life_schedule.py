"""The call order of the device loop in which the GNSS scalars enter, are estimated and leave (ingvio_amd/closed_loop_gnss_life.py, DESIGN
4.11), pinned without a GPU with the recording stand-in of tests/test_update_form_schedule.py: ingvio_nominal_add_gnss in front of the
loop, the acquisition and the drop as late calls behind their frame's epoch - in front of the next frame's stage, serial and pipelined -
the epoch behind the frame or staged with it, and its results fetched before the next frame runs."""
import numpy as np
import pytest

from conftest import load_golden
from ingvio_amd import closed_loop_gnss_life as gl
from ingvio_amd.closed_loop_gnss_init import fresh
from test_update_form_schedule import Recorder

F = 24
STAGE = ["frame_stage_tracks_nominal_prepare", "frame_stage_tracks_nominal"]
BEHIND = ["gnss_front_stage_nominal_prepare", "gnss_front_stage_nominal", "gnss_run", "gnss_fetch"]
INFRAME = ["gnss_frame_stage_nominal_prepare", "gnss_frame_stage_nominal"]
OURS = ("nominal_add_gnss", "nominal_marg_gnss", "gnss_init_nominal")


class LifeRecorder(Recorder):
    def __init__(self, cases, F=24):
        super().__init__(cases, F)
        self.n0 = [c["P"].shape[0] for c in cases]

    def result(self, name):
        B = self.batch
        if name == "nominal_add_gnss":
            return np.full(B, 40, dtype=np.int32), np.array(self.n0, dtype=np.int32)
        if name == "gnss_init_nominal":                                  # nothing accepted: the books stay
            return dict(added=np.zeros((B, 5), dtype=np.int32), new_idx=np.full((B, 5), -1, dtype=np.int32), slot=np.full((B, 5), -1, dtype=np.int32),
                        chi2=np.zeros((B, 5)), noise=np.zeros((B, 5)), dx=None, status=np.zeros(B, dtype=np.int32))
        if name == "gnss_fetch":
            return np.zeros((B, self.ldp)), np.zeros(B, dtype=np.int32), np.zeros((B, 64), dtype=np.int32), np.zeros((B, 64)), np.zeros(B, dtype=np.int32)
        if name == "debug_gnss_fused_last":
            return 1
        return super().result(name)


@pytest.fixture(scope="module")
def cases():
    return gl.make_life_loop(load_golden("gnss_front"), 4, 4)


def run(cases, pipelined, script=gl.SCRIPT, frames=(0, 1, 2, 3)):
    cs = fresh(cases)
    r = LifeRecorder(cs, F)
    out, form = gl.device_life(r, cs, list(frames), None, pipelined, script)
    return [n for n in r.log if n != "sync"], out, form, cs


def test_serial_order(cases):
    """frame 0: no epoch, the acquisition behind it; frame 1: the epoch behind the frame; frame 2: the epoch staged with the frame, then
    the drop; frame 3: the epoch behind the frame"""
    log, out, form, cs = run(cases, False)
    assert log == (["nominal_add_gnss"]
                   + STAGE + ["frame_run", "frame_fetch", "gnss_init_nominal"]
                   + STAGE + ["frame_run", "frame_fetch"] + BEHIND
                   + STAGE + INFRAME + ["frame_run", "frame_fetch", "gnss_fetch", "debug_gnss_fused_last", "nominal_marg_gnss"]
                   + STAGE + ["frame_run", "frame_fetch"] + BEHIND)
    assert len(out) == 4 and out[0][1] == () and all(len(o[1]) == 5 for o in out[1:])
    assert sorted(form.verdicts) == [0] and form.how == {2: 1}
    # YOF's slot and idx came from the call; the books counted it
    for c, c0 in zip(cs, cases):
        assert c["gnss_slots"][gl.YOF] == 40 and c["frames"][0]["new_idx"] == c0["P"].shape[0] + 1


def test_pipelined_order(cases):
    """late: fetch_begin(i); the epoch, the acquisition or the drop of frame i; stage(i + 1) (+ its in-frame epoch); run(i + 1); fetch_end(i)"""
    log, out, form, cs = run(cases, True)
    assert log == (["nominal_add_gnss"] + STAGE + ["frame_run"]
                   + ["frame_fetch_begin", "gnss_init_nominal"] + STAGE + ["frame_run", "frame_fetch_end"]
                   + ["frame_fetch_begin"] + BEHIND + STAGE + INFRAME + ["frame_run", "frame_fetch_end"]
                   + ["frame_fetch_begin", "gnss_fetch", "debug_gnss_fused_last", "nominal_marg_gnss"] + STAGE + ["frame_run", "frame_fetch_end"]
                   + ["frame_fetch_begin"] + BEHIND + ["frame_fetch_end"])
    assert len(out) == 4


@pytest.mark.parametrize("pipelined", [False, True])
def test_without_the_script_the_loop_is_the_late_plain_loop(cases, pipelined):
    """what the life cycle adds are its own calls and the epochs: with an empty script only ingvio_nominal_add_gnss is left of them"""
    log, _, _, _ = run(cases, pipelined, script={})
    assert log[0] == "nominal_add_gnss" and not set(log[1:]) & (set(OURS) | set(BEHIND) | set(INFRAME))
    full, _, _, _ = run(cases, pipelined)
    assert [n for n in full if n not in OURS and n not in BEHIND and n not in INFRAME and n != "debug_gnss_fused_last"] == log[1:]
