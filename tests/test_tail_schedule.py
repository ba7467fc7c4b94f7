"""The call order of the closed loop with the landmark tail (ingvio_amd/closed_loop_tail.py), pinned without a GPU beside
tests/test_closed_loop_schedule.py with its recording stand-in for the context: ingvio_nominal_tail of frame i lies behind that frame's
run and fetch_begin and in front of the stage of frame i + 1 - the stage validates against the mirror the tail has just moved."""
import numpy as np
import pytest

from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_lm as clm
from ingvio_amd import closed_loop_tail as clt
from test_closed_loop_schedule import LMS, STAGE, Recorder


class TailRecorder(Recorder):
    def result(self, name):
        if name == "nominal_tail":
            return np.ones((self.batch, 64), dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
        return super().result(name)


@pytest.fixture(scope="module")
def cases():
    return clt.make_tail_loop(4, 3)


def run(cases, form, pipelined, **kw):
    r = TailRecorder(cases)
    cl.DeviceLoop(r, cases, [0, 1, 2], form, pipelined, **kw).run()
    return r.log


def test_tail_loop(cases):
    TAIL = ["landmark_fetch", "nominal_tail"]
    form = lambda **kw: clt.TailForm(clm.lm_opts(), cases, **kw)
    assert run(cases, form(), False) == 3 * (STAGE + LMS + ["frame_run", "frame_fetch"] + TAIL)
    assert run(cases, form(), True) == (STAGE + LMS + ["frame_run"]
                                        + 2 * (["frame_fetch_begin"] + TAIL + STAGE + LMS + ["frame_run", "frame_fetch_end"])
                                        + ["frame_fetch_begin"] + TAIL + ["frame_fetch_end"])
    # as the bench tool drives it: the landmark results stay on the device
    assert run(cases, form(fetch_lm=False), True, collect=False) == (
        STAGE + LMS + ["frame_run"] + 2 * (["frame_fetch_begin", "nominal_tail"] + STAGE + LMS + ["frame_run", "frame_fetch_end"])
        + ["frame_fetch_begin", "nominal_tail", "frame_fetch_end"])


def test_frames_are_staged_without_a_marginalisation(cases):
    """the tail drops the clone, not the frame; the plan follows the table's integers and the verdicts"""
    assert all(fr["marg"] == -1 and fr["marg_pos"] == [0] for c in cases for fr in c["frames"])
    c = cases[0]
    t = c["table"].as_dict()
    plan = clt.frame_plan(c, c["frames"][0], dict(t, clone_var=list(t["clone_var"]) + [len(t["kind"])]), list(range(6)))
    assert plan["marg_slot"] == [t["clone_var"][0]] and plan["new_anchor"] == len(t["kind"]) and plan["lm_slot"] == c["lm_slots"]
    assert clt.plan_survivors(c, plan, [1, 1, 0, 1, 1, 0], list(range(6))) == [0, 1, 3, 4]
