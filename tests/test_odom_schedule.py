"""Where OdomForm (ingvio_amd/closed_loop_odom.py) puts ingvio_odom_begin / _end in the call sequences of
closed_loop.DeviceLoop, pinned without a GPU with the recording stand-in of tests/test_closed_loop_schedule.py: behind run(i) and in
front of stage(i + 1) for the plain and in-frame forms, behind the inner form's own run for the late ones, and never two begins
without an end between them (one slot is pending at a time)."""
import pytest

from conftest import load_golden
from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_gnss as cg
from ingvio_amd import closed_loop_lm as clm
from ingvio_amd.closed_loop_odom import OdomForm
from test_closed_loop_schedule import GNSS, LMS, STAGE, Recorder, run

B, FRAMES = 4, 4


@pytest.fixture(scope="module")
def loops():
    from ingvio_amd import synth
    return dict(plain=cl.make_loop(B, FRAMES), gnss=cg.make_gnss_loop(load_golden("gnss_front"), B, FRAMES), lm=clm.make_lm_loop(B, FRAMES),
                chi2=synth.chi2_table(), opts=clm.lm_opts())


def one_slot(log):
    calls = [c for c in log if c in ("odom_begin", "odom_end")]
    return calls == ["odom_begin", "odom_end"] * (len(calls) // 2)


def test_base_form_has_the_hook():
    assert cl.Form().ran(None, 0) is None


def test_serial(loops):
    log = run(loops["plain"], OdomForm(), False)
    assert log == 3 * (STAGE + ["frame_run", "odom_begin", "frame_fetch", "odom_end"])
    log = run(loops["gnss"], OdomForm(cg.GnssForm(loops["chi2"])), False)
    assert log == 3 * (STAGE + ["frame_run", "frame_fetch"] + GNSS + ["gnss_run", "odom_begin", "gnss_fetch", "odom_end"])


def test_pipelined(loops):
    # odom_begin(i) behind run(i) and in front of stage(i + 1); collected before run(i + 1), whose own record follows it
    log = run(loops["plain"], OdomForm(), True)
    assert log == (STAGE + ["frame_run", "odom_begin"]
                   + 2 * (STAGE + ["frame_fetch_begin", "odom_end", "frame_run", "odom_begin", "frame_fetch_end"])
                   + ["frame_fetch", "odom_end"])
    assert one_slot(log)
    # the in-frame landmark form: its stage of frame i + 1 follows the frame stage, the record of frame i is taken in front of both
    log = run(loops["lm"], OdomForm(clm.LmForm(loops["opts"])), True)
    assert log == (STAGE + LMS + ["frame_run", "odom_begin"]
                   + 2 * (STAGE + LMS + ["frame_fetch_begin", "landmark_fetch", "odom_end", "frame_run", "odom_begin", "frame_fetch_end"])
                   + ["frame_fetch", "landmark_fetch", "odom_end"])


def test_pipelined_not_collected(loops):
    """as the bench tool drives it: record i is ended behind run(i + 1), right in front of odom_begin(i + 1)"""
    S = STAGE[1:]
    form = OdomForm()
    log = run(loops["plain"], form, True, prepare=True, collect=False)
    assert log == (S + ["frame_run", "odom_begin"]
                   + 2 * (S + ["frame_fetch_begin", "frame_run", "odom_end", "odom_begin", "frame_fetch_end"])
                   + ["frame_fetch"])
    r = Recorder(loops["plain"])
    form.finish(r)
    assert r.log == ["odom_end"] and not form.pending


def test_pipelined_late(loops):
    # behind the GNSS run of frame i, in front of stage(i + 1); odom_end(i) behind fetch_end(i), after run(i + 1)
    log = run(loops["gnss"], OdomForm(cg.GnssForm(loops["chi2"])), True)
    assert log == (STAGE + ["frame_run"]
                   + 2 * (["frame_fetch_begin"] + GNSS + ["gnss_run", "odom_begin"] + STAGE + ["frame_run", "frame_fetch_end", "gnss_fetch", "odom_end"])
                   + ["frame_fetch_begin"] + GNSS + ["gnss_run", "odom_begin", "frame_fetch_end", "gnss_fetch", "odom_end"])
    assert one_slot(log)
