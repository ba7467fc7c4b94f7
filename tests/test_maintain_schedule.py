"""The call order of the two-update closed loop with the MSCKF anchor change / invalid-feature erase (ingvio_amd/closed_loop_maintain.py,
DESIGN 4.11), pinned without a GPU with the recording stand-in of tests/test_update_form_schedule.py: the synchronous call as a late
form, the free-running form (_begin right behind the run of a camera frame's second update, _end right behind the run of the next
camera frame's first update, whose stage was built without the verdicts), the key-frame cadence with its ingvio_nominal_tail in front
of the call - and the loops without the form calling exactly what they called before."""
import numpy as np
import pytest

from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_maintain as cm
from ingvio_amd import closed_loop_update as cu
from test_update_form_schedule import Recorder

F = 24
STAGE = ["frame_stage_tracks_nominal_tri_prepare", "frame_stage_tracks_nominal_tri"]
USTAGE = ["update_stage_tracks_nominal_prepare", "update_stage_tracks_nominal"]
OURS = ("tracks_maintain", "tracks_maintain_begin", "tracks_maintain_end", "nominal_tail")


class MaintainRecorder(Recorder):
    def result(self, name):
        if name in ("tracks_maintain", "tracks_maintain_end"):
            return [dict(verdict=np.zeros(cm.DECOYS + 1, dtype=np.uint8), depth=np.zeros(cm.DECOYS + 1), lm_verdict=np.zeros(0, dtype=np.uint8)) for _ in range(self.batch)]
        if name == "nominal_tail":
            return np.ones((self.batch, 64), dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
        return super().result(name)


@pytest.fixture(scope="module")
def loops():
    return dict(sw=cm.add_decoys(cu.make_update_loop(4, 4, F, first_tri=True), F, "sw"),
                kf=cm.add_decoys(cu.make_keyframe_loop(4, 4, F, first_tri=True), F, "kf"))


def run(cases, free_running, pipelined, form=True):
    r = MaintainRecorder(cases, F + cm.DECOYS)
    out = {}
    f = cm.decoy_form(cases, [cm.Book(c) for c in cases], out, free_running) if form else None
    cl.DeviceLoop(r, cases, cu.two_update_entries([0, 1]), f, pipelined, update_stage=cu.update_stage).run()
    return r.log, out


@pytest.mark.parametrize("mode", ["sw", "kf"])
def test_synchronous_form(loops, mode):
    tail = ["nominal_tail"] if mode == "kf" else []                      # (the key-frame cadence drops two clones behind camera frame 1)
    first = STAGE + ["frame_run", "frame_fetch", "frame_fetch_tri"]
    log, out = run(loops[mode], False, False)
    assert log == (first + USTAGE + ["frame_run", "frame_fetch", "tracks_maintain", "frame_fetch_tri"]
                   + first + USTAGE + ["frame_run", "frame_fetch"] + tail + ["tracks_maintain", "frame_fetch_tri"])
    assert sorted(out) == [0, 1] and all(tr == [cm.REAL, F, F + 1, F + 2] for per in out.values() for tr, _, _ in per)
    # pipelined, a late form: fetch_begin(i); maintain(i); stage(i + 1); run(i + 1); fetch_end(i)
    step = ["frame_run", "frame_fetch_end", "frame_fetch_tri"]
    log, _ = run(loops[mode], False, True)
    assert log == (STAGE + ["frame_run", "frame_fetch_begin"] + USTAGE + step + ["frame_fetch_begin", "tracks_maintain"]
                   + STAGE + step + ["frame_fetch_begin"] + USTAGE + step + ["frame_fetch_begin"] + tail + ["tracks_maintain", "frame_fetch_end", "frame_fetch_tri"])


@pytest.mark.parametrize("mode", ["sw", "kf"])
def test_free_running_form(loops, mode):
    """run(u_i); maintain_begin(i); fetch_end; stage(i + 1); fetch_begin; run(i + 1); maintain_end(i); ...; the last one is ended at once"""
    tail = ["nominal_tail"] if mode == "kf" else []
    step = ["frame_fetch_begin", "frame_run"]
    log, out = run(loops[mode], True, True)
    assert log == (STAGE + ["frame_run"] + USTAGE + step + ["tracks_maintain_begin", "frame_fetch_end", "frame_fetch_tri"]
                   + STAGE + step + ["tracks_maintain_end", "frame_fetch_end", "frame_fetch_tri"]
                   + USTAGE + step + tail + ["tracks_maintain_begin", "tracks_maintain_end", "frame_fetch_end", "frame_fetch_tri"]
                   + ["frame_fetch", "frame_fetch_tri"])
    assert sorted(out) == [0, 1]


@pytest.mark.parametrize("mode", ["sw", "kf"])
@pytest.mark.parametrize("pipelined", [False, True])
def test_the_loop_without_the_form_is_unchanged(loops, mode, pipelined):
    """what the form adds are its own calls: taken out of the serial and of the free-running sequence, the plain loop's is left"""
    plain, _ = run(loops[mode], False, pipelined, form=False)
    with_form, _ = run(loops[mode], pipelined, pipelined)
    assert [n for n in with_form if n not in OURS] == plain and not set(plain) & set(OURS)


def test_bookkeeping_of_lagged_verdicts(loops):
    """verdicts that arrive behind the next stage leave the bookkeeping the synchronous form has: an erased track observed since is a
    restarted one, the mover hangs on the window's second clone again"""
    c = loops["sw"][0]
    a, b = cm.Book(c), cm.Book(c)
    for bk in (a, b):
        bk.staged()
        gone = bk.leave(c["frames"][0])
    tracks, _ = a.words(gone)
    verdicts = [cm.ERASED_INVALID, cm.KEEP, cm.ERASED_MOVE, cm.ERASED_INVALID]
    new, then = a.ints.clones[-1], a.stages
    a.done(tracks, verdicts, new, then); a.staged()                      # synchronous: verdicts, then the stage
    b.staged(); b.done(tracks, verdicts, new, then)                      # free-running: the stage, then the verdicts
    assert a.an.slot == b.an.slot and sorted(a.an.slot) == tracks and a.ints.clones == b.ints.clones
    # mask = the observations since, anchor = the first of them: the erased tracks hold the one observation of the later stage
    assert a.obs == b.obs and [a.mask(t) for t in tracks] == [b.mask(t) for t in tracks]
    new = a.ints.clones[-1]
    assert a.obs[cm.REAL] == [new] and a.an.slot[cm.REAL] == new and a.obs[F + cm.INVALID] == [new] and len(a.obs[F + cm.KEEPER]) == 2
