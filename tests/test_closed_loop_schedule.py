"""The order in which the closed-loop harness calls the context (ingvio_amd/closed_loop*.py), pinned without a GPU: a
stand-in for capi.Context records the method names while closed_loop.DeviceLoop drives every form of the loop over three frames, and
the host reference steps run one frame.  The nominal stages refuse when issued out of turn, so the order is part of the interface.
The lists were recorded from the loops as they were written out before DeviceLoop replaced them, one loop per form and mode."""
import copy

import numpy as np
import pytest

from conftest import load_golden
from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_gnss as cg
from ingvio_amd import closed_loop_lm as clm


class Recorder:
    """stands in for capi.Context: logs the name of every method called on it; a *_prepare method hands back a callable that logs the
    name of the stage it issues; fetches return zeros of the right shapes, nominal_get the cases' start tables"""

    def __init__(self, cases, F=24):
        self.log = []
        self.batch, self.f_max = len(cases), F
        self.ldp = max(c["P"].shape[0] for c in cases) + 16
        self.tables = [c["table"].as_dict() for c in cases]

    def result(self, name):
        B, n = self.batch, self.ldp
        if name in ("frame_fetch", "frame_fetch_end"):
            return np.zeros((B, n)), np.zeros((B, self.f_max), dtype=np.int32), np.zeros(B, dtype=np.int32)
        if name in ("gnss_fetch", "landmark_fetch"):
            return np.zeros((B, n)), np.zeros(B, dtype=np.int32), np.zeros((B, 64), dtype=np.int32), np.zeros((B, 64)), np.zeros(B, dtype=np.int32)
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


B, FRAMES = 24, 13
STAGE = ["frame_stage_tracks_nominal_prepare", "frame_stage_tracks_nominal"]
GNSS = ["gnss_front_stage_nominal_prepare", "gnss_front_stage_nominal"]
LMS = ["landmark_stage_nominal_prepare", "landmark_stage_nominal"]
GNSS_RT = ["nominal_get", "gnss_front_stage_prepare", "gnss_front_stage", "gnss_run", "gnss_fetch", "nominal_box_plus"]
LM_RT = ["nominal_get", "landmark_stage", "landmark_run", "landmark_fetch", "nominal_box_plus"]
HOST = ["frame_stage_tracks_prepare", "frame_stage_tracks", "frame_run", "frame_fetch"]


@pytest.fixture(scope="module")
def loops():
    from ingvio_amd import synth
    return dict(plain=cl.make_loop(B, FRAMES), gnss=cg.make_gnss_loop(load_golden("gnss_front"), B, FRAMES), lm=clm.make_lm_loop(B, FRAMES),
                chi2=synth.chi2_table(), opts=clm.lm_opts())


def run(cases, form, pipelined, prepare=False, **kw):
    r = Recorder(cases)
    loop = cl.DeviceLoop(r, cases, [0, 1, 2], form, pipelined, **kw)
    if prepare:
        loop.prepare()
        r.log.clear()
    loop.run()
    return r.log


def test_plain_loop(loops):
    assert run(loops["plain"], None, False) == 3 * (STAGE + ["frame_run", "frame_fetch"])
    assert run(loops["plain"], None, True) == (STAGE + ["frame_run"]
                                                + 2 * (STAGE + ["frame_fetch_begin", "frame_run", "frame_fetch_end"])
                                                + ["frame_fetch"])


def test_gnss_loop(loops):
    form = cg.GnssForm(loops["chi2"])
    assert run(loops["gnss"], form, False) == 3 * (STAGE + ["frame_run", "frame_fetch"] + GNSS + ["gnss_run", "gnss_fetch"])
    assert run(loops["gnss"], form, False, sync_every_call=True) == 3 * (
        STAGE + ["sync", "frame_run", "sync", "frame_fetch"] + GNSS + ["sync", "gnss_run", "sync", "gnss_fetch"])
    # the GNSS stage of frame i between fetch_begin(i) and the stage of frame i + 1
    assert run(loops["gnss"], form, True) == (STAGE + ["frame_run"]
                                               + 2 * (["frame_fetch_begin"] + GNSS + ["gnss_run"] + STAGE + ["frame_run", "frame_fetch_end", "gnss_fetch"])
                                               + ["frame_fetch_begin"] + GNSS + ["gnss_run", "frame_fetch_end", "gnss_fetch"])


def test_landmark_loop(loops):
    form = clm.LmForm(loops["opts"])
    assert run(loops["lm"], form, False) == 3 * (STAGE + LMS + ["frame_run", "frame_fetch", "landmark_fetch"])
    # the landmark stage of frame i + 1 right after its frame stage and before fetch_begin(i); landmark_fetch(i) before run(i + 1)
    assert run(loops["lm"], form, True) == (STAGE + LMS + ["frame_run"]
                                             + 2 * (STAGE + LMS + ["frame_fetch_begin", "landmark_fetch", "frame_run", "frame_fetch_end"])
                                             + ["frame_fetch", "landmark_fetch"])


def test_round_trip_forms(loops):
    """as the bench tool drives them: every frame stage prepared beforehand"""
    S = STAGE[1:]
    assert run(loops["gnss"], cg.GnssRoundTrip(loops["chi2"]), True, prepare=True) == (
        S + ["frame_run"] + 2 * (["frame_fetch_begin"] + GNSS_RT + S + ["frame_run", "frame_fetch_end"])
        + ["frame_fetch_begin"] + GNSS_RT + ["frame_fetch_end"])
    assert run(loops["lm"], clm.LmRoundTrip(loops["opts"]), True, prepare=True) == (
        S + ["frame_run"] + 2 * (["frame_fetch_begin"] + LM_RT + S + ["frame_run", "frame_fetch_end"])
        + ["frame_fetch_begin"] + LM_RT + ["frame_fetch_end"])


def test_bench_tool_forms(loops):
    """prepared beforehand, the forms' results not collected"""
    S, G, L = STAGE[1:], GNSS[1:], LMS[1:]
    assert run(loops["gnss"], cg.GnssForm(loops["chi2"]), True, prepare=True, collect=False) == (
        S + ["frame_run"] + 2 * (["frame_fetch_begin"] + G + ["gnss_run"] + S + ["frame_run", "frame_fetch_end"])
        + ["frame_fetch_begin"] + G + ["gnss_run", "frame_fetch_end"])
    assert run(loops["gnss"], cg.GnssForm(loops["chi2"], epochs=False), True, prepare=True, collect=False) == (
        S + ["frame_run"] + 2 * (["frame_fetch_begin"] + S + ["frame_run", "frame_fetch_end"]) + ["frame_fetch_begin", "frame_fetch_end"])
    assert run(loops["lm"], clm.LmForm(loops["opts"]), True, prepare=True, collect=False) == (
        S + L + ["frame_run"] + 2 * (S + L + ["frame_fetch_begin", "frame_run", "frame_fetch_end"]) + ["frame_fetch"])


def test_host_reference_steps(loops):
    def tabs(cases):
        return [copy.deepcopy(c["table"]) for c in cases]
    r = Recorder(loops["plain"])
    cl.host_step(r, loops["plain"], tabs(loops["plain"]), 0)
    assert r.log == HOST
    r = Recorder(loops["gnss"])
    cg.host_step_gnss(r, loops["gnss"], tabs(loops["gnss"]), 0, loops["chi2"])
    assert r.log == HOST + ["gnss_front_stage", "gnss_run", "gnss_fetch"]
    r = Recorder(loops["lm"])
    clm.host_step_lm(r, loops["lm"], tabs(loops["lm"]), 0, loops["opts"])
    assert r.log == HOST + ["landmark_stage", "landmark_run", "landmark_fetch"] + B * ["marginalize"]
    r = Recorder(loops["lm"])
    clm.host_step_lm_prestaged(r, loops["lm"], tabs(loops["lm"]), 0, loops["opts"])
    assert r.log == HOST[:2] + ["landmark_stage", "frame_run", "frame_fetch", "landmark_fetch"]
