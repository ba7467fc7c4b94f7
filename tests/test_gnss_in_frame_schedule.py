"""The call order of the closed loop with the GNSS epoch staged WITH its frame (closed_loop_gnss.GnssInFrameForm,
ingvio_gnss_frame_stage_nominal), pinned without a GPU with the recording stand-in of tests/test_closed_loop_schedule.py:
the epoch's stage lies right behind the frame stage it belongs to, no gnss_run is issued (the frame's run applies the epoch), and the
GNSS results of frame i are fetched between fetch_begin(i) and run(i + 1) - the form is not late, frame i + 1 is staged while frame
i runs."""
import pytest

from conftest import load_golden
from ingvio_amd import closed_loop_gnss as cg
from test_closed_loop_schedule import STAGE, run

GIF = ["gnss_frame_stage_nominal_prepare", "gnss_frame_stage_nominal"]


@pytest.fixture(scope="module")
def loop():
    from ingvio_amd import synth
    return cg.make_gnss_loop(load_golden("gnss_front"), 4, 3, scalars_in_front=True, n_sat=8), synth.chi2_table()


def test_in_frame_gnss_loop(loop):
    cases, chi2 = loop
    form = cg.GnssInFrameForm(chi2)
    assert not form.late
    assert run(cases, form, False) == 3 * (STAGE + GIF + ["frame_run", "frame_fetch", "gnss_fetch"])
    assert run(cases, form, False, sync_every_call=True) == 3 * (STAGE + ["sync"] + GIF + ["sync", "frame_run", "sync", "frame_fetch", "gnss_fetch"])
    # run(i); stage(i + 1); gnss_frame_stage(i + 1); fetch_begin(i); gnss_fetch(i); run(i + 1); fetch_end(i)
    assert run(cases, form, True) == (STAGE + GIF + ["frame_run"]
                                      + 2 * (STAGE + GIF + ["frame_fetch_begin", "gnss_fetch", "frame_run", "frame_fetch_end"])
                                      + ["frame_fetch", "gnss_fetch"])
    assert "gnss_run" not in run(cases, form, True) + run(cases, form, False)


def test_in_frame_gnss_loop_as_the_bench_tool_drives_it(loop):
    """every stage prepared beforehand, the GNSS results not collected"""
    cases, chi2 = loop
    S, G = STAGE[1:], GIF[1:]
    assert run(cases, cg.GnssInFrameForm(chi2), True, prepare=True, collect=False) == (
        S + G + ["frame_run"] + 2 * (S + G + ["frame_fetch_begin", "frame_run", "frame_fetch_end"]) + ["frame_fetch"])


def test_loop_keywords(loop):
    """scalars_in_front leaves the GNSS scalars below every clone (no marginalisation moves them); n_sat truncates every epoch; the
    defaults are the loop as it was"""
    cases, _ = loop
    z = load_golden("gnss_front")
    for c in cases:
        lo = min(c["table"].slots[v]["idx"] for v in c["table"].clones)
        assert all(c["table"].slots[s]["idx"] < lo for s in c["gnss_slots"] if s >= 0)
        assert all(fr["gnss_idx"] == c["frames"][0]["gnss_idx"] for fr in c["frames"])
        assert all(e is None or (e["eph"].shape == (8, 25) and e["obs"].shape == (8, 6)) for e in c["epochs"])
    assert sorted(int(s) for s in z["eph"][:8, 0]) == [0, 0, 0, 0, 2, 2, 3, 3]      # four GPS, two Galileo, two BDS
    default = cg.make_gnss_loop(z, 2, 2)
    for c in default:
        lo = min(c["table"].slots[v]["idx"] for v in c["table"].clones)
        assert all(c["table"].slots[s]["idx"] > lo for s in c["gnss_slots"] if s >= 0)
        assert all(e is None or e["eph"].shape[0] == z["eph"].shape[0] for e in c["epochs"])
