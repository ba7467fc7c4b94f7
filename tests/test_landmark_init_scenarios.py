"""The scenarios tests/test_gpu_landmark_init.py runs (landmark_init_helpers.py), checked on the CPU: the numpy restatement of
calcResJacobianSingleFeatAll{Mono,Stereo}Obs against oracle/stream_filter.py, and - through oracle.Cov.add_variable_delayed alone,
candidate by candidate with boxPlus in between - the conditions the GPU tests rely on.  A seed that does not meet them is changed here."""
import os
import re
import types

import numpy as np
import pytest

import landmark_init_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_exports():
    text = open(os.path.join(ROOT, "include", "ingvio_hip.h")).read()
    for name in ("ingvio_landmark_init_nominal", "ingvio_debug_landmark_init_rows"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    for name in ("ingvio_lm_init_cand", "ingvio_lm_init_block"):
        assert re.search(r"}\s*%s\s*;" % name, text), name
    from ingvio_amd import capi
    assert "ingvio_landmark_init_nominal" in capi.EXPORTS and "ingvio_debug_landmark_init_rows" in capi.EXPORTS
    assert hasattr(capi.Context, "landmark_init_nominal")


@pytest.mark.parametrize("stereo", [True, False])
def test_numpy_rows_against_the_stream_oracle(stereo):
    from oracle import stream_filter as sf
    from ingvio_amd import synth
    f = H.make_scenario((6,), seed=3, stereo=stereo)[0]
    cR, cp, _ = H.window_of(f["table"])
    Rlr, tlr = synth.t_cl2cr()
    sw = {}
    for q in range(f["Cw"]):
        v = sf.Var("se3", 6); v.R, v.p = cR[q], cp[q]
        sw[float(q)] = v
    flt = types.SimpleNamespace(sw=sw, stereo=stereo, R_cl2cr=Rlr, t_cl2cr=tlr, sw_sorted=lambda: sorted(sw.items()))
    for tr in (H.T_GOOD, H.T_GAP):
        fi = sf.Feature()
        fi.pf, fi.anchor = f["pf"][tr], sw[float(f["anchor"][tr])]
        fi.obs = {float(q): tuple(uv) for q, uv in H.obs_of(f, tr)}
        fi.obs[99.0] = (0.0, 0.0, 0.0, 0.0)                                           # a stamp outside the window: skipped
        res, Hx, Hf = sf.Filter.feat_all_obs_rows(flt, fi)
        H_old, H_new, r = H.rows_at(f, f["table"], tr)
        assert H_old.shape == Hx.shape and H_old.shape[0] == (4 if stereo else 2) * len(H.obs_of(f, tr))
        s = np.abs(Hx).max()
        assert np.abs(H_old - Hx).max() <= 1e-13 * s and np.abs(H_new - Hf).max() <= 1e-13 * s and np.abs(r - res).max() <= 1e-13


def far_from_gate(r):
    for g, thr, m in zip(r["chi2"], r["thr"], r["m"]):
        if m > 3:
            assert abs(g - thr) > 0.02 * thr, (g, thr)


@pytest.mark.parametrize("stereo", [True, False])
def test_one_candidate_scenarios(stereo):
    scn = H.make_scenario(H.MIXED_WINDOWS, seed=11, stereo=stereo)
    for f in scn:
        a = H.oracle_sequence(f, [H.T_GOOD]); g = H.oracle_sequence(f, [H.T_GROSS])
        assert a["added"] == [True] and g["added"] == [False] and a["m"][0] > 3 and g["m"][0] > 3
        far_from_gate(a); far_from_gate(g)
        assert np.array_equal(g["P"], f["P"])


def test_row_scenarios():
    for stereo in (True, False):
        scn = H.make_scenario(H.ROW_WINDOWS, seed=7, drops=H.ROW_DROPS, stereo=stereo)
        for f in scn:
            per = 4 if stereo else 2
            for tr in (H.T_GOOD, H.T_GAP, H.T_PAIR, H.T_SINGLE):
                m = H.rows_at(f, f["table"], tr)[0].shape[0]
                assert m == per * bin(f["wmask"][tr]).count("1")
            assert all(q != f["anchor"][H.T_GAP] for q, _ in H.obs_of(f, H.T_GAP))          # the anchor clone does not observe it
            assert any(q == f["anchor"][H.T_PAIR] for q, _ in H.obs_of(f, H.T_PAIR))        # observer == anchor
            assert len(H.obs_of(f, H.T_SINGLE)) == 1


def test_sequence_scenario():
    scn = H.make_scenario(H.SEQ_WINDOWS, seed=21)
    for f in scn:
        r = H.oracle_sequence(f, H.SEQ_TRACKS)
        assert r["added"] == [True, False, True] and min(r["m"]) > 3
        far_from_gate(r)
        n0 = f["P"].shape[0]
        free = H.free_slots(f["table"])
        assert r["new_idx"] == [n0, -1, n0 + 3] and r["slot"] == [free[0], -1, free[2]]
        # the third candidate's rows at the updated poses against its rows at the initial poses: the order test can fail
        Hn, _, rn = H.rows_at(f, r["table"], H.T_GOOD2)
        H0, _, r0 = H.rows_at(f, f["table"], H.T_GOOD2)
        assert np.abs(Hn - H0).max() > 1e-6 * np.abs(H0).max()
        up = H.oracle_sequence(f, H.SEQ_TRACKS, reform=False)
        assert up["added"] == r["added"]
        gap = abs(up["chi2"][2] - r["chi2"][2]) / max(1.0, r["chi2"][2])
        dgap = np.linalg.norm(up["dx"][2] - r["dx"][2]) / np.linalg.norm(r["dx"][2])
        assert gap > 1e-6 and dgap > 1e-6, (gap, dgap)
