"""The conditions the GPU comparisons of tests/test_gpu_delayed_large.py rest on, asserted on the oracle alone (no GPU): every scenario
has accepted and refused candidates, no chi2 lies within 1e-6 (relative) of its threshold, no formed row has a camera-frame depth within
1e-6 (relative) of zero, and the trailing update's S is positive definite in every accepted case.

Nearest distances found (relative): chi2 from its threshold 0.959 (host-fed scenarios; `small`) and 0.943 (rows formed from the table,
27 clones stereo).  Each test prints its own figures."""
import numpy as np
import pytest

import delayed_large_helpers as L
import landmark_init_helpers as H


@pytest.mark.parametrize("name", sorted(L.SCENARIOS))
def test_host_fed_scenarios(name):
    priors, blocks, refs = L.reference(name)
    tried = [a for r, cs in zip(refs, blocks) for a, cand in zip(r[0][1], cs) if cand[3].shape[0] > cand[3].shape[1]]      # not skipped for m <= s
    assert any(tried) and not all(tried), (name, tried)
    gaps = [g for r in refs for g in r[1]]
    eigs = [e for r in refs for e in r[2]]
    print("%s: nearest chi2 to its threshold %.3g (relative), smallest eigenvalue of an accepted S %.3g" % (name, min(gaps), min(eigs)))
    assert min(gaps) > 1e-6 and min(eigs) > 0.0


@pytest.mark.parametrize("stereo", [True, False])
def test_rows_from_the_table(stereo):
    from ingvio_amd import synth
    tab = synth.chi2_table()
    per = 4 if stereo else 2
    for f in L.lm_scenario(stereo):
        assert per * f["Cw"] < len(tab)
        for tr in (H.T_GOOD, H.T_GROSS, H.T_GOOD2, H.T_GAP):
            Hx, Hf, res, depth = L.reference_rows(f, f["table"], tr)
            H_old, H_new, r = H.rows_at(f, f["table"], tr)
            s = np.abs(Hx).max()
            assert np.abs(H_old - Hx).max() <= 1e-13 * s and np.abs(H_new - Hf).max() <= 1e-13 * s and np.abs(r - res).max() <= 1e-13
            assert depth > 1e-6, (f["Cw"], tr, depth)
        assert f["anchor"][H.T_GAP] == 0 and not (f["wmask"][H.T_GAP] & 1)                       # the anchor does not observe
        ref = H.oracle_sequence(f, L.LM_TRACKS)
        assert ref["added"] == [True, False, True]
        gaps = [abs(g - t) / t for g, t in zip(ref["chi2"], ref["thr"])]
        up = H.oracle_sequence(f, L.LM_TRACKS, reform=False)
        moved = abs(up["chi2"][2] - ref["chi2"][2]) / max(1.0, ref["chi2"][2])
        print("stereo=%d window=%d: nearest chi2 to its threshold %.3g, the third candidate moves by %.3g with the poses" % (stereo, f["Cw"], min(gaps), moved))
        assert min(gaps) > 1e-6
        # S of the first candidate on the prior (the later ones meet a covariance the oracle keeps to itself)
        Hx, Hf, res, _ = L.reference_rows(f, f["table"], H.T_GOOD)
        _, _, cidx = H.window_of(f["table"])
        cols = np.concatenate([np.arange(i, i + 6) for i in cidx])
        Hu = np.linalg.qr(Hf, mode="complete")[0].T[3:] @ Hx
        assert np.linalg.eigvalsh(Hu @ f["P"][np.ix_(cols, cols)] @ Hu.T + H.NOISE ** 2 * np.eye(Hu.shape[0])).min() > 0.0
