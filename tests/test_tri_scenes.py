"""The inputs of tests/test_gpu_triangulation_classes.py judged by the oracle alone (tests/tri_scenes.py), before anything reaches a
device: every gate class a case claims to exercise is hit at least 10 times, at least 30 % of the features are accepted (two cases
cannot: see tri_scenes.GATE_CASES), at most 1 % of the features sit on a branch boundary, the shaped masks do what their names say,
and the behind-the-anchor scene holds points behind their anchor."""
import numpy as np
import pytest

import tri_scenes as ts


@pytest.mark.parametrize("case,stereo,C", [pytest.param(case, stereo, C, id="%s-%s%d" % (case.name, "stereo" if stereo else "mono", C))
                                           for case in ts.GATE_CASES for stereo, C in ts.GATE_PAIRS if C in case.windows])
def test_gate_cases_bite(case, stereo, C):
    t = ts.assert_bites(ts.gate_keys(stereo, C, case.noise), case, C)
    print("gate", case.name, stereo, C, t)


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("c_max", ts.CMAXES)
@pytest.mark.parametrize("full", [True, False])
def test_class_scenes_bite(full, c_max, stereo):
    keys = ts.class_keys(stereo, c_max, full)
    t = ts.tally(keys)
    assert t["few"] >= 10 and t["accepted"] >= 0.3 * t["features"] and t["marginal"] <= 0.01 * t["features"], t
    Cs = [k[1] for k in keys]
    assert (min(Cs) == c_max) if full else (max(Cs) < c_max and len(set(Cs)) > 1)
    Fs = [k[2] for k in keys]
    assert 0 in Fs and any(F % 8 for F in Fs) and max(Fs) == ts.F_DEF


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("C", [9, 12, 24, 32, 36])
def test_mask_shapers(C, stereo):
    key = (7, C, 16, stereo, ts.NOISE)
    fr = ts.scene(*key); jd = ts.judged(key)
    n = [ts.n_obs(m, C, stereo) for m in fr["obs_mask"][:ts.N_EDGE]]
    eyes = 2 if stereo else 1
    assert n[0] == 4 and not jd.ok[0] and jd.gate[0] == "few" and not jd.pf[0].any()
    assert n[1] == (6 if stereo else 5) and jd.gate[1] != "few"
    assert n[2] == eyes * C and int(fr["obs_mask"][2]) == (1 << C) - 1
    k = 3 if stereo else 6
    assert int(fr["obs_mask"][3]) == (1 << k) - 1 and int(fr["obs_mask"][4]) == ((1 << k) - 1) << (C - k)
    assert not (int(fr["obs_mask"][5]) >> (C - 1)) & 1 and n[5] == eyes * (C - 1)
    dirty, clean = int(fr["obs_mask"][6]), int(fr["obs_mask"][7])
    assert dirty >> C == (1 << (64 - C)) - 1 and dirty & ((1 << C) - 1) == clean and clean < (1 << C)
    assert np.array_equal(fr["uv"][6], fr["uv"][7]) and jd.ok[6] == jd.ok[7] and np.array_equal(jd.pf[6], jd.pf[7])
    # the register share of a lane is exactly full where the issue's shapes say so
    assert ts.instantiation(True, 12, 24) == (True, 6, 4) and ts.instantiation(False, 24, 24) == (False, 6, 4)
    assert ts.instantiation(True, 32, 2) == (True, 4, 16) and ts.instantiation(True, 36, 2) == (True, 0, 16)


def test_instantiations_cover_every_reachable_class():
    seen = {ts.instantiation(s, c, nb) for s in (True, False) for c in ts.CMAXES for nb in (3, 24)}
    assert seen == {(True, 4, 16), (True, 0, 16), (False, 4, 16), (True, 6, 4), (True, 0, 4), (False, 6, 4), (False, 0, 4)}
    # <false, 0, 16> needs a mono window of more than 64 clones
    assert all(ts.instantiation(False, c, 2)[1] == 4 for c in range(1, 65))


@pytest.mark.parametrize("stereo", [True, False])
def test_behind_anchor_scene(stereo):
    for key in ts.behind_keys(stereo):
        fr = ts.behind_frame(key); jd = ts.judged(key)
        behind = [j for j in range(len(jd.ok)) if jd.ok[j] and ts.anchor_depth(fr, j, jd.pf[j]) <= 0]
        front = [j for j in range(len(jd.ok)) if jd.ok[j] and ts.anchor_depth(fr, j, jd.pf[j]) > 0]
        assert len(behind) >= 5 and len(front) > 20
        assert all(fr["anchor"][j] == ts.AWAY for j in behind) and not any((int(m) >> ts.AWAY) & 1 for m in fr["obs_mask"])
        assert not jd.marginal.any()


def test_nan_measurement_quirk():
    """a NaN in an observed measurement makes every comparison false: the oracle, like the reference, accepts the initial guess of
    a share of such features.  Kept as it is; the GPU test asserts parity with it."""
    key = ts.gate_keys(True, 11)[0]
    fr = ts.nan_frame(ts.scene(*key))
    oks = [ts.oracle_feature(fr, j)[0] for j in range(0, ts.F_DEF, 2)]
    assert 5 <= sum(oks) < len(oks)
    assert all(np.isnan(fr["uv"][j]).sum() == 1 for j in range(0, ts.F_DEF, 2))
    assert not np.isnan(fr["uv"][1::2]).any()
