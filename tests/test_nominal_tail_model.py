"""The landmark tail of a frame as ONE congruence (ingvio_nominal_tail), checked without a GPU.

The device kernels compute S T P T^T S^T in one sweep; the reference (LandmarkUpdate.cpp:273-361, StateManager.cpp:639-693, :155-192,
:340-353) replaces landmark by landmark and marginalises variable by variable.  Here the numpy model of the joint form
(closed_loop_tail.joint_tail, integer bookkeeping included) is compared with the C oracle applied sequentially
(closed_loop_tail.sequential_tail on oracle.Cov), and the teeth of the GPU tests are asserted on the oracle alone."""
import copy

import numpy as np
import pytest

from ingvio_amd import closed_loop_tail as clt
from ingvio_amd.closed_loop import SIZE

WINDOWS = (3, 6, 11, 12)
LANDMARKS = (0, 1, 3, 6)


def scenario(C, n_lm, two):
    """the case of a window / landmark count: GNSS scalars behind the start window's clones for every other one, the last landmark behind
    the new anchor when there are at least three, one erased when there are six"""
    marg = ((0, 2) if C >= 4 else (0, 1)) if two else (0,)
    behind = (n_lm - 1,) if n_lm >= 3 else ()
    erase = (1,) if n_lm >= 6 else ()
    return clt.synthetic_case(C, n_lm, seed=100 * C + 10 * n_lm + two, gnss=(C + n_lm) % 2 == 0, marg_pos=marg, behind=behind, erase=erase,
                              hole=n_lm == 3)


def ints(t):
    return [None if s is None else (s["kind"], s["idx"], s["anchor"]) for s in t.slots], list(t.clones)


@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("n_lm", LANDMARKS)
@pytest.mark.parametrize("C", WINDOWS)
def test_joint_form_equals_the_sequential_oracle(C, n_lm, two):
    from oracle import oracle as orc
    case = scenario(C, n_lm, two)
    P, plan = case["P"], case["plan"]
    ts, tj = copy.deepcopy(case["table"]), copy.deepcopy(case["table"])
    cov = orc.Cov(P)
    vs, depth = clt.sequential_tail(cov, ts, plan)
    Pj, vj = clt.joint_tail(P, tj, plan)
    assert vs == vj
    assert all(abs(z) >= 0.1 for z in depth), depth
    assert ints(ts) == ints(tj)
    gone = sum(SIZE[case["table"].slots[sl]["kind"]] for sl in plan["erase_slot"] + plan["marg_slot"]) + 3 * vs.count(0)
    assert cov.n == Pj.shape[0] == P.shape[0] - gone
    err = np.max(np.abs(cov.P - Pj)) / np.max(np.abs(cov.P))
    assert err <= 1e-13, err
    if case["gnss_slots"][0] >= 0:                                       # the clocks lie behind clones that left: they moved down
        for g in case["gnss_slots"]:
            assert ts.slots[g]["idx"] == case["table"].slots[g]["idx"] - 6 * len(plan["marg_slot"])
    for s0, s1 in zip(case["table"].slots, tj.slots):                     # no value of a surviving variable moves
        if s1 is not None:
            assert all(np.array_equal(s0[k], s1[k]) for k in ("R", "p", "v"))
    if n_lm >= 3:
        assert 0 in vs and 1 in vs


def test_plans_cover_what_the_gpu_tests_claim():
    """a landmark anchored to a clone that stays is left out of the plan; with two clones leaving, landmarks hang on both"""
    case = scenario(11, 6, 1)
    t, plan = case["table"], case["plan"]
    assert len(plan["marg_slot"]) == 2 and len(plan["lm_slot"]) < 6 - len(plan["erase_slot"])
    assert {t.slots[sl]["anchor"] for sl in plan["lm_slot"]} == set(plan["marg_slot"])


@pytest.mark.parametrize("C,n_lm", [(6, 3), (11, 6)])
def test_skipping_the_anchor_change_is_far_outside_the_gpu_tolerance(C, n_lm):
    """marginalise only, without replaceVarLinear: the columns of the re-anchored landmarks differ by far more than 1e-11"""
    from oracle import oracle as orc
    case = scenario(C, n_lm, 0)
    t0, t1 = copy.deepcopy(case["table"]), copy.deepcopy(case["table"])
    c0, c1 = orc.Cov(case["P"]), orc.Cov(case["P"])
    v0, _ = clt.sequential_tail(c0, t0, case["plan"])
    clt.sequential_tail(c1, t1, case["plan"], reanchor=False)
    P0, P1 = c0.P, c1.P
    hit = 0
    for sl, v in zip(case["plan"]["lm_slot"], v0):
        if v:
            L = t0.slots[sl]["idx"]
            d = np.max(np.abs(P0[:, L:L + 3] - P1[:, L:L + 3])) / np.max(np.abs(P0))
            assert d >= 1e-6, (sl, d)
            hit += 1
    assert hit >= 1
