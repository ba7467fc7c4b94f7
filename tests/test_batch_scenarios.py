"""The scenarios of tests/test_gpu_batch_paths.py, checked against the oracle alone (no GPU): each batch is what it claims to be.
These are conditions on the INPUTS of the GPU tests - a later change of ingvio_amd.synth that hollowed them out (no feature
accepted, one state size, a role missing) fails here instead of passing there silently."""
import numpy as np
import pytest

import batch_scenarios as bs


@pytest.mark.parametrize("C,stereo", [(11, True), (11, False), (16, True), (16, False)])
def test_mixed_batch_is_what_it_claims(orc, C, stereo):
    desc = bs.mixed_desc(C, stereo, 70)
    cases = bs.build_batch(orc, 1000 * C + (0 if stereo else 500), desc)
    n_max = bs.n_max_of(cases)
    ld = (n_max + 15) // 16 * 16
    roles = [c[3]["role"] for c in cases]
    for r in bs.ROLES:
        assert roles.count(r) >= 2, r
    # tile counts of the posterior (what k_info_apply sweeps), at least three; the largest filter fills the context, the smallest one
    # leaves the second workgroup of its share idle (2 * part * 4 >= nt at part = 1) while the launch has two per filter
    nt = [(c[3]["N_update"] - (6 if c[1]["marg_idx"] >= 0 else 0) + 15) // 16 for c in cases]
    assert len(set(nt)) >= 3, sorted(set(nt))
    wgpf = (((n_max + 15) // 16 + 1) // 2 + 3) // 4
    assert wgpf >= 2 and min(nt) <= 8 and cases[0][3]["N_update"] == n_max
    marg = [c[1]["marg_idx"] >= 0 for c in cases]
    empties = [b for b, r in enumerate(roles) if r == "empty"]
    assert any(marg[b] for b in empties) and any(not marg[b] for b in empties)
    assert all(marg[b] for b, r in enumerate(roles) if r in ("ordinary", "rejected")) and not any(marg[b] for b, r in enumerate(roles) if r == "inplace")
    # consecutive steps fit: a filter that does not marginalise grows by six per step
    for c in cases:
        if c[1]["marg_idx"] < 0:
            assert c[3]["N_update"] + 12 <= n_max
    want = bs.oracle_steps(orc, cases, ld)[0]
    good = 0
    for b, (P, dx, acc, n) in enumerate(want):
        F = cases[b][3]["F"]
        assert n == cases[b][3]["N_update"] - (6 if marg[b] else 0)
        if roles[b] in ("rejected", "empty"):
            assert not acc.any() and not dx.any(), (b, roles[b])
        else:
            assert acc.sum() >= 1, b
            good += acc.sum() > F / 4
    n_upd = sum(r in ("ordinary", "inplace") for r in roles)
    assert good >= 0.9 * n_upd, (good, n_upd)


@pytest.mark.parametrize("C,stereo,selected", [(4, False, 0), (6, True, 0), (9, False, 0), (12, True, 1), (13, False, 0), (22, True, 0), (36, False, 0),
                                               (24, True, 1)])
def test_uniform_batch_accepts_features(orc, C, stereo, selected):
    """the uniform batches of the class sweep (a sample of eight filters each): every filter accepts most of its features"""
    desc = bs.uniform_desc(C, stereo, 8, F=40 if C <= 16 else 48, lm_max=10 if C <= 16 else 8, selected=bool(selected))
    cases = bs.build_batch(orc, 3000 + 10 * C, desc)
    ld = (bs.n_max_of(cases) + 15) // 16 * 16
    assert len({c[3]["N_update"] for c in cases}) >= 3
    for b, (P, dx, acc, n) in enumerate(bs.oracle_steps(orc, cases, ld, selected_variant=selected)[0]):
        assert acc.sum() > cases[b][3]["F"] / 4 and dx.any(), (b, acc.sum())
        assert np.array_equal(P, P.T)


def test_update_time_prior_equals_the_frame_path(orc):
    """prior_at_update + Cov.msckf_update + marginalize == orc.frame_update: what the sub-range and few-versus-many tests rely on"""
    cases = bs.build_batch(orc, 77, bs.mixed_desc(11, True, 8))
    ld = (bs.n_max_of(cases) + 15) // 16 * 16
    want = bs.oracle_steps(orc, cases, ld)[0]
    for b, case in enumerate(cases):
        oc = orc.Cov(bs.prior_at_update(orc, case, ld), ld=ld)
        dx, acc, gam, m = oc.msckf_update(case[2], max_accept=0, compress_rule=1)
        if case[1]["marg_idx"] >= 0:
            oc.marginalize(case[1]["marg_idx"], 6)
        assert np.array_equal(acc, want[b][2]) and np.array_equal(oc.P, want[b][0]) and np.array_equal(dx, want[b][1]), b
