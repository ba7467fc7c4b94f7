"""The 80-bit reference of the generic EKF update (tests/ekf_cases.py) against itself and against the float64 oracle.  No GPU.

tests/test_gpu_ekf_routes.py holds the kernels to 1e-11 (LDS route) / 1e-10 (dense routes) of the reference.  That only means
something where the formula itself is determined well below those figures: the float64 oracle - another evaluation of the same
formula, LU instead of Cholesky - has to land within 1e-12 of the reference on every case of that matrix.  A case that does not
is ill-posed for the purpose and gets a lower cond in ekf_cases.py; the bound stays."""
import numpy as np
import pytest

import ekf_cases as ec

ORACLE_TOL = 1e-12

GROUPS = {
    "lds": ec.LDS_CASES,
    "capacity": ec.CAP_LDS_CASES + ec.CAP_DENSE_CASES + [ec.CAP_EDGE],
    "dense_reg": [c for _, cs in ec.DENSE_REG.values() for c in cs] + [ec.DENSE_REG_SMALL],
    "sweep": ec.SWEEP_CASES + [ec.SWEEP_SMALL],
    "pingpong_shrunk": list(ec.PINGPONG.values()) + [ec.SHRUNK_BIG, ec.SHRUNK],
    "batch_lds": [c for cs in ec.BATCH_LDS.values() for c in cs] + ec.BATCH_LDS_SIZING,
    "batch_dense": ec.BATCH_MIXED + ec.BATCH_GEMM64 + [ec.BATCH_SPLIT[i] for i in ec.BATCH_SPLIT_LD],
    "gates": ec.GATE_CASES + [ec.GATE_FIT],
    "not_pd_neighbours": [c for kinds in ec.NOT_PD_NEIGHBOURS.values() for pair in kinds.values() for c in pair],
}


def test_groups_cover_the_matrix():
    listed = [c for cs in GROUPS.values() for c in cs]
    assert sorted(listed) == sorted(ec.reference_cases()) and len(set(listed)) == len(listed)


def test_var_orders():
    """non-adjacent blocks in non-ascending order inside the state; the whole state as one block and a single scalar column occur"""
    whole = scalar = False
    for c in ec.reference_cases() + ec.BATCH_SPLIT + list(ec.NOT_PD.values()):
        n_live = c.n - ec.MARG_SIZE if c.marg else c.n
        vo, vs = ec.var_order(n_live, c.nc)
        assert sum(vs) == c.nc and min(vs) >= 1 and min(vo) >= 0
        spans = sorted(zip(vo, vs))
        assert all(a + s < b for (a, s), (b, _) in zip(spans, spans[1:])), c          # a gap between any two blocks
        assert spans[-1][0] + spans[-1][1] <= n_live
        if len(vo) > 1:
            assert list(vo) != sorted(vo), c
        whole |= vs == [n_live]
        scalar |= vs == [1]
    assert whole and scalar


def test_reference_closed_form_one_row():
    """one row: P+ = P - Pc h^T h Pc^T / s, dx = Pc h^T r / s, gamma = r^2 / s with s = h Pcc h^T + R"""
    c = ec.case(49, 1, 17, "scalar", tag="closed")
    d = ec.inputs(c)
    Pn, dx, gam = ec.expected(c)
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63                    # the x87 extended format: 11 bits more than float64
    P = d["P"].astype(LD); h = d["H"].astype(LD)[0]
    cols = np.concatenate([np.arange(i, i + s) for i, s in zip(d["vidx"], d["vsize"])])
    k = P[:, cols] @ h
    s = h @ k[cols] + LD(d["R"])
    r = LD(d["res"][0])
    assert ec.rel(Pn, (P - np.outer(k, k) / s).astype(np.float64)) < 1e-15
    assert ec.rel(dx, (k * r / s).astype(np.float64)) < 1e-15
    assert abs(gam - float(r * r / s)) < 1e-15 * float(r * r / s)
    assert np.array_equal(Pn, Pn.T)


def test_reference_reports_not_pd():
    for c in ec.NOT_PD.values():
        d = ec.inputs(c)
        for kind in ("scalar", "diag", "full"):
            assert ec.reference_update(d["prior"], d["vidx"], d["vsize"], d["H"], d["res"], ec.not_pd_noise(c.m, kind)) is None


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_oracle_within_1e12_of_reference(orc, group):
    """the float64 oracle's ekfUpdate / whitenResidual within 1e-12 of the 80-bit reference on P+, dx and gamma"""
    worst = [0.0, 0.0, 0.0, None]
    for c in GROUPS[group]:
        d = ec.inputs(c)
        Pn, dx, gam = ec.expected(c)
        oc = orc.Cov(d["prior"])
        g = oc.whiten(d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
        dxo, _ = oc.ekf_update(d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
        eP, ex, eg = ec.rel(oc.P, Pn), ec.rel(dxo, dx), abs(g - gam) / max(1.0, gam)
        if max(eP, ex, eg) > max(worst[:3]):
            worst = [eP, ex, eg, c.name]
        assert eP < ORACLE_TOL and ex < ORACLE_TOL and eg < ORACLE_TOL, (c.name, eP, ex, eg)
    print("oracle vs 80-bit, %s: worst case %s  P+ %.2e  dx %.2e  gamma %.2e" % (group, worst[3], *worst[:3]))
