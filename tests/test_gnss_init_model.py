"""ingvio_gnss_init_nominal without a GPU: the export is declared and wrapped, and the scenario of tests/test_gpu_gnss_init.py does on
the ORACLE alone what the GPU tests rely on - otherwise they could pass vacuously.  If a condition here fails, the scenario
(ingvio_amd/closed_loop_gnss_init.py::MIXED) is what has to change, not the assertion."""
import copy
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from conftest import rel_err as rel
from ingvio_amd.closed_loop_gnss_init import CAND, candidates, make_mixed, oracle_acquire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9                               # the tolerance of the GPU comparisons (tests/test_gpu_nominal_gnss.py)


def test_the_header_declares_the_export_and_capi_wraps_it():
    from ingvio_amd import capi
    hdr = open(os.path.join(ROOT, "include", "ingvio_hip.h")).read()
    assert re.search(r"#define\s+INGVIO_GNSS_INIT_CAND\s+5\b", hdr)
    assert re.search(r"\}\s*ingvio_gnss_init_block\s*;", hdr)
    decl = re.search(r"int\s+ingvio_gnss_init_nominal\s*\(([^;]*)\)\s*;", hdr)
    assert decl, "include/ingvio_hip.h does not declare ingvio_gnss_init_nominal"
    args = " ".join(decl.group(1).split())
    for piece in ("const ingvio_gnss_init_block* blocks", "const double* chi2_table", "int chi2_len", "double chi2_mult", "int do_chi2",
                  "int* added", "int* new_idx", "int* slot", "double* chi2", "double* noise", "double* dx", "int* status"):
        assert piece in args, piece
    assert re.search(r"int\s+ingvio_debug_gnss_init_rows\s*\(", hdr)
    assert "ingvio_gnss_init_nominal" in capi.EXPORTS and "ingvio_debug_gnss_init_rows" in capi.EXPORTS
    assert capi.GNSS_INIT_CAND == 5
    assert callable(capi.Context.gnss_init_nominal) and callable(capi.Context.debug_gnss_init_rows)
    # the block's layout: the nominal epoch first, then posSpp [7] and velSpp [4]
    assert [f[0] for f in capi.GnssInitBlock._fields_] == ["epoch", "pos_spp", "vel_spp"]
    assert capi.GnssInitBlock.pos_spp.offset == capi.GnssInitBlock.epoch.size and capi.GnssInitBlock.vel_spp.offset == capi.GnssInitBlock.pos_spp.offset + 56
    arr, keep = capi.make_gnss_init_blocks([None, dict(epoch=None, pos_spp=np.arange(7.0), vel_spp=np.arange(4.0))])
    assert arr[0].epoch.n_sat == 0 and arr[1].epoch.n_sat == 0 and list(arr[1].pos_spp) == list(range(7)) and arr[1].vel_spp[3] == 3.0


@pytest.fixture(scope="module")
def acquired(orc):
    from ingvio_amd import synth
    cases = make_mixed(load_golden("gnss_front"))
    table = synth.chi2_table()
    out = []
    for c in cases:
        tab, slots = copy.deepcopy(c["table"]), list(c["gnss_slots"])
        ver, P = oracle_acquire(c["P"], tab, slots, c["epochs"][0], c["spp"], table)
        out.append((ver, P, tab, slots))
    return cases, table, out


def test_the_mixed_scenario_adds_refuses_and_skips_on_the_oracle(acquired):
    cases, table, out = acquired
    added = refused = skipped = 0
    for b, (c, (ver, P, tab, slots)) in enumerate(zip(cases, out)):
        m = c["mixed"]
        cands = candidates(c["gnss_slots"], c["spp"]) if not m.get("no_epoch") else []
        assert cands == ([] if m.get("no_epoch") else sorted(m["removed"])), b
        for g in range(CAND):
            v = ver[g]
            if g not in cands:
                assert not v["added"] and v["chi2"] == 0.0, (b, g)
                continue
            if m.get("one_glo") and g == 2:                              # exactly the m = 1 candidates are skipped
                assert v["m"] == 1 and not v["added"] and v["chi2"] == 0.0, (b, g, v)
                skipped += 1
            elif m.get("bds_outlier") and g == 4:                        # exactly the constellations with the outlier are refused
                assert v["m"] >= 2 and not v["added"] and v["chi2"] > 0.95 * table[v["m"]], (b, g, v)
                refused += 1
            else:
                assert v["m"] >= 2 and v["added"] and 0.0 < v["chi2"] <= 0.95 * table[v["m"]], (b, g, v)
                assert v["new_idx"] == c["P"].shape[0] + sum(ver[q]["added"] for q in range(g)), (b, g)
                added += 1
        n_add = sum(ver[g]["added"] for g in range(CAND))
        assert P.shape[0] == c["P"].shape[0] + n_add, b
        if not n_add:
            assert np.array_equal(P, c["P"]), b
    assert added >= 20 and refused == 2 and skipped == 1, (added, refused, skipped)
    # a refused candidate leaves its slot free: the next accepted one still takes the slot reserved for IT
    for b, (c, (ver, P, tab, slots)) in enumerate(zip(cases, out)):
        taken = [ver[g]["slot"] for g in range(CAND) if ver[g]["added"]]
        assert len(set(taken)) == len(taken) and all(tab.slots[s]["kind"] == 3 for s in taken), b


def test_reading_p_v_once_moves_the_second_candidates_posterior(acquired, orc):
    """the "moved state" filter: FS's trailing update moves p_w, which the GPS clock's rows are linearised at (GnssUpdate.cpp:458)"""
    cases, table, out = acquired
    b = next(i for i, c in enumerate(cases) if c["mixed"].get("moved"))
    c = cases[b]
    ver, P = out[b][0], out[b][1]
    assert all(ver[g]["added"] for g in range(CAND)), [ver[g]["added"] for g in range(CAND)]
    tab, slots = copy.deepcopy(c["table"]), list(c["gnss_slots"])
    ver1, P1 = oracle_acquire(c["P"], tab, slots, c["epochs"][0], c["spp"], table, read_once=True)
    assert all(ver1[g]["added"] for g in range(CAND))
    assert np.array_equal(ver1[0]["dx"], ver[0]["dx"])                   # the first candidate sees the same state either way
    d = rel(ver1[1]["dx"], ver[1]["dx"])
    assert d > 100 * TOL, d
    assert rel(P1, P) > 100 * TOL, rel(P1, P)
