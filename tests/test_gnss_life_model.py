"""The GNSS scalars' life cycle in the device loop (ingvio_set_gnss_adjust_yof, ingvio_nominal_add_gnss, ingvio_nominal_marg_gnss; DESIGN
4.11) without a GPU: the exports are declared and wrapped, the numpy yaw-offset columns of ingvio_amd/closed_loop_gnss_life.py are the
reference's (the update rows against the shim's C++ transcription, the acquisition rows against the formula as the reference writes
it), and the scenario of tests/test_gpu_gnss_life.py does on the ORACLE alone what the GPU tests rely on."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from ingvio_amd import closed_loop_gnss_life as gl
from ingvio_amd.closed_loop_gnss import R_ENU, rot_z
from ingvio_amd.closed_loop_gnss_init import oracle_records, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4


@pytest.fixture(scope="module")
def cases():
    return gl.make_life_loop(load_golden("gnss_front"), B)


def test_the_header_declares_the_exports_and_capi_wraps_them():
    from ingvio_amd import capi
    hdr = open(os.path.join(ROOT, "include", "ingvio_hip.h")).read()
    want = {"ingvio_set_gnss_adjust_yof": ("ingvio_ctx* ctx", "int on"),
            "ingvio_nominal_add_gnss": ("int b0", "int nb", "const int* gtype", "const double* value", "const double* var", "int* slot_out", "int* idx_out"),
            "ingvio_nominal_marg_gnss": ("int b0", "int nb", "const unsigned* mask")}
    for name, pieces in want.items():
        decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, "include/ingvio_hip.h does not declare " + name
        args = " ".join(re.sub(r"/\*.*?\*/", " ", decl.group(1), flags=re.S).split())
        for piece in pieces:
            assert piece in args, (name, piece)
        assert name in capi.EXPORTS
    for meth in ("set_gnss_adjust_yof", "nominal_add_gnss", "nominal_marg_gnss"):
        assert callable(getattr(capi.Context, meth))


def test_the_cases_keep_the_yaw_offset_column_away_from_rounding(cases):
    """every tested filter: horizontal |p_w| >= 1 m and |v_w| >= 0.1 m/s, windows of 5-8 clones, 8 satellites of three constellations, and
    a start state without a GNSS scalar"""
    assert sorted(c["C"] for c in cases) == [5, 6, 7, 8]
    for c in cases:
        e = c["table"].slots[c["table"].v_pose]
        assert np.linalg.norm(e["p"][:2]) >= 1.0 and np.linalg.norm(e["v"][:2]) >= 0.1
        assert c["gnss_slots"] == [-1] * 6 and not any(s is not None and s["kind"] == 3 for s in c["table"].slots)
        assert gl.check_state_continuity(c["table"], c["P"].shape[0])
        for f, ep in enumerate(c["epochs"]):
            sys = sorted(set(ep["eph"][:, 0].astype(int)))
            assert sys == ([0, 3] if gl.SCRIPT[f].get("absent") == gl.DROP else [0, 2, 3]) and 6 <= len(ep["eph"]) <= 10


def test_update_rows_equal_the_shims_transcription(cases):
    """update_rows (numpy) against host.gnss_rows with adjust_yof - host/GnssUpdate.cpp's transcription of GnssUpdate.cpp:148-272 - on
    the same satellite records: every entry to 1e-13 (relative to the row's scale), the yaw-offset column at least 0.1 in size"""
    from ingvio_amd import host
    for b, c in enumerate(cases):
        e = c["table"].slots[c["table"].v_pose]
        ep = dict(c["epochs"][1], p_w=e["p"], v_w=e["v"], cb=[150.0, 0.0, 160.0, 180.0], fs=5.0, yaw_offset=c["yof"],
                  idx_se23=e["idx"], idx_yof=40, idx_fs=41, idx_cb=[42, -1, 44, 43])
        rec = oracle_records(ep)
        vidx, vsize, H, res, Rd, sats = gl.update_rows(ep, rec, True)
        eph, obs = ep["eph"][sats], ep["obs"][sats]
        g = dict(los=rec[sats, 2:5], sys=eph[:, 0].astype(int), res_pos=rec[sats, 0], res_vel=rec[sats, 1], sin_el=np.sin(rec[sats, 6]), ura=eph[:, 24],
                 psr_std=obs[:, 3], dopp_std_mps=obs[:, 4] * 2.99792458e8 / obs[:, 5], R_w2ecef=R_ENU @ rot_z(c["yof"]), p_w=e["p"], v_w=e["v"],
                 idx_se23=e["idx"], idx_yof=40, idx_cb=[42, -1, 44, 43], idx_fs=41, adjust_yof=True, R_enu2ecef=R_ENU, yaw_offset=c["yof"])
        hv, hs, Hh, rh, Rh = host.gnss_rows(g)
        assert list(hv) == vidx and list(hs) == vsize and Hh.shape == H.shape == (16, 14), (b, hv, vidx)
        scale = 1.0 + np.linalg.norm(e["p"])
        assert np.abs(H - Hh).max() <= 1e-13 * scale, (b, np.abs(H - Hh).max())
        assert np.array_equal(res, rh) and np.abs(Rd - Rh).max() <= 1e-13 * Rh.max()
        assert np.abs(H[:, 9]).max() >= 0.1 and np.abs(H[:8, 9]).min() > 0.0, (b, H[:, 9])
        H0 = gl.update_rows(ep, rec, False)[2]
        assert not H0[:, 9].any() and np.array_equal(np.delete(H0, 9, axis=1), np.delete(H, 9, axis=1))


def test_acquisition_rows_follow_the_reference_as_written(cases):
    """column 9 of the acquisition rows is -u^T R_enu2ecef^T dRz(yaw) x (GnssUpdate.cpp:401-404, :462-465: getRecef2enu()), spelled out
    here entry by entry, and differs from the update rows' column on the same inputs - the guard against "fixing" the quirk"""
    for b, c in enumerate(cases):
        e = c["table"].slots[c["table"].v_pose]
        ep = dict(c["epochs"][0], p_w=e["p"], v_w=e["v"], cb=[150.0, 0.0, 160.0, 180.0], fs=5.0, yaw_offset=c["yof"])
        rec = oracle_records(ep)
        yaw = c["yof"]
        Rw = R_ENU @ rot_z(yaw)
        for g, x in ((0, e["v"]), (1, e["p"]), (3, e["p"]), (4, e["p"])):
            Hx, res, noise, sats = rows_of(g, ep, rec, Rw, x, yaw)
            H0 = rows_of(g, ep, rec, Rw, x)[0]
            assert len(sats) >= 2 and not H0[:, 9].any() and np.array_equal(Hx[:, :9], H0[:, :9])
            cy, sy = np.cos(yaw), np.sin(yaw)
            d = np.array([-sy * x[0] - cy * x[1], cy * x[0] - sy * x[1], 0.0])
            for r, i in enumerate(sats):
                u = rec[i, 2:5]
                want = -sum(u[k] * sum(R_ENU[j, k] * d[j] for j in range(3)) for k in range(3))      # R_enu2ecef TRANSPOSED
                assert abs(Hx[r, 9] - want) <= 1e-13 * (1.0 + np.linalg.norm(x)), (b, g, r)
            col = gl.acquire_yof_column(rec[sats, 2:5], R_ENU, yaw, x)
            upd = gl.update_yof_column(rec[sats, 2:5], R_ENU, yaw, x)
            assert np.abs(Hx[:, 9] - col).max() <= 1e-13 * (1.0 + np.linalg.norm(x))
            assert np.abs(col).max() >= 0.05 and np.abs(col - upd).max() >= 0.05, (b, g, col, upd)


@pytest.mark.parametrize("adjust", [True, False])
def test_the_host_loop_on_the_oracle_alone(cases, orc, adjust):
    """YOF enters, FS and three clocks are acquired, an epoch updates, the Galileo clock leaves and is acquired again;
    checkStateContinuity after every step; the yaw offset is estimated exactly when the switch is on"""
    from ingvio_amd import synth
    table = synth.chi2_table()
    for b, c in enumerate(cases):
        steps = []

        def check(step, tab, slots, cov):
            steps.append(step)
            assert gl.check_state_continuity(tab, cov.n), (b, step)
            P = cov.P
            assert np.array_equal(P, P.T) or np.abs(P - P.T).max() <= 1e-12 * np.abs(P).max(), (b, step)
        n0 = c["P"].shape[0]
        tab, slots, P, log = gl.oracle_life(c, table, adjust, check)
        assert steps == ["add_yof", "acquire", "update", "drop", "update_without", "reacquire", "update_again"]
        by = {l["step"]: l for l in log}
        assert by["add_yof"]["idx"] == n0 and by["add_yof"]["n"] == n0 + 1
        assert by["acquire"]["added"] == [0, 1, 3, 4] and by["acquire"]["n"] == n0 + 5                  # FS, GPS, GAL, BDS; no GLONASS satellite
        assert by["drop"]["gone"] == [n0 + 3] and by["drop"]["n"] == n0 + 4                             # Galileo's clock, between GPS's and BeiDou's
        assert by["reacquire"]["added"] == [3] and by["reacquire"]["n"] == n0 + 5
        assert (by["update"]["rows"], by["update_without"]["rows"], by["update_again"]["rows"]) == (16, 12, 16)
        assert all(by[s]["rc"] == 0 for s in ("update", "update_without", "update_again"))
        yo = tab.slots[slots[gl.YOF]]
        var = P[yo["idx"], yo["idx"]]
        if adjust:
            assert min(by[s]["col9"] for s in ("update", "update_without", "update_again")) >= 0.1
            assert var < gl.INIT_COV_YOF and yo["p"][0] != c["yof"], (b, var, yo["p"][0])
        else:
            assert by["update"]["col9"] == 0.0 and var == gl.INIT_COV_YOF and yo["p"][0] == c["yof"], (b, var)
        assert slots[1] == -1 and all(slots[s] >= 0 for s in (0, 2, 3, 4, 5))


def test_add_and_marg_on_the_host_table():
    """table_add_gnss takes the lowest free slot; table_marg_gnss shifts every surviving idx by the removed columns below it"""
    from ingvio_amd.closed_loop import HostTable
    mk = lambda kind, idx: dict(kind=kind, idx=idx, anchor=-1, R=np.eye(3), p=np.zeros(3), v=np.zeros(3))
    tab = HostTable([mk(0, 0), None, mk(2, 9), mk(1, 12), None], [3], -1, 0, 2, -1, np.zeros(3))
    slots = [-1] * 6
    assert gl.table_add_gnss(tab, slots, 5, 18, 0.3) == 1 and gl.table_add_gnss(tab, slots, 4, 19, 5.0) == 4
    assert gl.table_add_gnss(tab, slots, 0, 20, 1.0) == 5 and len(tab.slots) == 6
    tab.slots.append(mk(1, 21))
    assert gl.check_state_continuity(tab, 27) and not gl.check_state_continuity(tab, 26)
    gone = gl.table_marg_gnss(tab, slots, (1 << 5) | (1 << 0))
    assert gone == [18, 20] and slots == [-1, -1, -1, -1, 4, -1]
    assert tab.slots[4]["idx"] == 18 and tab.slots[6]["idx"] == 19 and tab.slots[1] is None and tab.slots[5] is None
    assert gl.check_state_continuity(tab, 25)
