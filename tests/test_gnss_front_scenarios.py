"""k_gnss_front (kernels_gnss.hip) away from the one recorded instant of tests/golden/gnss_front.npz: the scenarios of
tests/gnss_scenarios.py - hemispheres, latitude bands, height cut-offs, Klobuchar clamps, week wrap, GLONASS step counts, the BeiDou
GEO frame, eccentric orbits, satellites below the horizon, a receiver on the polar axis and at the origin, unusable entries, 1 and 64
satellites - and a ragged batch of epochs through the row assembly and the update.

CPU part: every scenario reaches the branch it was built for and keeps its distance from every step function (device and host libm
differ in the last bits; no branch may hang on them); the C oracle and the numpy transcription agree on all of them.
GPU part: the kernel's per-satellite records against the oracle for all scenarios in one launch; candidate rows, per-row gates,
block gate and update against a chain made from the oracle alone; the same through the table-reading instantiation.
Tolerances are the ones tests/test_gnss_front.py and tests/test_gvio_aligner.py already hold the kernel and the oracle to."""
import math

import numpy as np
import pytest

import gnss_scenarios as gs
from conftest import rel_err
from oracle import gen_gnss_golden as gg

C_LIGHT = 2.99792458e8
# field -> (columns of a front record, key / columns of the oracle's result, tolerance oracle vs transcription, tolerance kernel vs oracle)
FIELDS = (("res_pos", [0], "res_pos", None, 1e-6, 1e-6), ("res_vel", [1], "res_vel", None, 1e-9, 1e-9), ("los", [2, 3, 4], "los", None, 1e-13, 1e-12),
          ("azel", [5, 6], "azel", None, 1e-12, 1e-11), ("atmos", [7, 8], "atmos", None, 1e-10, 1e-9), ("sat_pos", [10, 11, 12], "sat", slice(0, 3), 1e-6, 1e-6),
          ("sat_vel", [13, 14, 15], "sat", slice(3, 6), 1e-9, 1e-9), ("sat_clock", [16, 17, 18], "sat", slice(6, 9), 1e-15, 1e-15),
          ("ttx", [19], "sat", slice(9, 10), 1e-9, 1e-9))

IDLE = np.r_[np.zeros(6), math.pi / 2, np.zeros(13)]      # a lane without a usable satellite: elevation pi / 2, everything else 0
_memo = {}


def _col(o, key, sl):
    v = np.asarray(o[key], dtype=float)
    v = v.reshape(len(v), -1)
    return v if sl is None else v[:, sl]


def oracle_results(orc):
    """orc.gnss_residuals of every scenario, once"""
    if "oracle" not in _memo:
        _memo["oracle"] = [orc.gnss_residuals(sc["eph"], sc["obs"], sc["ion"], sc["doy"], sc["xyzt"], sc["velt"]) for sc in gs.scenarios()]
    return _memo["oracle"]


# ---- CPU: the scenarios themselves ------------------------------------------------------------------------------------------------------
def test_scenarios_cover_the_families():
    S = gs.scenarios()
    names = [sc["name"] for sc in S]
    assert len(set(names)) == len(names) >= 40
    for fam in ("site_", "height_", "time_", "orbit_", "iono_", "geometry_", "usable_", "size_"):
        assert any(n.startswith(fam) for n in names), fam
    ns = sorted(len(sc["eph"]) for sc in S)
    assert ns[0] == 1 and ns[-1] == 64 and len(set(ns)) >= 6                 # ragged on purpose
    big = [sc for sc in S if len(sc["eph"]) == 64][0]
    assert [int((big["eph"][:, gg.SYS] == s).sum()) for s in (0, 3, 2, 1)] == [20, 18, 18, 8] and big["obs"][63, gg.FREQ] > 0
    for sc in S:
        assert sc["eph"].shape == (len(sc["obs"]), 25) and sc["obs"].shape[1] == 6 and sc["xyzt"].shape == (7,) and sc["velt"].shape == (4,)
        assert np.isfinite(sc["eph"]).all() and np.isfinite(sc["obs"]).all()
        assert (sc["obs"][:, gg.FREQ] != 0).all()                          # freq = 0 divides by zero: not a defined input
    again = gs.build()                                                       # deterministic: the same bits from the same seeds
    for a, b in zip(S, again):
        assert np.array_equal(a["eph"], b["eph"]) and np.array_equal(a["obs"], b["obs"]) and np.array_equal(a["xyzt"], b["xyzt"])


def test_every_scenario_reaches_its_branch():
    """evaluated with the transcription's own functions; a scenario that misses its branch fails here, so the sweep cannot pass on easy
    inputs"""
    for sc in gs.scenarios():
        p = gs.probe(sc)
        assert sc["branch"](p), sc["name"]
        for s in p["sats"]:
            if s is not None and s["terms"] is not None:                    # the terms the predicates read are the ones gg.iono computes
                assert s["terms"]["delay"] == s["iono"], sc["name"]
    # the named examples of the families, spelled out once more
    by = {sc["name"]: gs.probe(sc) for sc in gs.scenarios()}
    up = lambda n: [s for s in by[n]["sats"] if s is not None and s["azel"] is not None and s["azel"][1] > 0]
    assert all(s["trop"] == 0.0 for s in up("height_-150") + up("height_10100")) and all(s["trop"] != 0.0 for s in up("height_-50") + up("height_9900"))
    assert all(s["iono"] == 0.0 for s in up("height_-1100")) and all(s["iono"] == 0.0 for s in by["geometry_antipode"]["sats"])
    assert [len(s["steps"]) for s in by["orbit_glonass_steps"]["sats"][:6]] == [0, 1, 1, 3, 15, 15]
    for n in ("time_tow100", "time_tow604700"):
        kep = [s for s in by[n]["sats"] if s["sys"] != 1]
        assert all(s["tk"] * s["raw"] < 0 for s in kep) and len(kep) == 8, n
    assert all(abs(s["terms"]["phi_raw"]) > 0.416 for n in ("iono_phi_clamp_north", "iono_phi_clamp_south") for s in up(n))
    assert all(abs(s["terms"]["x"]) < 1.57 for s in up("iono_day")) and all(abs(s["terms"]["x"]) > 1.57 for s in up("iono_night"))
    assert by["geometry_polar_axis"]["lla"].tolist() == [0.0, 0.0, 0.0] and by["geometry_origin"]["rn"] == 0.0
    pole = [sc for sc in gs.scenarios() if sc["name"] == "geometry_polar_axis"][0]
    assert pole["xyzt"][0] == 0.0 and pole["xyzt"][1] == 0.0 and pole["xyzt"][2] > 6.3e6
    # both hemispheres, every latitude band of interpc, eccentricities up to 0.17 are in the sweep
    lats = [p["lla"][0] for p in by.values()]
    assert {min(int(abs(x) / 15.0), 5) for x in lats} >= {0, 1, 2, 3, 4, 5} and min(lats) < -75.0 and max(lats) > 75.0
    assert max(s["e"] for s in by["orbit_eccentric"]["sats"]) == 0.17


def test_margins_from_every_step_function():
    """A condition on the generator, not a measurement: the evaluation point stays >= 50 m from the height cut-offs, every elevation
    >= 1 degree from the horizon, |x| >= 1e-3 from 1.57, and in the clamp scenarios phi >= 1e-3 from +-0.416.  (`hgt < 0 -> 0` is a
    clamp - continuous, like the band edges at 15 and 75 degrees - so the scenarios that sit ON 0 m by design are exempt from that one
    cut-off: on_clamp.  height_-50 lies 50 m from two cut-offs at once; the geodetic round trip costs it a nanometre, allowed as 1e-6 m.)"""
    worst = dict(h=1e9, el=1e9, x=1e9, phi=1e9)
    for sc in gs.scenarios():
        p = gs.probe(sc)
        cuts = [c for c in gs.HEIGHT_CUTS if not (c == 0.0 and sc["on_clamp"])]
        dh = min(abs(p["lla"][2] - c) for c in cuts)
        assert dh >= gs.H_MARGIN - 1e-6, (sc["name"], p["lla"][2])
        worst["h"] = min(worst["h"], dh)
        for s in p["sats"]:
            if s is None or s["azel"] is None:
                continue
            assert abs(s["azel"][1]) >= gs.EL_MARGIN, (sc["name"], s["azel"])
            worst["el"] = min(worst["el"], abs(s["azel"][1]))
            if s["terms"] is not None:
                dx = abs(abs(s["terms"]["x"]) - 1.57)
                assert dx >= gs.X_MARGIN, (sc["name"], s["terms"]["x"])
                worst["x"] = min(worst["x"], dx)
                if "phi_clamp" in sc["name"]:
                    dp = abs(abs(s["terms"]["phi_raw"]) - 0.416)
                    assert dp >= gs.PHI_MARGIN, (sc["name"], s["terms"]["phi_raw"])
                    worst["phi"] = min(worst["phi"], dp)
    print("margins: height %.3f m, elevation %.2f deg, |x| %.3g, phi %.3g" % (worst["h"], math.degrees(worst["el"]), worst["x"], worst["phi"]))


def test_oracle_matches_transcription_on_every_scenario(orc):
    """tolerances of test_gnss_front.py::test_oracle_matches_numpy_transcription"""
    worst = {f[0]: 0.0 for f in FIELDS}
    for sc, o in zip(gs.scenarios(), oracle_results(orc)):
        t = gg.residuals(sc["eph"], sc["obs"], sc["ion"], sc["doy"], sc["xyzt"], sc["velt"])
        assert np.array_equal(o["usable"], t["usable"]), sc["name"]
        for name, _, key, sl, tol, _ in FIELDS:
            d = float(np.abs(_col(o, key, sl) - _col(t, key, sl)).max())
            worst[name] = max(worst[name], d)
            assert d < tol, (sc["name"], name, d)
    print("oracle vs transcription, worst over the sweep:", {k: "%.2g" % v for k, v in worst.items()})


# ---- CPU: the ragged batch of the row tests and its reference chain, from the oracle alone -------------------------------------------------
NB = 6
IDX_CB_OFF = {4: (1, 2)}                                                     # filter 4: GLONASS and Galileo clocks not in the state


def _renu():
    lat, lon = np.deg2rad(gs.BATCH_LAT), np.deg2rad(gs.BATCH_LON)
    return np.array([[-np.sin(lon), -np.sin(lat) * np.cos(lon), np.cos(lat) * np.cos(lon)],
                     [np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat) * np.sin(lon)], [0.0, np.cos(lat), np.sin(lat)]])


def _rot_z(yaw):
    return np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])


def receiver_epoch(raw, p_w, v_w, yaw, idx_se23, idx_yof, idx_fs, idx_cb, cb=None):
    """a raw epoch of gs.update_batch as ingvio_gnss_front_stage takes it: the anchor maps the filter's position onto the epoch's
    evaluation point"""
    Rw = _renu() @ _rot_z(yaw)
    return dict(eph=raw["eph"], obs=raw["obs"], ion=raw["ion"], doy=raw["doy"], p_w=p_w, v_w=v_w, cb=raw["xyzt"][3:] if cb is None else cb, fs=float(raw["velt"][3]),
                yaw_offset=yaw, R_enu2ecef=_renu(), anchor_ecef=raw["xyzt"][:3] - Rw @ p_w, idx_se23=idx_se23, idx_yof=idx_yof, idx_fs=idx_fs,
                idx_cb=list(idx_cb), psr_amp=1.0, dopp_amp=1.0)


def reference_update(orc, P, e, table):
    """GnssUpdate::updateTrackedSys on the oracle alone for prior P and receiver epoch e: residuals -> candidate rows -> per-row gates
    (gnss_chi2_test) -> block gate (strong reject, GnssUpdate.cpp:286) -> ekfUpdate.
    -> dict(front, cand (H, res, noise, colmap: every candidate row, over var_order = SE23, YOF, clocks by first appearance, FS), n_cand,
    keep [n_cand], gamma [n_cand], rows, status (0 / 3 = rejected), block (gamma, threshold) or None, dx, P)"""
    Rw = np.asarray(e["R_enu2ecef"]) @ _rot_z(e["yaw_offset"])
    xyzt = np.r_[Rw @ e["p_w"] + e["anchor_ecef"], e["cb"]]
    velt = np.r_[Rw @ e["v_w"], e["fs"]]
    o = orc.gnss_residuals(e["eph"], e["obs"], e["ion"], e["doy"], xyzt, velt)
    u = o["usable"] == 1
    g = dict(los=o["los"][u], sys=e["eph"][u, 0].astype(int), res_pos=o["res_pos"][u], res_vel=o["res_vel"][u], sin_el=np.sin(o["azel"][u, 1]),
             ura=e["eph"][u, 24], psr_std=e["obs"][u, 3], dopp_std_mps=e["obs"][u, 4] * C_LIGHT / e["obs"][u, 5], R_w2ecef=Rw, p_w=e["p_w"],
             v_w=e["v_w"], idx_se23=e["idx_se23"], idx_yof=e["idx_yof"], idx_cb=e["idx_cb"], idx_fs=e["idx_fs"], chi2_table=table)
    oc = orc.Cov(P, ld=256)
    Hc, rc, Rc, vi, vs = orc.gnss_rows(oc, dict(g, chi2_test=0))               # every candidate row: pseudo-ranges in order, then Dopplers
    n_cand, half = len(rc), len(rc) // 2
    off = np.cumsum(np.r_[0, vs])
    col = {int(i): int(off[k]) for k, i in enumerate(vi)}                     # first column of a variable in the stacked rows
    gamma = np.zeros(n_cand)
    for r in range(n_cand):                                                  # the row alone on the prior, over [SE23, YOF, its clock or FS]
        own = [i for i in vi[2:] if Hc[r, col[int(i)]] != 0.0]
        assert len(own) == 1 and (own[0] == e["idx_fs"]) == (r >= half)
        Hi = np.r_[Hc[r, :9], 0.0, 1.0][None]
        gamma[r] = oc.whiten([e["idx_se23"], e["idx_yof"], own[0]], [9, 1, 1], Hi, rc[r:r + 1], np.float64(Rc[r]))
    keep = (gamma < table[1]).astype(np.int32)
    Ho, ro, Ro, vio, vso = orc.gnss_rows(oc, dict(g, chi2_test=1))             # the reference's own gating and stacking
    assert len(ro) == keep.sum() and np.array_equal(ro, rc[keep == 1]) and np.array_equal(Ro, Rc[keep == 1])
    cand = dict(H=Hc, res=rc, noise=Rc, colmap=np.concatenate([np.arange(i, i + k) for i, k in zip(vi, vs)]) if n_cand else np.zeros(0, dtype=int))
    out = dict(front=o, cand=cand, n_cand=n_cand, keep=keep, gamma=gamma, rows=len(ro), status=0, block=None, dx=np.zeros(P.shape[0]), P=P.copy())
    if len(ro) == 0:
        return out
    if len(ro) <= 14:
        out["block"] = (oc.whiten(vio, vso, Ho, ro, Ro), table[len(ro)])
        if not out["block"][0] < out["block"][1]:
            out["status"] = 3
            return out
    dx, rc_ = oc.ekf_update(vio, vso, Ho, ro, Ro)
    assert rc_ == 0
    out["dx"], out["P"] = dx, oc.P
    return out


def batch_case(orc):
    """six filters built on the oracle's covariance algebra (priors, indices, poses), their epochs, and the reference chain; once"""
    if "batch" in _memo:
        return _memo["batch"]
    from ingvio_amd import synth
    flts = []
    for b in range(NB):
        n_gnss = 0 if b == 2 else (3 if b % 2 else 6)                        # filter 2 has no GNSS scalars at all (and no epoch)
        flt = synth.Filter(lambda P: orc.Cov(P, ld=256), orc.imu_transition, t0=0.3 * b, n_gnss=n_gnss, n_landmarks=2)
        rngb = np.random.default_rng(b)
        for _ in range(3):
            flt.propagate_cov(flt.imu_steps(rngb)); flt.clone()
        flts.append(flt)
    yaws = [0.3 + 0.01 * b for b in range(NB)]
    raws = gs.update_batch([_renu() @ _rot_z(yaws[b]) @ flts[b].v for b in range(NB)])
    table = synth.chi2_table()
    eps, refs = [], []
    for b, (flt, raw) in enumerate(zip(flts, raws)):
        if raw is None:
            eps.append(None); refs.append(None)
            continue
        idx_cb = [(-1 if s in IDX_CB_OFF.get(b, ()) else flt.gnss_idx[s]) for s in range(4)]
        e = receiver_epoch(raw, flt.p.copy(), flt.v.copy(), yaws[b], 0, flt.idx_yof, flt.gnss_idx[4], idx_cb)
        eps.append(e); refs.append(reference_update(orc, flt.cov.P, e, table))
    _memo["batch"] = dict(flts=flts, priors=[f.cov.P for f in flts], eps=eps, refs=refs, table=table)
    return _memo["batch"]


def test_row_batch_reference_chain_is_decisive(orc):
    """Before anything runs on a GPU: no chi^2 statistic of the batch lies within 1 % of its threshold (device and oracle must take the
    same decisions), the batch is what it claims to be, and the oracle's own chain accepts: every filter keeps more than half of its
    ordinary rows, so the GPU test cannot pass with everything gated away."""
    c = batch_case(orc)
    table = c["table"]
    assert [0 if e is None else len(e["eph"]) for e in c["eps"]] == [1, 12, 0, 64, 7, 12]
    assert [int(s) for s in c["eps"][1]["eph"][:6, 0]] == [3, 0, 3, 1, 2, 0]    # BDS, GPS, BDS, GLO, GAL, GPS, ...
    assert c["priors"][2].shape[0] + 6 == c["priors"][0].shape[0]               # filter 2 carries no GNSS scalars
    for b, (e, r) in enumerate(zip(c["eps"], c["refs"])):
        if e is None:
            continue
        assert np.abs(r["gamma"] / table[1] - 1.0).min() > 0.01, (b, r["gamma"])
        if r["block"] is not None:
            assert abs(r["block"][0] / r["block"][1] - 1.0) > 0.01, (b, r["block"])
        sysu = e["eph"][r["front"]["usable"] == 1, 0].astype(int)
        in_state = np.array([e["idx_cb"][s] >= 0 for s in sysu])
        assert r["n_cand"] == 2 * in_state.sum()
        cand_sys = np.r_[sysu[in_state], sysu[in_state]]
        gross = cand_sys == 1 if b == 3 else np.zeros(r["n_cand"], dtype=bool)
        assert not r["keep"][gross].any()                                   # filter 3: no GLONASS row passes, its clock column stays empty
        assert r["keep"][~gross].sum() > 0.5 * (~gross).sum(), (b, r["keep"])
        assert r["status"] == 0 and r["dx"].any(), b
        print("filter %d: n_sat %2d candidates %3d kept %3d  min |gamma/thr - 1| %.3f" % (b, len(e["eph"]), r["n_cand"], r["rows"],
                                                                                         np.abs(r["gamma"] / table[1] - 1.0).min()))
    for b in (1, 4):                                                        # first appearance is not the order of the systems there
        clocks = list(c["refs"][b]["cand"]["colmap"][10:-1])
        assert sorted(clocks) == sorted(i for i in c["eps"][b]["idx_cb"] if i >= 0) and clocks != [i for i in c["eps"][b]["idx_cb"] if i >= 0], b
    assert c["refs"][3]["n_cand"] == 128 and c["refs"][3]["rows"] > 14        # the widest batch the row buffers take; past the block gate
    r4, e4 = c["refs"][4], c["eps"][4]
    assert (r4["front"]["usable"] == 1).all() and r4["n_cand"] == 2 * int(np.isin(e4["eph"][:, 0], (0, 3)).sum()) == 8
    assert c["refs"][5]["front"]["usable"][5] == 0 and c["refs"][5]["n_cand"] == 22


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _compare_front(rec, o, ns, what, worst):
    """one epoch's records [64, 20] against the oracle's result for its ns satellites; lanes from ns on hold the idle record"""
    assert np.array_equal(rec[:ns, 9].astype(int), o["usable"]) and set(rec[:, 9]) <= {0.0, 1.0}, what
    for name, cols, key, sl, _, tol in FIELDS:
        d = float(np.abs(rec[:ns, cols] - _col(o, key, sl)).max()) if ns else 0.0
        worst[name] = max(worst.get(name, 0.0), d)
        assert d < tol, (what, name, d)
    assert np.array_equal(rec[ns:], np.tile(IDLE, (64 - ns, 1))), what
    skipped = rec[:ns][o["usable"] == 0]                                    # an unusable entry inside the epoch: the same idle record
    assert np.array_equal(skipped, np.tile(IDLE, (len(skipped), 1))), what


@pytest.mark.gpu
def test_gpu_sat_records_match_the_oracle_on_every_scenario(orc):
    """All scenarios through ingvio_gnss_sat_eval in ONE launch (n_sat ragged, 1 .. 64); all 20 fields of every record against
    orc.gnss_residuals, at the tolerances of test_gnss_front_kernel_vs_oracle_and_through_the_update (residuals, line of sight, angles,
    delays) and test_sat_eval_matches_oracle (satellite state)."""
    from ingvio_amd import capi
    S = gs.scenarios()
    ctx = capi.Context(batch=1, n_max=64, c_max=4, f_max=8, m_max=16)
    out = ctx.gnss_sat_eval([gs.sat_eval_epoch(sc) for sc in S])
    ctx.close()
    worst = {}
    for sc, o, rec in zip(S, oracle_results(orc), out):
        w = {}
        _compare_front(rec, o, len(sc["eph"]), sc["name"], w)
        for k, v in w.items():
            worst[k] = max(worst.get(k, (0.0, ""))[0], v), (sc["name"] if v >= worst.get(k, (0.0, ""))[0] else worst[k][1])
    for k, (v, where) in worst.items():
        print("kernel vs oracle, worst %-9s %.3g  (%s)" % (k, v, where))


def _check_update(ctx, c, order, fr, staged, res, P1, what):
    """device results of the staged batch (filters `order` of the case, in this order) against the reference chain.
    staged: ingvio_debug_gnss_staged_rows per filter.  Its bounds follow from the record's: H holds -u^T R and u^T R [p]x, u^T R [v]x with
    u good to 1e-12, hence 4e-12 max(1, |p|, |v|); the row variance goes with 1 / sin^2(el), el good to 1e-11 and >= 15 degrees: 1e-9
    relative; the column map is exact."""
    dx, rows, keep, gam, st = res
    for i, b in enumerate(order):
        e, r, prior = c["eps"][b], c["refs"][b], c["priors"][b]
        n = prior.shape[0]
        if e is None:                                                       # no satellite: bit-identical to the prior, nothing moved
            assert rows[i] == 0 and st[i] == 0 and not keep[i].any() and not dx[i].any() and np.array_equal(P1[i], prior), (what, b)
            assert np.array_equal(fr[i], np.tile(IDLE, (64, 1))) and staged[i][0].shape[0] == 0, (what, b)
            continue
        _compare_front(fr[i], r["front"], len(e["eph"]), (what, b), {})
        Hs, rs, ns_, cm = staged[i]
        cand = r["cand"]
        assert Hs.shape == cand["H"].shape and np.array_equal(cm, cand["colmap"]), (what, b, cm, cand["colmap"])
        half = r["n_cand"] // 2
        assert np.abs(Hs - cand["H"]).max() < 4e-12 * max(1.0, np.linalg.norm(e["p_w"]), np.linalg.norm(e["v_w"])), (what, b)
        assert np.abs(rs[:half] - cand["res"][:half]).max() < 1e-6 and np.abs(rs[half:] - cand["res"][half:]).max() < 1e-9, (what, b)
        assert np.allclose(ns_, cand["noise"], rtol=1e-9, atol=0.0), (what, b)
        assert rows[i] == r["rows"], (what, b, rows[i], r["rows"])
        assert np.array_equal(keep[i, :r["n_cand"]], r["keep"]) and not keep[i, r["n_cand"]:].any(), (what, b)
        assert st[i] == r["status"], (what, b, st[i])
        assert rel_err(P1[i], r["P"]) < 1e-11, (what, b, rel_err(P1[i], r["P"]))
        assert rel_err(dx[i, :n], r["dx"]) < 1e-7, (what, b, rel_err(dx[i, :n], r["dx"]))
        print("%s filter %d: rows %3d/%3d  posterior %.1e  dx %.1e" % (what, b, rows[i], r["n_cand"], rel_err(P1[i], r["P"]), rel_err(dx[i, :n], r["dx"])))


@pytest.mark.gpu
def test_gpu_ragged_batch_rows_through_the_update(orc):
    """gnss_front_stage -> gnss_run -> gnss_fetch on a ragged batch (n_sat 1, 12, 0, 64, 7, 12; clocks missing from the state, interleaved
    constellations, a constellation whose rows are all gated away), per-row gates and strong reject on, against the oracle's chain."""
    from ingvio_amd import capi
    from ingvio_amd.closed_loop_gnss import NO_EPOCH
    c = batch_case(orc)
    ctx = capi.Context(batch=NB + 1, n_max=256, c_max=11, f_max=8, m_max=128)
    for b in range(NB):
        ctx.cov_set(b, c["priors"][b])
    ctx.cov_set(NB, c["priors"][0] * 1.5)                                    # a neighbour outside the staged range
    ctx.gnss_front_stage(0, [NO_EPOCH if e is None else e for e in c["eps"]], c["table"], gate_rows=True, strong_reject=True)
    fr = ctx.gnss_front_fetch()
    staged = [ctx.debug_gnss_staged_rows(b) for b in range(NB)]
    ctx.gnss_run()
    res = ctx.gnss_fetch()
    P1 = [ctx.cov_get(b) for b in range(NB + 1)]
    _check_update(ctx, c, list(range(NB)), fr, staged, res, P1, "host-fed")
    assert np.array_equal(P1[NB], c["priors"][0] * 1.5)
    ctx.close()


@pytest.mark.gpu
def test_gpu_ragged_batch_from_the_nominal_table(orc):
    """Three epochs of the batch (12 interleaved, 64 with the gated constellation, 7) through ingvio_gnss_front_stage_nominal: receiver
    state and indices come from the device table.  Filter 2's table leaves the Galileo and BeiDou clocks unregistered: their bias is the
    receiver record's (zero), their satellites are usable and give no rows.  Records, decisions and posterior against the oracle's chain
    at the same tolerances; no bit-identity between the two instantiations is asked for."""
    from ingvio_amd import capi, synth
    from ingvio_amd.closed_loop import make_loop
    from ingvio_amd.closed_loop_gnss import gnss_slots
    cases = make_loop(3, 1)
    table = synth.chi2_table()
    yaws = [0.25, 0.31, 0.37]
    pose = [c["table"].slots[c["table"].v_pose] for c in cases]
    raws = gs.update_batch([None, _renu() @ _rot_z(yaws[0]) @ pose[0]["v"], None, _renu() @ _rot_z(yaws[1]) @ pose[1]["v"],
                            _renu() @ _rot_z(yaws[2]) @ pose[2]["v"], None], only=(1, 3, 4))
    eps, refs, slots = [], [], []
    for i, (c, raw) in enumerate(zip(cases, raws)):
        sl = gnss_slots(c)
        if i == 2:
            sl[2] = sl[3] = -1
        t = c["table"]
        cb = np.array([raw["xyzt"][3 + s] if sl[s] >= 0 else 0.0 for s in range(4)])
        for s in range(4):
            if sl[s] >= 0:
                t.slots[sl[s]]["p"] = np.array([cb[s], 0.0, 0.0])
        t.slots[sl[4]]["p"] = np.array([float(raw["velt"][3]), 0.0, 0.0])
        t.slots[sl[5]]["p"] = np.array([yaws[i], 0.0, 0.0])
        idx = lambda v: t.slots[v]["idx"] if v >= 0 else -1
        e = receiver_epoch(raw, pose[i]["p"], pose[i]["v"], yaws[i], idx(t.v_pose), idx(sl[5]), idx(sl[4]), [idx(v) for v in sl[:4]], cb=cb)
        eps.append(e); refs.append(reference_update(orc, c["P"], e, table)); slots.append(sl)
    r2, e2 = refs[2], eps[2]
    assert (r2["front"]["usable"] == 1).all() and r2["n_cand"] == 2 * int(np.isin(e2["eph"][:, 0], (0, 1)).sum()) > 0
    for r in refs:                                                          # decisive on the CPU first, as for the host-fed batch
        assert np.abs(r["gamma"] / table[1] - 1.0).min() > 0.01 and (r["block"] is None or abs(r["block"][0] / r["block"][1] - 1.0) > 0.01)
        assert r["status"] == 0 and r["rows"] > 0.5 * r["n_cand"]
    n_max = max(c["P"].shape[0] for c in cases) + 6
    ctx = capi.Context(batch=3, n_max=((n_max + 15) // 16) * 16, c_max=12, f_max=24, m_max=128)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c["P"])
    ctx.nominal_create(48)
    ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    ctx.nominal_set_gnss(0, slots)
    host_only = ("eph", "obs", "ion", "doy", "R_enu2ecef", "anchor_ecef", "psr_amp", "dopp_amp")
    ctx.gnss_front_stage_nominal(0, [{k: e[k] for k in host_only} for e in eps], table, gate_rows=True, strong_reject=True)
    fr = ctx.gnss_front_fetch()
    staged = [ctx.debug_gnss_staged_rows(b) for b in range(3)]
    ctx.gnss_run()
    res = ctx.gnss_fetch()
    P1 = [ctx.cov_get(b) for b in range(3)]
    _check_update(ctx, dict(eps=eps, refs=refs, priors=[c["P"] for c in cases]), [0, 1, 2], fr, staged, res, P1, "table")
    ctx.close()
