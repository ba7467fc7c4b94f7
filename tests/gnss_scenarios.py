"""Deterministic GNSS epochs for the front kernel's sweep (tests/test_gnss_front_scenarios.py): every branch of the geodesy of
kernels_gnss.hip that the one recorded instant of tests/golden/gnss_front.npz never takes - hemispheres and latitude bands of the Niell
mapping, the height cut-offs of both delay models, the Klobuchar clamps and its day/night switch, the week wrap, the step counts of
the GLONASS integration, the BeiDou GEO frame by PRN, eccentric orbits, satellites below the horizon, a receiver on the polar axis and
at the origin, unusable entries, 1 and 64 satellites.  Built from seeds with the builders of the numpy transcription
(oracle/gen_gnss_golden.py); observations come from make_obs, so residuals stay at metre scale.  No GPU, no import side effects.

A scenario is a dict: name, eph [ns, 25], obs [ns, 6], ion ([8] or None), doy, the true receiver (rcv_true, vel_true, cb_true, fs_true),
the evaluation state xyzt [7] / velt [4], branch (a predicate over probe(scenario): the branch the scenario exists for) and on_clamp
(the evaluation height sits on the continuous `hgt < 0 -> 0` clamp on purpose).  The evaluation point is the scenario's nominal site
exactly - the latitude band edges and the height margins are properties of the point the kernel evaluates - and the true receiver
lies a few metres beside it."""
import math

import numpy as np

from oracle import gen_gnss_golden as gg

WEEK = gg.WEEK
T_RX, DOY = 360300.0, 270.4
ION = np.array([0.1118e-07, 0.2235e-07, -0.1192e-06, -0.1192e-06, 0.1167e+06, 0.1802e+06, -0.1311e+06, -0.4588e+06])
VEL, CB, FS = np.array([1.2, -0.7, 0.3]), np.array([150.0, 140.0, 165.0, 180.0]), 5.0
D_CB, D_VEL, D_FS = np.array([2.0, -1.5, -1.0, 1.5]), np.array([0.05, -0.02, 0.01]), 0.1
WANT = (("gps", 0, 4), ("bds", 3, 2), ("gal", 2, 2))
HGT = 120.0                                                     # default site height: clear of every height cut-off by more than 50 m
HEIGHT_CUTS = (-1000.0, -100.0, 0.0, 10000.0)
H_MARGIN, EL_MARGIN, X_MARGIN, PHI_MARGIN = 50.0, math.radians(1.0), 1e-3, 1e-3
GLO_TARGETS = (0.0, 60.0, -60.0, 120.0 + 1e-7, 899.0, -899.0)  # t_tx - toe of the step-count scenario
GLO_STEPS = (0, 1, 1, 3, 15, 15)                               # Runge-Kutta steps they take: none, one, 2 + remainder, 14 + remainder


# ---- what a scenario is checked on: the transcription's own functions, satellite by satellite ---------------------------------------
def iono_terms(tow, ion, lla, azel):
    """the intermediate values of gg.iono (same expressions): phi before its clamp, amp and per before theirs, x"""
    psi = 0.0137 / (azel[1] / math.pi + 0.11) - 0.022
    phi_raw = lla[0] / 180.0 + psi * math.cos(azel[0])
    phi = min(max(phi_raw, -0.416), 0.416)
    lam = lla[1] / 180.0 + psi * math.sin(azel[0]) / math.cos(phi * math.pi)
    phi += 0.064 * math.cos((lam - 1.617) * math.pi)
    tt = 43200.0 * lam + tow
    tt -= math.floor(tt / 86400.0) * 86400.0
    amp_raw = ion[0] + phi * (ion[1] + phi * (ion[2] + phi * ion[3]))
    per_raw = ion[4] + phi * (ion[5] + phi * (ion[6] + phi * ion[7]))
    amp, per = max(amp_raw, 0.0), max(per_raw, 72000.0)
    x = 2.0 * math.pi * (tt - 50400.0) / per
    f = 1.0 + 16.0 * (0.53 - azel[1] / math.pi) ** 3
    return dict(phi_raw=phi_raw, amp_raw=amp_raw, per_raw=per_raw, x=x,
                delay=gg.C_LIGHT * f * (5E-9 + amp * (1.0 + x * x * (-0.5 + x * x / 24.0)) if abs(x) < 1.57 else 5E-9))


def glo_steps(ttx, ep):
    """the steps gg.geph2posvel hands to gg.glo_orbit for transmit time ttx"""
    calls, orig = [], gg.glo_orbit
    gg.glo_orbit = lambda tt, x, acc: (calls.append(tt), orig(tt, x, acc))[1]
    try:
        gg.geph2posvel(ttx, ep)
    finally:
        gg.glo_orbit = orig
    return calls


def probe(sc):
    """-> dict(lla, rn, sats): per satellite None (unusable) or dict(sys, prn, e, ttx, raw = t - toe before the wrap, tk, steps (GLONASS),
    azel, trop, iono, terms (iono_terms; None without a sky or parameters))"""
    xyz = sc["xyzt"][:3]
    lla, rn = gg.ecef2geo(xyz), float(np.linalg.norm(xyz))
    sats = []
    for ep, ob in zip(sc["eph"], sc["obs"]):
        st = gg.sat_state(ep, ob)
        if st is None:
            sats.append(None)
            continue
        pos, ttx = st[0], st[5]
        s = dict(sys=int(ep[gg.SYS]), prn=int(ep[gg.PRN]), e=float(ep[gg.E]), ttx=ttx, raw=ttx - ep[gg.TOE], tk=gg.wrap(ttx - ep[gg.TOE]),
                 steps=glo_steps(ttx, ep) if int(ep[gg.SYS]) == 1 else None, azel=None, trop=0.0, iono=0.0, terms=None)
        if rn > 0:
            s["azel"] = gg.sat_azel(xyz, pos)
            s["trop"] = gg.trop(sc["doy"], lla, s["azel"])
            if sc["ion"] is not None:
                s["iono"] = gg.iono(ttx, sc["ion"], lla, s["azel"])
                if s["azel"][1] > 0 and lla[2] >= -1E3:
                    s["terms"] = iono_terms(ttx, sc["ion"], lla, s["azel"])
        sats.append(s)
    return dict(lla=lla, rn=rn, sats=sats)


def _up(p):
    """the usable satellites above the horizon"""
    return [s for s in p["sats"] if s is not None and s["azel"] is not None and s["azel"][1] > 0]


# ---- builders --------------------------------------------------------------------------------------------------------------------------
def _el(rcv, ep, t_rx):
    pos = gg.geph2posvel(t_rx - 0.075, ep)[0] if int(ep[gg.SYS]) == 1 else gg.eph2pos(t_rx - 0.075, ep)[0]
    return math.degrees(gg.sat_azel(rcv, pos)[1])


def _draw(rng, rcv, t_rx, name, sysid, edit, ok):
    """one satellite of make_constellation, edited, redrawn until ok(ep)"""
    for _ in range(4000):
        ep = gg.make_constellation(rng, rcv, t_rx, ((name, sysid, 1),))[0]
        edit(ep)
        if ok(ep):
            return ep
    raise RuntimeError("no satellite found: " + name)


def _number(eph):
    """PRNs in order of appearance per constellation (BeiDou from 7: MEO; scenarios about the GEO frame set theirs afterwards)"""
    cnt = {}
    for ep in eph:
        s = int(ep[gg.SYS])
        cnt[s] = cnt.get(s, 0) + 1
        ep[gg.PRN] = cnt[s] + (6 if s == 3 else 0)
    return eph


def _sky(rng, rcv, t_rx, want=WANT, n_glo=1):
    eph = gg.make_constellation(rng, rcv, t_rx, want)
    if n_glo:
        eph = np.vstack([eph, gg.make_glonass(rng, rcv, t_rx, n_glo)])
    return _number(eph)


def _rereference(ep, d):
    """the same Kepler orbit and clock polynomial (af2 = 0) referred to toe + d"""
    mu = gg.MU_GPS if int(ep[gg.SYS]) == 0 else gg.MU
    n = math.sqrt(mu / ep[gg.A] ** 3) + ep[gg.DELTA_N]
    ep[gg.M0] += n * d; ep[gg.OMG0] += ep[gg.OMG_DOT] * d; ep[gg.I0] += ep[gg.I_DOT] * d; ep[gg.AF0] += ep[gg.AF1] * d
    ep[gg.TOE] += d; ep[gg.TOC] += d; ep[gg.TOE_SYS] += d


def _site(lat, lon, hgt):
    """-> (evaluation point = the site itself, true receiver a few metres beside and 1.5 m above it)"""
    return gg.geo2ecef(np.array([lat, lon, hgt])), gg.geo2ecef(np.array([lat - 2e-5, lon + 3e-5, hgt + 1.5]))


def _scenario(name, rng, eph, xyz, rcv, branch, t_rx=T_RX, doy=DOY, ion=ION, on_clamp=False, obs_rows=None, edit=None, vel=VEL):
    obs = gg.make_obs(rng, eph, rcv, vel, CB, FS, ion if ion is not None else np.zeros(8), doy, t_rx)
    for i, ob in (obs_rows or {}).items():
        obs[i] = ob
    if edit is not None:
        edit(eph, obs)
    return dict(name=name, eph=eph, obs=obs, ion=ion, doy=doy, rcv_true=rcv, vel_true=vel, cb_true=CB, fs_true=FS,
                xyzt=np.r_[xyz, CB + D_CB], velt=np.r_[vel + D_VEL, FS + D_FS], branch=branch, on_clamp=on_clamp)


def _at_site(name, seed, lat, lon, hgt, branch, t_rx=T_RX, doy=DOY, ion=ION, want=WANT, n_glo=1, on_clamp=False, edit=None):
    rng = np.random.default_rng(seed)
    xyz, rcv = _site(lat, lon, hgt)
    return _scenario(name, rng, _sky(rng, rcv, t_rx, want, n_glo), xyz, rcv, branch, t_rx, doy, ion, on_clamp, edit=edit)


def _glonass_at(rng, rcv, t_rx, target, prn, seed):
    """a GLONASS record and its observation with t_tx - toe = target: the record is the SAME orbit re-expressed at the new toe (integrated
    there with the transcription), toe found by fixed-point iteration on the transmit time the observation implies (the pseudo-range
    moves by micrometres when toe moves by a microsecond: it contracts at once)"""
    base = gg.make_glonass(rng, rcv, t_rx, 1)[0]
    toe, ep, ob = t_rx - 0.08 - target, None, None
    for _ in range(12):
        ep = base.copy()
        ep[gg.PRN], ep[gg.TOE] = prn, toe
        p, v, _, _ = gg.geph2posvel(toe, base)
        ep[gg.GLO_POS:gg.GLO_POS + 3], ep[gg.GLO_VEL:gg.GLO_VEL + 3] = p, v
        ob = gg.make_obs(np.random.default_rng(seed), ep[None], rcv, VEL, CB, FS, ION, DOY, t_rx)[0]
        new = gg.sat_state(ep, ob)[5] - target
        if new == toe:
            break
        toe = new
    return ep, ob


def _bds_trio(rng, rcv, t_rx, geo):
    """one set of BeiDou elements (GEO-like or MEO-like) under PRN 3, 5 and 6: two take the GEO frame, one does not; all three in view"""
    def edit(ep):
        if geo:
            ep[gg.A], ep[gg.E], ep[gg.I0] = 42164e3, 3e-4, 0.08

    def ok(ep):
        for prn in (3, 5, 6):
            ep[gg.PRN] = prn
            if _el(rcv, ep, t_rx) < 8.0:
                return False
        return True
    ep = _draw(rng, rcv, t_rx, "bds", 3, edit, ok)
    out = np.repeat(ep[None], 3, axis=0)
    out[:, gg.PRN] = (3, 5, 6)
    return out


# ---- branch predicates -------------------------------------------------------------------------------------------------------------------
def _lat_band(lo, hi, south=False):
    """every satellite in view has a troposphere delay; |latitude| / 15 truncates into [lo, hi]; the hemisphere is the stated one"""
    return lambda p: (lo <= int(abs(p["lla"][0]) / 15.0) <= hi and (p["lla"][0] < 0) == south and len(_up(p)) >= 4 and all(s["trop"] > 0 for s in _up(p)))


def _wraps(sign):
    """t - toe of every Kepler satellite and of a GLONASS one lies beyond half a week with the stated sign, tk has the other sign"""
    def f(p):
        sats = [s for s in p["sats"] if s is not None]
        kep = [s for s in sats if s["sys"] != 1]
        glo = [s for s in sats if s["sys"] == 1]
        w = lambda s: abs(s["raw"]) > WEEK / 2 and s["raw"] * sign > 0 and s["tk"] * sign < 0 and abs(s["tk"]) < 7200.0
        return len(kep) >= 6 and all(w(s) for s in kep) and any(w(s) for s in glo)
    return f


def build():
    """the list of scenarios (42 epochs, n_sat 1 .. 64), in a fixed order"""
    S = []
    # -- site: hemisphere and latitude band of the Niell coefficients; longitudes around the globe and at the date line
    for k, (lat, lon) in enumerate(((-80.0, -179.95), (-45.0, 170.3), (-10.0, -75.2), (5.0, 12.6), (14.99, 179.97), (15.0, -120.0),
                                    (45.0, 60.1), (74.99, -179.9), (75.0, 121.4), (82.0, -30.7))):
        i = int(abs(lat) / 15.0)
        lo = i - 1 if lat % 15.0 == 0.0 else i                   # on a band edge the geodetic round trip may land on either side: continuous
        S.append(_at_site("site_lat%+06.2f" % lat, 100 + k, lat, lon, HGT, _lat_band(lo, i, lat < 0)))
    # -- height: the cut-offs of the two delay models, seen from the evaluation point
    zero_t = lambda p: len(_up(p)) >= 4 and all(s["trop"] == 0.0 for s in _up(p))
    some_t = lambda p: len(_up(p)) >= 4 and all(s["trop"] > 0.0 for s in _up(p))
    zero_i = lambda p: all(s["iono"] == 0.0 for s in _up(p))
    some_i = lambda p: all(s["iono"] > 0.0 for s in _up(p))
    S.append(_at_site("height_-1100", 120, 31.0, 121.4, -1100.0, lambda p: zero_t(p) and zero_i(p) and p["lla"][2] < -1E3))
    S.append(_at_site("height_-150", 121, 31.0, 121.4, -150.0, lambda p: zero_t(p) and some_i(p) and -1E3 < p["lla"][2] < -100.0))
    S.append(_at_site("height_-50", 122, 31.0, 121.4, -50.0, lambda p: some_t(p) and some_i(p) and -100.0 < p["lla"][2] < 0.0))      # hgt clamped, dm negative
    S.append(_at_site("height_0", 123, 31.0, 121.4, 0.0, lambda p: some_t(p) and abs(p["lla"][2]) < 1e-6, on_clamp=True))
    S.append(_at_site("height_9900", 124, 31.0, 121.4, 9900.0, lambda p: some_t(p) and 9000.0 < p["lla"][2] < 1E4))
    S.append(_at_site("height_10100", 125, 31.0, 121.4, 10100.0, lambda p: zero_t(p) and some_i(p) and p["lla"][2] > 1E4))
    # -- time: both branches of the week wrap, the middle of the week, the phase of the seasonal term in both hemispheres
    def wrap_toe(eph, obs):
        for ep in eph:
            ep[gg.TOE] = ep[gg.TOE] % WEEK
            if int(ep[gg.SYS]) != 1:
                ep[gg.TOC] = ep[gg.TOC] % WEEK
    S.append(_at_site("time_tow100", 130, 31.0, 121.4, HGT, _wraps(-1), t_rx=100.0, n_glo=2, edit=wrap_toe))
    rng = np.random.default_rng(131)
    xyz, rcv = _site(-33.0, 151.2, HGT)
    eph = _sky(rng, rcv, 604700.0, n_glo=2)
    for ep in eph[:-2]:
        _rereference(ep, 3600.0)                                  # toe from half an hour before to half an hour after the epoch: next week
    sc = _scenario("time_tow604700", rng, eph, xyz, rcv, _wraps(+1), t_rx=604700.0)
    wrap_toe(sc["eph"], sc["obs"])
    S.append(sc)
    no_wrap = lambda p: all(abs(s["raw"]) < 7200.0 for s in p["sats"] if s is not None) and len(_up(p)) >= 6
    S.append(_at_site("time_tow302300", 132, 31.0, 121.4, HGT, no_wrap, t_rx=302300.0))
    for k, (doy, lat, lon) in enumerate(((28.0, -33.0, 18.4), (210.0, 52.0, 13.4), (365.9, -62.0, -45.0))):
        i = int(abs(lat) / 15.0)
        S.append(_at_site("time_doy%g" % doy, 133 + k, lat, lon, HGT, _lat_band(i, i, lat < 0), doy=doy))
    # -- orbits: eccentric Galileo, the BeiDou GEO frame by PRN, the step counts of the GLONASS integration
    rng = np.random.default_rng(140)
    xyz, rcv = _site(48.1, 11.6, HGT)
    eph = [_draw(rng, rcv, T_RX, "gal", 2, lambda ep, e=e: ep.__setitem__(gg.E, e), lambda ep: _el(rcv, ep, T_RX) > 10.0) for e in (0.05, 0.09, 0.13, 0.17)]
    eph = _number(np.vstack([np.array(eph), gg.make_constellation(rng, rcv, T_RX, (("gps", 0, 2),))]))
    S.append(_scenario("orbit_eccentric", rng, eph, xyz, rcv, lambda p: sorted(round(s["e"], 2) for s in p["sats"] if s["sys"] == 2) == [0.05, 0.09, 0.13, 0.17]
                       and len(_up(p)) == 6))
    for geo in (True, False):
        rng = np.random.default_rng(141 + geo)
        xyz, rcv = _site(22.3, 114.2, HGT)
        eph = np.vstack([_bds_trio(rng, rcv, T_RX, geo), _number(gg.make_constellation(rng, rcv, T_RX, (("gps", 0, 2),)))])

        def trio(p, geo=geo):
            b = [s for s in p["sats"] if s["sys"] == 3]
            return [s["prn"] for s in b] == [3, 5, 6] and len(_up(p)) == 5 and (b[0]["e"] < 1e-3) == geo
        S.append(_scenario("orbit_bds_%s_prn356" % ("geo" if geo else "meo"), rng, eph, xyz, rcv, trio))
    rng = np.random.default_rng(143)
    xyz, rcv = _site(55.7, 37.6, HGT)
    glo = [_glonass_at(rng, rcv, T_RX, tgt, k + 1, 1430 + k) for k, tgt in enumerate(GLO_TARGETS)]
    eph = np.vstack([np.array([g[0] for g in glo]), _number(gg.make_constellation(rng, rcv, T_RX, (("gps", 0, 2),)))])

    def steps(p):
        got = [s["steps"] for s in p["sats"][:6]]
        return ([len(c) for c in got] == list(GLO_STEPS) and all(abs(s["tk"] - t) < 2e-9 for s, t in zip(p["sats"], GLO_TARGETS))
                and 0.5e-7 < got[3][2] < 2e-7 and got[4][0] == 60.0 and got[5][0] == -60.0 and len(_up(p)) == 8)
    S.append(_scenario("orbit_glonass_steps", rng, eph, xyz, rcv, steps, obs_rows={k: g[1] for k, g in enumerate(glo)}))
    # -- ionosphere: no parameters, the clamps of amplitude, period and latitude, day and night
    S.append(_at_site("iono_none", 150, 31.0, 121.4, HGT, lambda p: all(s["iono"] == 0.0 and s["trop"] > 0.0 for s in _up(p)), ion=None))
    neg_amp, short_per = ION.copy(), ION.copy()
    neg_amp[:4] = (-3e-8, 0.0, 0.0, 0.0)
    short_per[4:] = (5e4, 0.0, 0.0, 0.0)
    S.append(_at_site("iono_amp_negative", 151, 31.0, 121.4, HGT, lambda p: all(s["terms"]["amp_raw"] < 0.0 and abs(s["terms"]["x"]) < 1.57 for s in _up(p)), ion=neg_amp))
    S.append(_at_site("iono_per_short", 152, 31.0, 121.4, HGT, lambda p: all(s["terms"]["per_raw"] < 72000.0 and abs(s["terms"]["x"]) < 1.57 for s in _up(p)), ion=short_per))
    S.append(_at_site("iono_day", 153, 31.0, 121.4, HGT, lambda p: all(abs(s["terms"]["x"]) < 1.57 and s["terms"]["amp_raw"] > 0.0 for s in _up(p))))
    S.append(_at_site("iono_night", 154, 31.0, 121.4, HGT, lambda p: all(abs(s["terms"]["x"]) > 1.57 for s in _up(p)), t_rx=T_RX + 43200.0))
    S.append(_at_site("iono_phi_clamp_north", 155, 85.0, 20.0, HGT, lambda p: all(s["terms"]["phi_raw"] > 0.416 for s in _up(p)) and len(_up(p)) >= 6))
    S.append(_at_site("iono_phi_clamp_south", 156, -85.0, -160.0, HGT, lambda p: all(s["terms"]["phi_raw"] < -0.416 for s in _up(p)) and len(_up(p)) >= 6))
    # -- geometry: below the horizon, on the polar axis, at the origin
    rng = np.random.default_rng(160)
    xyz, rcv = _site(31.0, 121.4, HGT)
    eph = _sky(rng, rcv, T_RX)
    below = lambda p: all(s["azel"][1] < 0 and s["trop"] == 0.0 and s["iono"] == 0.0 for s in p["sats"]) and len(p["sats"]) == 9
    S.append(_scenario("geometry_antipode", rng, eph, -xyz, -rcv, below))
    rng = np.random.default_rng(161)
    eph = _number(np.vstack([gg.make_constellation(rng, rcv, T_RX), gg.make_constellation(rng, -rcv, T_RX)]))
    mixed = lambda p: [s["azel"][1] > 0 for s in p["sats"]] == [True] * 8 + [False] * 8 and all((s["trop"] > 0) == (s["azel"][1] > 0) for s in p["sats"])
    S.append(_scenario("geometry_mixed_horizon", rng, eph, xyz, rcv, mixed))
    rng = np.random.default_rng(162)
    pole = np.array([0.0, 0.0, 6356752.3142 + HGT])
    axis = lambda p: p["rn"] > 0 and not p["lla"].any() and len(_up(p)) >= 4       # ecef2geo gives up: lat = lon = hgt = 0, as in the reference
    S.append(_scenario("geometry_polar_axis", rng, _sky(rng, pole, T_RX), pole + np.array([0.0, 0.0, 1.5]), pole, axis, on_clamp=True))
    rng = np.random.default_rng(163)
    near = np.array([3.0, -2.0, 1.5])
    origin = lambda p: p["rn"] == 0.0 and all(s["azel"] is None and s["trop"] == 0.0 and s["iono"] == 0.0 for s in p["sats"])
    S.append(_scenario("geometry_origin", rng, _sky(rng, near, T_RX), np.zeros(3), near, origin, on_clamp=True))
    # -- usability: entries the front must skip, first, in the middle and last
    def unusable(order):
        def edit(eph, obs):
            for i, how in order.items():
                if how == "freq":
                    obs[i, gg.FREQ] = -1.0
                else:
                    eph[i, gg.SYS] = how
        return edit
    for k, order in enumerate(({0: "freq", 4: 4, 8: -1}, {0: 4, 3: "freq", 4: -1, 8: "freq"}, {0: -1, 5: "freq", 8: 4})):
        S.append(_at_site("usable_%d" % k, 170 + k, 31.0, 121.4, HGT, lambda p, order=order: [s is None for s in p["sats"]] == [i in order for i in range(9)],
                          edit=unusable(order)))
    # -- size
    S.append(_at_site("size_1", 180, 31.0, 121.4, HGT, lambda p: len(p["sats"]) == 1 and len(_up(p)) == 1, want=(("gal", 2, 1),), n_glo=0))
    S.append(_at_site("size_64", 181, 31.0, 121.4, HGT, lambda p: len(p["sats"]) == 64 and len(_up(p)) == 64 and p["sats"][63]["sys"] == 1,
                      want=(("gps", 0, 20), ("bds", 3, 18), ("gal", 2, 18)), n_glo=8))
    return S


_CACHE = []


def scenarios():
    """build() once per process; the arrays are shared: read them, do not write"""
    if not _CACHE:
        _CACHE.extend(build())
    return _CACHE


def sat_eval_epoch(sc):
    """the scenario as a free-standing epoch of ingvio_gnss_sat_eval: the receiver given in ECEF (include/ingvio_hip.h)"""
    return dict(eph=sc["eph"], obs=sc["obs"], ion=sc["ion"], doy=sc["doy"], p_w=np.zeros(3), v_w=sc["velt"][:3], cb=sc["xyzt"][3:], fs=float(sc["velt"][3]),
                yaw_offset=0.0, R_enu2ecef=np.eye(3), anchor_ecef=sc["xyzt"][:3])


# ---- the ragged batch of the row tests ----------------------------------------------------------------------------------------------------
BATCH_LAT, BATCH_LON = 31.0, 121.4


def update_batch(vel_ecef, only=None):
    """raw epochs for the staged-row tests, one per filter (None: no satellite): n_sat 1, 12, 0, 64, 7, 12; vel_ecef [6][3]: the ECEF
    velocity each filter will evaluate at (the true receiver moves D_VEL slower); only: the epochs wanted (-> just those, in order).
    1: constellations interleaved (BDS, GPS, BDS, GLO, GAL, GPS, ...), so the clock columns' order of first appearance is not the order
    of the systems; 3: 64 satellites, every pseudo-range and Doppler of GLONASS grossly wrong (no row of it passes its gate: the clock
    column stays as a zero column); 4: seven satellites of all four constellations, GLONASS first, no ionosphere parameters - for a
    filter whose state lacks two of the clocks; 5: one entry without L1 in the middle.
    -> list of dict(eph, obs, ion, doy, xyzt, velt) / None"""
    def epoch(seed, want, n_glo, order=None, edit=None, ion=ION):
        rng = np.random.default_rng(seed)
        xyz, rcv = _site(BATCH_LAT, BATCH_LON, HGT)
        eph = _sky(rng, rcv, T_RX, want, n_glo)
        if order is not None:
            eph = eph[list(order)]
        sc = _scenario("batch_%d" % seed, rng, eph, xyz, rcv, None, ion=ion, edit=edit, vel=np.asarray(vel_ecef[seed - 200]) - D_VEL)
        return {k: sc[k] for k in ("eph", "obs", "ion", "doy", "xyzt", "velt")}

    def gross(eph, obs):
        g = eph[:, gg.SYS] == 1
        obs[g, gg.PSR] += 400.0
        obs[g, gg.DOPP] += 60.0

    def no_l1(eph, obs):
        obs[5, gg.FREQ] = -1.0
    # _sky order of 1 and 5: GPS 0-3, BDS 4-6, GAL 7-9, GLO 10-11; of 4: GPS 0-1, BDS 2-3, GAL 4-5, GLO 6
    recipe = {0: lambda: epoch(200, (("gps", 0, 1),), 0),
              1: lambda: epoch(201, (("gps", 0, 4), ("bds", 3, 3), ("gal", 2, 3)), 2, order=(4, 0, 5, 10, 7, 1, 8, 11, 2, 6, 9, 3)),
              2: lambda: None,
              3: lambda: epoch(203, (("gps", 0, 20), ("bds", 3, 18), ("gal", 2, 18)), 8, edit=gross),
              4: lambda: epoch(204, (("gps", 0, 2), ("bds", 3, 2), ("gal", 2, 2)), 1, order=(6, 2, 0, 4, 3, 1, 5), ion=None),
              5: lambda: epoch(205, (("gps", 0, 4), ("bds", 3, 3), ("gal", 2, 3)), 2, edit=no_l1)}
    return [recipe[k]() for k in (range(6) if only is None else only)]
