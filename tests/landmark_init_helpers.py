"""What tests/test_landmark_init_scenarios.py (CPU) and tests/test_gpu_landmark_init.py share: the scenarios of
ingvio_landmark_init_nominal, a numpy restatement of LandmarkUpdate::calcResJacobianSingleFeatAll{Mono,Stereo}Obs
(LandmarkUpdate.cpp:426-500, :803-890) and the reference's loop over new landmarks (:399-421, :928-955) on the C oracle."""
import copy

import numpy as np

from ingvio_amd import synth
from ingvio_amd.closed_loop import LM, make_loop

NOISE = synth.PARAMS["visual_noise"]
PX = 0.02                       # pixel noise of the synthetic observations (a quarter of the filter's sigma)
N_TRACKS = 8
BASELINE = 0.3                  # metres between neighbouring clones of a scenario's window
P_SCALE = 1.0                   # make_loop's prior as it is (a tighter one does not make the gate refuse a wrong point either, see displace_grossly)
T_GOOD, T_GROSS, T_GOOD2, T_GAP, T_SINGLE, T_PAIR = 0, 1, 2, 3, 4, 5


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def numpy_rows(clone_R, clone_p, pf, anchor, obs, stereo):
    """clone_R / clone_p: the window's clones in ascending time; obs: [(window position, uv [4])] ascending; anchor: window position.
    -> (H_old [m, 6 C], H_new [m, 3], res [m]) as the reference forms them."""
    Rlr, tlr = synth.t_cl2cr()
    C = len(clone_R)
    Hx, Hf, res = [], [], []
    for q, uv in obs:
        Rw, pw = clone_R[q], clone_p[q]
        pc = Rw.T @ (pf - pw)                                                          # :460 / :838
        Hp = np.array([[1.0 / pc[2], 0.0, -pc[0] / pc[2] ** 2], [0.0, 1.0 / pc[2], -pc[1] / pc[2] ** 2]])
        D = np.zeros((3, 6 * C))
        if q != anchor:                                                                # :470-474 / :855-860
            D[:, 6 * q:6 * q + 3] = Rw.T @ skew(pf)
            D[:, 6 * anchor:6 * anchor + 3] = -D[:, 6 * q:6 * q + 3]
        D[:, 6 * q + 3:6 * q + 6] = -Rw.T
        Hx.append(Hp @ D); Hf.append(Hp @ Rw.T)
        res.append(np.asarray(uv[:2]) - np.array([pc[0] / pc[2], pc[1] / pc[2]]))
        if stereo:
            pr = Rlr @ pc + tlr                                                        # :839
            Hr = np.array([[1.0 / pr[2], 0.0, -pr[0] / pr[2] ** 2], [0.0, 1.0 / pr[2], -pr[1] / pr[2] ** 2]])
            Hx.append(Hr @ Rlr @ D); Hf.append(Hr @ Rlr @ Rw.T)
            res.append(np.asarray(uv[2:4]) - np.array([pr[0] / pr[2], pr[1] / pr[2]]))
    if not obs:
        return np.zeros((0, 6 * C)), np.zeros((0, 3)), np.zeros(0)
    return np.vstack(Hx), np.vstack(Hf), np.concatenate(res)


def window_of(table):
    cl = [table.slots[s] for s in table.clones]
    return [s["R"] for s in cl], [s["p"] for s in cl], [s["idx"] for s in cl]


def opts_frame(stereo, table=None):
    Rlr, tlr = synth.t_cl2cr()
    return dict(stereo=1 if stereo else 0, R_cl2cr=Rlr, t_cl2cr=tlr, noise=NOISE, chi2_table=synth.chi2_table() if table is None else table)


def make_scenario(windows, seed, drops=None, stereo=True):
    """One filter per window size: covariance and table of closed_loop.make_loop, a track store of N_TRACKS tracks over the window's
    clones plus the pending drop columns drops[b] (store columns, ascending; their measurements are junk that must be skipped).
    Tracks: T_GOOD / T_GOOD2 every clone observes, point near the truth; T_GROSS the same, point displaced grossly; T_GAP a mask with
    gaps that the anchor (window position 0) is not part of; T_SINGLE one observation; T_PAIR two, the anchor's among them."""
    cases = make_loop(len(windows), 1, F=N_TRACKS, seed=seed, windows=[w + 1 for w in windows], n_landmarks=0)      # build_case: C - 1 clones in the prior window
    Rlr, tlr = synth.t_cl2cr()
    out = []
    for b, c in enumerate(cases):
        rng = np.random.default_rng(1000 * seed + b)
        t = copy.deepcopy(c["table"])
        Cw = len(t.clones)
        side = t.slots[t.clones[Cw // 2]]["R"][:, 0]
        for q, sl in enumerate(t.clones):                                               # make_loop's clones lie millimetres apart: spread them,
            t.slots[sl]["p"] = t.slots[sl]["p"] + BASELINE * q * side                    # so that a wrong point is inconsistent between the views
        cR, cp, _ = window_of(t)
        drop = list((drops or {}).get(b, []))
        n_store = max([Cw + len(drop)] + [s + 1 for s in drop])
        cols = [s for s in range(n_store) if s not in drop][:Cw]                       # window position -> store column
        pts = []
        while len(pts) < N_TRACKS:
            depth = rng.uniform(4.0, 12.0)
            pw = cR[Cw // 2] @ np.array([rng.uniform(-0.3, 0.3) * depth, rng.uniform(-0.2, 0.2) * depth, depth]) + cp[Cw // 2]
            qs = [R.T @ (pw - p) for R, p in zip(cR, cp)]
            if all(q[2] > 1.0 and (Rlr @ q + tlr)[2] > 1.0 for q in qs):
                pts.append(pw)
        pts = np.array(pts)
        uv = np.zeros((N_TRACKS, n_store, 4))
        mask = np.zeros(N_TRACKS, dtype=np.uint64)
        wmask = [(1 << Cw) - 1] * N_TRACKS                                              # over window positions
        wmask[T_GAP] = sum(1 << q for q in range(1, Cw) if q % 3 != 2) if Cw > 3 else 0b110
        wmask[T_SINGLE] = 1 << (Cw - 1)
        wmask[T_PAIR] = 0b11
        for j in range(N_TRACKS):
            m = 0
            for q in range(Cw):
                if not (wmask[j] >> q) & 1:
                    continue
                pc = cR[q].T @ (pts[j] - cp[q]); pr = Rlr @ pc + tlr
                uv[j, cols[q]] = np.array([pc[0] / pc[2], pc[1] / pc[2], pr[0] / pr[2], pr[1] / pr[2]]) + rng.normal(0.0, PX, 4)
                m |= 1 << cols[q]
            for s in drop:                                                              # the clone has left the window: junk, bit set
                uv[j, s] = rng.normal(0.0, 0.3, 4)
                m |= 1 << s
            mask[j] = m
        if not stereo:
            uv[:, :, 2:] = 0.0
        pf = pts + rng.normal(0.0, 0.01, pts.shape)
        anchor = [0] * N_TRACKS
        anchor[T_SINGLE] = Cw - 1
        c = dict(c, table=t)
        f = dict(P=P_SCALE * c["P"], table=t, case=c, Cw=Cw, drop=drop, cols=cols, uv=uv, mask=mask, wmask=wmask, pf=pf, anchor=anchor, stereo=stereo)
        displace_grossly(f, pts[T_GROSS])
        out.append(f)
    return out


def displace_grossly(f, true):
    """T_GROSS, the candidate the gate must refuse.  A wrong POINT alone is not refused in these windows: the new variable and the
    window's prior absorb it (the oracle's chi2 stays below 0.3 of its threshold for displacements of 5 to 12 m, at the loop's prior
    and at a prior 1000 times tighter).  So the point is displaced by 1.5 m AND the track's observations are grossly inconsistent:
    +-0.5 in normalised image coordinates, alternating from view to view."""
    f["pf"][T_GROSS] = true + np.array([1.5, -1.0, 0.5])
    for q in range(f["Cw"]):
        f["uv"][T_GROSS, f["cols"][q]] += (0.5 if q % 2 == 0 else -0.5) * (np.array([1.0, -1.0, 1.0, -1.0]) if f["stereo"] else np.array([1.0, -1.0, 0.0, 0.0]))


def obs_of(f, track):
    return [(q, f["uv"][track, f["cols"][q]]) for q in range(f["Cw"]) if (f["wmask"][track] >> q) & 1]


def rows_at(f, table, track):
    cR, cp, _ = window_of(table)
    return numpy_rows(cR, cp, f["pf"][track], f["anchor"][track], obs_of(f, track), f["stereo"])


def enter_landmark(table, slot, idx, anchor_pos, pf):
    """the new landmark in the host table, in the slot the call reserves (free slots in between stay None)"""
    while len(table.slots) <= slot:
        table.slots.append(None)
    table.slots[slot] = dict(kind=LM, idx=idx, anchor=table.clones[anchor_pos], R=np.eye(3), p=np.array(pf, dtype=float), v=np.zeros(3))


def free_slots(table, v_max=48):
    return [i for i in range(v_max) if i >= len(table.slots) or table.slots[i] is None]


def oracle_sequence(f, tracks, reform=True, chi2_mult=1.0):
    """the reference's loop (LandmarkUpdate.cpp:399-421) for one filter on the C oracle: candidate by candidate, boxPlus in between.
    reform=False: every candidate's rows at the poses before the first one (what ingvio_add_variable_delayed_batch is handed).
    -> dict(added, new_idx, slot, chi2, thr, m, dx, P, n, table)"""
    from oracle import oracle as orc
    tab = synth.chi2_table()
    t = copy.deepcopy(f["table"])
    t0 = copy.deepcopy(f["table"])
    cov = orc.Cov(f["P"], ld=f["P"].shape[0] + 3 * len(tracks) + 8)
    res = dict(added=[], new_idx=[], slot=[], chi2=[], thr=[], m=[], dx=[])
    slots = free_slots(t)
    for j, tr in enumerate(tracks):
        H_old, H_new, r = rows_at(f, t if reform else t0, tr)
        m = H_old.shape[0]
        _, _, cidx = window_of(t)
        res["m"].append(m); res["thr"].append(chi2_mult * tab[m])
        if m <= 3:
            res["added"].append(False); res["new_idx"].append(-1); res["slot"].append(-1); res["chi2"].append(0.0); res["dx"].append(None)
            continue
        n0 = cov.n
        a, dx, g = cov.add_variable_delayed(cidx, [6] * len(cidx), H_old, H_new, r, NOISE, chi2_mult, True, tab[m])
        res["added"].append(a); res["new_idx"].append(n0 if a else -1); res["slot"].append(slots[j] if a else -1); res["chi2"].append(g)
        res["dx"].append(dx if a else None)
        if a:
            enter_landmark(t, slots[j], n0, f["anchor"][tr], f["pf"][tr])
            t.box_plus(dx)
    P = cov.P() if callable(cov.P) else cov.P
    res.update(P=np.array(P)[:cov.n, :cov.n], n=cov.n, table=t)
    return res


def blocks_of(scn, tracks_per_filter):
    return [dict(cands=[(tr, f["anchor"][tr], f["pf"][tr]) for tr in trs], drop=f["drop"]) for f, trs in zip(scn, tracks_per_filter)]


# the scenarios of the GPU tests (windows 3 ... 12; c_max = 16 leaves room for the pending drop columns)
ROW_WINDOWS = (3, 6, 11, 12)
ROW_DROPS = {1: [0], 2: [1, 12], 3: [13]}           # column 0, a middle column with one above every observation, one above every observation
MIXED_WINDOWS = (3, 5, 8, 11)
SEQ_WINDOWS = (6, 11, 4)
SEQ_TRACKS = (T_GOOD, T_GROSS, T_GOOD2)
