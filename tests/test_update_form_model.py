"""The two-update scenario of ingvio_amd/closed_loop_update.py run through the oracle alone (oracle triangulation, orc_frame_update,
orc_msckf_update, HostTable, the host model of the track store): the conditions the GPU comparison of tests/test_gpu_nominal_update.py
rests on, asserted where no GPU is needed.  The comparison demands EQUAL flags and masks of two forms whose inputs differ by rounding, so
no decision may sit on its threshold; and it must compare something: real updates, both gate verdicts, failed triangulations."""
import copy

import numpy as np
import pytest

from ingvio_amd.closed_loop_update import N_LOST, make_update_loop
from track_store_model import TrackStoreModel

B, F, FRAMES, C_MAX = 8, 24, 10, 12
MIN_DEPTH, MAX_DEPTH = 0.2, 60.0                                          # ingvio_tri_opts' defaults (Triangulator.h:74-75)


def run_filter(c):
    """one filter's loop; -> per camera frame from the third on (accepted, rejected, failed, listed, worst gate margin, worst depth margin)"""
    from oracle import oracle as orc
    cov, tab, store = orc.Cov(c["P"], ld=160), copy.deepcopy(c["table"]), TrackStoreModel(F, C_MAX)
    opts, st = c["frame"], c["step"]
    stereo = bool(opts.get("stereo", 1))
    out = []
    for f, fr in enumerate(c["frames"]):
        e, bg, ba = tab.slots[tab.v_pose], tab.slots[tab.v_bg], tab.slots[tab.v_ba]
        R, p, v, Phi, G = e["R"], e["p"], e["v"], [], []
        for q in range(fr["imu"].shape[0]):
            R, p, v, Ph, Gq = orc.imu_transition(R, p, v, bg["p"], ba["p"], fr["imu"][q, :3], fr["imu"][q, 3:6], tab.gravity, fr["imu"][q, 6])
            Phi.append(Ph); G.append(Gq)
        e["R"], e["p"], e["v"] = R, p, v
        tab.append_clone(fr["new_idx"])
        store.apply(fr["delta"])
        cl = [tab.slots[s] for s in tab.clones]
        n = len(cl)
        win = dict(opts, clone_idx=[s["idx"] for s in cl], clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl]))
        d = fr["delta"]
        g = store.gather(d["feat_track"], d["feat_anchor"], d["feat_dof"])
        step = dict(Phi=Phi, G=G, dt=list(fr["imu"][:, 6]), sigma=st["sigma"], enable_gnss=st["enable_gnss"], gnss_idx=fr["gnss_idx"],
                    sigma_cb=st["sigma_cb"], sigma_rw=st["sigma_rw"], R_i2w=R, marg_idx=-1)
        dx, _, _, _ = orc.frame_update(cov, step, dict(win, pf=g["pf"], anchor=g["anchor"], dof=g["dof"], obs_mask=g["obs_mask"], uv=g["uv"][:, :n]))
        tab.box_plus(dx)
        # the second update, linearised at the state the first one left
        cl = [tab.slots[s] for s in tab.clones]
        win.update(clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl]))
        u = fr["upd"]
        g = store.gather(u["feat_track"], u["feat_anchor"], u["feat_dof"])
        sel = store.gather(u["feat_track"], u["feat_anchor"], u["feat_dof"], u["feat_sel"])["obs_mask"]
        nf = len(u["feat_track"])
        pf, ok, depth_margin = np.zeros((nf, 3)), np.zeros(nf, dtype=bool), np.inf
        for j in range(nf):
            okj, pj = orc.triangulate(win["clone_R"], win["clone_p"], int(g["obs_mask"][j]), g["uv"][j, :n], stereo, opts["R_cl2cr"], opts["t_cl2cr"])
            a = cl[u["feat_anchor"][j]]
            if okj:
                za = (a["R"].T @ (pj - a["p"]))[2]
                for s in range(n):
                    if (int(g["obs_mask"][j]) >> s) & 1:
                        q = cl[s]["R"].T @ (pj - cl[s]["p"])
                        for z in (q[2], (np.asarray(opts["R_cl2cr"]) @ q + np.asarray(opts["t_cl2cr"]))[2]):
                            depth_margin = min(depth_margin, abs(z - MIN_DEPTH) / MIN_DEPTH, abs(z - MAX_DEPTH) / MAX_DEPTH)
                depth_margin = min(depth_margin, abs(za))
                okj = za > 0.0
            ok[j] = okj; pf[j] = pj if okj else 0.0
            if okj:
                store.points[int(u["feat_track"][j])] = pj.copy()
        dx, acc, gam, _ = cov.msckf_update(dict(win, pf=pf, anchor=g["anchor"], dof=g["dof"], obs_mask=np.where(ok, sel, np.uint64(0)), uv=g["uv"][:, :n]),
                                           max_accept=0, compress_rule=1, selected_variant=1)
        cov.marginalize(fr["marg_upd"], 6)
        tab.box_plus(dx)
        tab.marginalize(fr["marg_upd"])
        if nf:
            thr = np.asarray(opts["chi2_table"])[np.asarray(u["feat_dof"])]
            gate_margin = min([abs(gam[j] - thr[j]) / thr[j] for j in range(nf) if ok[j]] + [np.inf])
            out.append((int(acc.sum()), int((ok & (acc == 0)).sum()), int((~ok).sum()), nf, gate_margin, depth_margin))
    return out


@pytest.fixture(scope="module")
def results():
    return [run_filter(c) for c in make_update_loop(B, FRAMES, F)]


def test_every_second_update_carries_rows(results):
    for b, res in enumerate(results):
        assert len(res) == FRAMES - 2
        for f, r in enumerate(res):
            assert r[3] == F - N_LOST and r[0] >= 8, (b, f + 2, r)


def test_both_verdicts_and_failed_triangulations_occur(results):
    for b, res in enumerate(results):
        assert sum(r[1] for r in res) >= 1 and sum(r[2] for r in res) >= 1, (b, res)
        assert 4 * sum(r[2] for r in res) <= sum(r[3] for r in res), (b, res)


def test_no_decision_sits_on_its_threshold(results):
    for b, res in enumerate(results):
        assert min(r[4] for r in res) > 1e-6 and min(r[5] for r in res) > 1e-6, (b, res)
