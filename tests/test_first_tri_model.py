"""The two-update scenario with triangulating first updates (closed_loop_update.make_update_loop(first_tri=True)) run through the oracle
alone (oracle triangulation, orc_frame_update, orc_msckf_update, HostTable, the host model of the track store): the conditions the GPU
comparison of tests/test_gpu_nominal_first_tri.py rests on, asserted where no GPU is needed.  No point is ever handed over: the first
update's points come from the window's clones behind the propagation and the new clone, from every stored observation."""
import copy

import numpy as np
import pytest

from ingvio_amd.closed_loop_update import far_track, make_update_loop
from track_store_model import TrackStoreModel

B, F, FRAMES, C_MAX = 6, 24, 10, 12


def oracle_tri(cl, opts, mask, uv, anchor, stereo):
    """-> (ok, point): the oracle's triangulation and the anchor's depth test (MapServerManager.cpp:290,325)"""
    from oracle import oracle as orc
    n = len(cl)
    ok, p = orc.triangulate(np.stack([s["R"] for s in cl]), np.stack([s["p"] for s in cl]), int(mask), uv[:n], stereo, opts["R_cl2cr"], opts["t_cl2cr"])
    if ok and (cl[anchor]["R"].T @ (p - cl[anchor]["p"]))[2] <= 0.0:
        ok = False
    return bool(ok), p


def run_filter(c):
    """one filter's loop; -> per camera frame from the third on, of its FIRST update: (listed tracks, their triangulation verdicts,
    accepted)"""
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
        d = fr["delta"]
        assert "pf_track" not in d and "pf" not in d
        store.apply(d)
        cl = [tab.slots[s] for s in tab.clones]
        n = len(cl)
        win = dict(opts, clone_idx=[s["idx"] for s in cl], clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl]))
        g = store.gather(d["feat_track"], d["feat_anchor"], d["feat_dof"])
        nf = len(d["feat_track"])
        ok, pf = np.zeros(nf, dtype=bool), np.zeros((nf, 3))
        for j in range(nf):
            ok[j], pj = oracle_tri(cl, opts, g["obs_mask"][j], g["uv"][j], d["feat_anchor"][j], stereo)
            if ok[j]:
                pf[j] = pj; store.points[int(d["feat_track"][j])] = pj.copy()
        step = dict(Phi=Phi, G=G, dt=list(fr["imu"][:, 6]), sigma=st["sigma"], enable_gnss=st["enable_gnss"], gnss_idx=fr["gnss_idx"],
                    sigma_cb=st["sigma_cb"], sigma_rw=st["sigma_rw"], R_i2w=R, marg_idx=-1)
        dx, acc, _, _ = orc.frame_update(cov, step, dict(win, pf=pf, anchor=g["anchor"], dof=g["dof"], obs_mask=np.where(ok, g["obs_mask"][:nf], np.uint64(0)),
                                                        uv=g["uv"][:, :n]))
        tab.box_plus(dx)
        if f >= 2:
            out.append((list(d["feat_track"]), ok.copy(), np.asarray(acc)[:nf].copy()))
        # the second update, linearised at the state the first one left
        cl = [tab.slots[s] for s in tab.clones]
        win.update(clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl]))
        u = fr["upd"]
        g = store.gather(u["feat_track"], u["feat_anchor"], u["feat_dof"])
        sel = store.gather(u["feat_track"], u["feat_anchor"], u["feat_dof"], u["feat_sel"])["obs_mask"]
        nu = len(u["feat_track"])
        ok2, pf2 = np.zeros(nu, dtype=bool), np.zeros((nu, 3))
        for j in range(nu):
            ok2[j], pj = oracle_tri(cl, opts, g["obs_mask"][j], g["uv"][j], u["feat_anchor"][j], stereo)
            if ok2[j]:
                pf2[j] = pj; store.points[int(u["feat_track"][j])] = pj.copy()
        dx, _, _, _ = cov.msckf_update(dict(win, pf=pf2, anchor=g["anchor"], dof=g["dof"], obs_mask=np.where(ok2, sel[:nu], np.uint64(0)), uv=g["uv"][:, :n]),
                                       max_accept=0, compress_rule=1, selected_variant=1)
        cov.marginalize(fr["marg_upd"], 6)
        tab.box_plus(dx)
        tab.marginalize(fr["marg_upd"])
    return out


@pytest.fixture(scope="module")
def results():
    return [run_filter(c) for c in make_update_loop(B, FRAMES, F, first_tri=True)]


def test_first_updates_list_enough_tracks_and_they_triangulate(results):
    for b, res in enumerate(results):
        assert len(res) == FRAMES - 2
        for f, (tracks, ok, acc) in enumerate(res):
            assert len(tracks) >= 7, (b, f + 2)
            for t, o in zip(tracks, ok):
                assert o == (t not in (F - 1, far_track(F))), (b, f + 2, t)


def test_half_of_the_listed_features_pass_the_gate(results):
    for b, res in enumerate(results):
        for f, (tracks, ok, acc) in enumerate(res):
            assert 2 * int(acc.sum()) >= len(tracks), (b, f + 2, int(acc.sum()), len(tracks))


def test_the_far_track_is_refused_wherever_it_is_listed(results):
    listed = 0
    for b, res in enumerate(results):
        for f, (tracks, ok, acc) in enumerate(res):
            assert far_track(F) in tracks, (b, f + 2)
            j = tracks.index(far_track(F))
            assert not ok[j] and not acc[j], (b, f + 2)
            listed += 1
    assert listed == B * (FRAMES - 2)
