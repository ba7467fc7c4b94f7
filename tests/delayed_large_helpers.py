"""What tests/test_delayed_large_model.py (CPU) and tests/test_gpu_delayed_large.py share: the scenarios of the large form of the
delayed-initialisation front (ingvio_set_delayed_form), their oracle results computed once, and a context for the
landmark-init scenarios of landmark_init_helpers.py at windows of up to 36 clones."""
import numpy as np

import landmark_init_helpers as H
from oracle import oracle as orc
from test_gpu_delayed_batch import NOISE, STEREO, SUBSET, WINDOWS, chi2_check, make_cand, mixed_batch
from test_landmark_path import spd

PANEL = 64                      # columns of a sweep panel (DLL_W, kernels_delayed.hip)
V_MAX = 56
LM_WINDOWS = {True: (20, 27), False: (35,)}
LM_DROPS = {True: {1: [3]}, False: {}}                  # one pending drop column below observations, on the 27-clone filter


def clones(first, count):
    return [21 + 6 * i for i in range(first, first + count)]


def refuse(cand):
    v, s, h, r, res, chk = cand
    return (v, s, h, r, 50.0 * np.ones(h.shape[0]), chk)


def small_batch():
    """the existing mixed batch (3 ... 16 clones, stereo and mono, two non-contiguous column maps, s = 3) and beside it s = 1 and 6,
    m = s + 1, odd m, and column counts around the panel width: 63, 64, 65 and 129"""
    priors, blocks = mixed_batch()
    rng = np.random.default_rng(4711)
    n = 21 + 6 * 19
    for vidx, vsize, m, s in (([0] + clones(0, 9), [9] + [6] * 9, 23, 1),                       # nc = 63, odd m
                              ([0] + clones(2, 9), [10] + [6] * 9, 24, 6),                      # nc = 64
                              ([0] + clones(1, 9), [11] + [6] * 9, 7, 6),                       # nc = 65, m = s + 1
                              ([0] + clones(0, 19), [15] + [6] * 19, 31, 3),                    # nc = 129 = 2 * 64 + 1
                              ([21], [6], 2, 1),                                                # the smallest m that is not skipped
                              ([0] + clones(3, 9), [9] + [6] * 9, 23, 3)):                      # refused by the gate
        priors.append(spd(n, rng, 1e-2))
        blocks.append([make_cand(rng, vidx, vsize, m, s)])
    blocks[-1] = [refuse(blocks[-1][0])]
    return priors, blocks


LARGE_SHAPES = ((18, True, 0), (27, True, 0), (36, True, 4), (27, False, 0), (36, False, 4))      # clones, stereo, GNSS scalars behind the clones


def large_batch():
    """one filter per shape the LDS form cannot take; per filter a refused candidate, then an accepted one"""
    rng = np.random.default_rng(360)
    priors, blocks = [], []
    for Cw, st, tail in LARGE_SHAPES:
        priors.append(spd(21 + 6 * Cw + tail, rng, 1e-2))
        m = (4 if st else 2) * Cw
        blocks.append([refuse(make_cand(rng, clones(0, Cw), [6] * Cw, m, 3)), make_cand(rng, clones(0, Cw), [6] * Cw, m, 3)])
    return priors, blocks


def mixed_forms_batch():
    """an 11-clone filter (LDS form), a 27-clone filter (large form), an empty filter, a 27-clone filter refused by the gate"""
    rng = np.random.default_rng(1127)
    priors = [spd(21 + 66, rng, 1e-2)] + [spd(21 + 162, rng, 1e-2) for _ in range(3)]
    blocks = [[make_cand(rng, clones(0, 11), [6] * 11, 44, 3)], [make_cand(rng, clones(0, 27), [6] * 27, 108, 3)], [],
              [refuse(make_cand(rng, clones(0, 27), [6] * 27, 108, 3))]]
    return priors, blocks


def sequence_batch():
    """27 clones: three candidates with a refused middle one, stereo and mono"""
    rng = np.random.default_rng(2703)
    priors, blocks = [], []
    for st in (True, False):
        priors.append(spd(21 + 162, rng, 1e-2))
        cs = [make_cand(rng, clones(0, 27), [6] * 27, (4 if st else 2) * 27, 3) for _ in range(3)]
        cs[1] = refuse(cs[1])
        blocks.append(cs)
    return priors, blocks


def partial_batch():
    """four filters of 18 clones; the call takes filters 1 and 2"""
    rng = np.random.default_rng(1802)
    priors = [spd(21 + 108, rng, 1e-2) for _ in range(4)]
    blocks = [[make_cand(rng, clones(0, 18), [6] * 18, 72, 3)], [refuse(make_cand(rng, clones(0, 18), [6] * 18, 72, 3)), make_cand(rng, clones(0, 18), [6] * 18, 36, 3)]]
    return priors, blocks


SCENARIOS = dict(small=small_batch, large=large_batch, mixed_forms=mixed_forms_batch, sequence=sequence_batch, partial=partial_batch)


def oracle_run(P0, cands, chi2_mult=1.0, do_chi2=True):
    """test_gpu_delayed_batch.oracle_run, which also records per tried candidate the relative distance of chi2 from its threshold and
    the smallest eigenvalue of the trailing update's S on the covariance the candidate met -> (that function's tuple, gaps, eigs)"""
    c = orc.Cov(P0)
    added, idx, chi2, dxs, gaps, eigs = [], [], [], [], [], []
    for vidx, vsize, H_old, H_new, res, chk in cands:
        m, s = H_new.shape
        n0 = c.n
        if m <= s:
            a, dx, g = False, None, 0.0
        else:
            cols = np.concatenate([np.arange(i, i + k) for i, k in zip(vidx, vsize)])
            Pcc = np.array(c.P)[np.ix_(cols, cols)]
            Hu = np.linalg.qr(H_new, mode="complete")[0].T[s:] @ H_old
            eig = float(np.linalg.eigvalsh(Hu @ Pcc @ Hu.T + NOISE * NOISE * np.eye(m - s)).min())
            a, dx, g = c.add_variable_delayed(vidx, vsize, H_old, H_new, res, NOISE, chi2_mult, do_chi2, chk)
            gaps.append(abs(g - chi2_mult * chk) / (chi2_mult * chk))
            if a:
                eigs.append(eig)
        added.append(a); idx.append(n0 if a else -1); chi2.append(g); dxs.append(dx if a else None)
    return (c, added, idx, chi2, dxs), gaps, eigs


_cache = {}


def reference(name):
    """(priors, blocks, [oracle_run of every filter]) of a scenario, computed once and left unchanged"""
    if name not in _cache:
        priors, blocks = SCENARIOS[name]()
        off = 1 if name == "partial" else 0
        _cache[name] = (priors, blocks, [oracle_run(priors[off + i], cs) for i, cs in enumerate(blocks)])
    return _cache[name]


def lm_scenario(stereo):
    key = ("lm", stereo)
    if key not in _cache:
        _cache[key] = H.make_scenario(LM_WINDOWS[stereo], seed=7, drops=LM_DROPS[stereo], stereo=stereo)
    return _cache[key]


def reference_rows(f, table, tr):
    """oracle/stream_filter.py::feat_all_obs_rows on the window of `table` -> (H_old, H_new, res, smallest |depth| / |p_c| of an observer)"""
    import types
    from ingvio_amd import synth
    from oracle import stream_filter as sf
    cR, cp, _ = H.window_of(table)
    Rlr, tlr = synth.t_cl2cr()
    sw = {}
    for q in range(f["Cw"]):
        v = sf.Var("se3", 6); v.R, v.p = cR[q], cp[q]
        sw[float(q)] = v
    flt = types.SimpleNamespace(sw=sw, stereo=f["stereo"], R_cl2cr=Rlr, t_cl2cr=tlr, sw_sorted=lambda: sorted(sw.items()))
    fi = sf.Feature()
    fi.pf, fi.anchor = f["pf"][tr], sw[float(f["anchor"][tr])]
    fi.obs = {float(q): tuple(uv) for q, uv in H.obs_of(f, tr)}
    res, Hx, Hf = sf.Filter.feat_all_obs_rows(flt, fi)
    depth = np.inf
    for q, _ in H.obs_of(f, tr):
        pc = cR[q].T @ (f["pf"][tr] - cp[q])
        for p in ([pc, Rlr @ pc + tlr] if f["stereo"] else [pc]):
            depth = min(depth, abs(p[2]) / np.linalg.norm(p))
    return Hx, Hf, res, depth


LM_TRACKS = (H.T_GOOD, H.T_GROSS, H.T_GOOD2)          # a sequence with a refused middle candidate; the third is formed at the moved poses


def lm_ctx(scn, form=1):
    """landmark_init_helpers' scenario on a context of 36 clones: covariances, tables and the track store (filled column by column)"""
    from ingvio_amd import capi
    B = len(scn)
    n_max = ((max(f["P"].shape[0] for f in scn) + 12 + 15) // 16) * 16
    ctx = capi.Context(batch=B, n_max=n_max, c_max=36, f_max=H.N_TRACKS, m_max=64)
    ctx.tracks_create(H.N_TRACKS)
    ctx.nominal_create(V_MAX)
    for b, f in enumerate(scn):
        ctx.cov_set(b, f["P"])
    ctx.nominal_set(0, [f["table"].as_dict() for f in scn])
    raw = dict(imu=np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 9.8, 0.005]]), R=np.eye(3), p=np.zeros(3), v=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3),
               gravity=np.array([0.0, 0.0, -9.8]))
    sigma = scn[0]["case"]["step"]["sigma"]
    for col in range(max(f["uv"].shape[1] for f in scn)):
        frames = []
        for f in scn:
            tr = [j for j in range(H.N_TRACKS) if col < f["uv"].shape[1] and (int(f["mask"][j]) >> col) & 1]
            frames.append(dict(append=col if tr else -1, obs_track=tr, obs_uv=f["uv"][tr, col] if tr else np.zeros((0, 4)), clone_idx=[],
                               clone_R=np.zeros((0, 9)), clone_p=np.zeros((0, 3)), feat_track=[], feat_anchor=[], feat_dof=[]))
        ctx.frame_stage_tracks_prepare(0, [dict(raw=raw)] * B, frames, H.opts_frame(scn[0]["stereo"]), sigma)()
    ctx.sync()
    ctx.set_delayed_form(form)
    return ctx
