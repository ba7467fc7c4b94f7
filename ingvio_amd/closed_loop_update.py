"""The second MSCKF update of a camera frame in the closed loop of the device-resident nominal state (ingvio_update_stage_tracks_nominal,
DESIGN 4.11) - harness code beside ingvio_amd/closed_loop.py, shared by tests/test_gpu_nominal_update.py,
tests/test_update_form_schedule.py, tests/test_update_form_model.py and tools/closed_loop_bench.py --two-updates: the loop inputs of closed_loop.make_loop split into the two updates of the reference's camera
callback (IngvioFilter.cpp:271-324), the host reference step in the reference's order built from the host-fed entry points, and the
device loop that alternates the two kinds of frame from the table.

Per camera frame f and filter:
  first update   the plain frame from the table: IMU steps, the new clone, the "lost" tracks 0 .. N_LOST - 1 with every stored
                 observation and the points the host sent once (frame 0); it marginalises nothing (fr["marg"] = -1)
  second update  fr["upd"]: the tracks N_LOST .. F - 1 (a count that is no multiple of four) with feat_sel masks over three or four
                 selected window slots, the window's second clone to marginalise (fr["marg_upd"]).  Their points are never handed over:
                 the run triangulates them from every stored observation.
From frame 3 on the first update also lists track N_LOST: its point is the one the previous frame's triangulation left in the store.
Track F - 1 is released and restarted every third frame (one or two stored observations: the triangulation refuses it, Triangulator.cpp:183-187),
track F - 2 carries a gross error of alternating sign in every observation from frame 1 on (the gate's business)."""
import numpy as np

from ingvio_amd.closed_loop import DeviceLoop, Form, HostTable, UpdateEntry, host_propagate, host_stage, make_loop, stage_args

N_LOST = 7


FAR_DEPTH = 2000.0


def far_track(F):
    """first_tri: the track whose true point lies FAR_DEPTH m out, far beyond ingvio_tri_opts' max_depth (60 m): its inverse depth is not
    observable over the window (1e-3 of noise against 5e-4 of parallax per metre of baseline), so whatever the iteration finds, a depth
    beyond max_depth, a negative one or no convergence, the triangulation refuses it - for geometry, with every observation stored"""
    return F - 3


def make_update_loop(B, n_frames, F=24, seed=5, stereo=True, n_lost=N_LOST, carry_point=True, first_tri=False, **kw):
    """closed_loop.make_loop in the two-update form (see the module's text); mono: the right eye's measurements are zero and the
    options name a mono camera; n_lost: the first update's tracks, the second lists the other F - n_lost; carry_point=False: the first
    update never lists a track whose point only the triangulation knows.
    first_tri: no point is ever handed over (no pf_track / pf in any delta) - the first update's stage carries tri
    (ingvio_frame_stage_tracks_nominal_tri) and finds its points itself.  Its list then also names the restarted track F - 1 in the frames
    where that one holds one or two observations (refused for want of observations) and far_track(F) (refused for its geometry)."""
    return split_updates(make_loop(B, n_frames, F=F, seed=seed, **kw), F, stereo, n_lost, carry_point, first_tri)


def far_observations(c, b, F):
    """[n_frames][4]: the far track's measurements from the true camera poses of case c's frames, with the features' pixel noise"""
    from ingvio_amd import synth
    times = [fr["t"] for fr in c["frames"]]
    Rm, pm = synth.true_cam_pose(times[len(times) // 2])
    pw = Rm @ np.array([0.05 * FAR_DEPTH, -0.03 * FAR_DEPTH, FAR_DEPTH]) + pm
    Rlr, tlr = synth.t_cl2cr()
    rng = np.random.default_rng(900 + b)
    out = np.zeros((len(times), 4))
    for f, t in enumerate(times):
        Rc, pc = synth.true_cam_pose(t)
        q = Rc.T @ (pw - pc)
        qr = Rlr @ q + tlr
        out[f] = [q[0] / q[2], q[1] / q[2], qr[0] / qr[2], qr[1] / qr[2]]
    return out + rng.normal(0.0, 1e-3, out.shape)


def split_updates(cases, F=24, stereo=True, n_lost=N_LOST, carry_point=True, first_tri=False):
    """the cases of closed_loop.make_loop (or of a loop built on it: closed_loop_lm.make_lm_loop) in the two-update form, in place"""
    for b, c in enumerate(cases):
        W = len(c["table"].clones) + 1                                   # the window with the frame's new clone
        if not stereo:
            c["frame"] = dict(c["frame"], stereo=0)
        if first_tri:
            c["first_tri"] = True
            far = far_observations(c, b, F)
        for f, fr in enumerate(c["frames"]):
            d = fr["delta"]
            nobs = min(f + 1, W - 1)                                     # the trailing window slots that hold observations
            uv = np.array(d["obs_uv"], dtype=np.float64, copy=True)
            if f >= 1:
                uv[F - 2, 0] += 0.3 * (-1.0) ** f
            if first_tri:
                uv[far_track(F)] = far[f]
            if not stereo:
                uv[:, 2:] = 0.0
            d["obs_uv"] = uv
            if f % 3 == 2:
                d["free"] = [F - 1]
            if first_tri:
                d.pop("pf_track", None); d.pop("pf", None)
            if "pf_track" in d:                                          # only the lost tracks' points travel
                d["pf_track"], d["pf"] = list(range(n_lost)), np.asarray(d["pf"])[:n_lost].copy()
            lost = (list(range(n_lost)) + ([n_lost] if f >= 3 and carry_point else [])) if nobs >= 3 else []
            if first_tri and lost:
                lost += ([F - 1] if f % 3 != 1 else []) + [far_track(F)]
            d["feat_track"], d["feat_anchor"], d["feat_dof"] = lost, [d["append"]] * len(lost), [nobs - 1] * len(lost)
            obs = list(range(W - nobs, W))
            sel = selected_slots(obs)
            tracks = list(range(n_lost, F)) if sel else []
            bits = np.uint64(sum(1 << s for s in sel))
            fr["upd"] = dict(feat_track=tracks, feat_anchor=[W - 1] * len(tracks), feat_dof=[len(sel) - 1] * len(tracks),
                             feat_sel=np.full(len(tracks), bits, dtype=np.uint64))
            fr["marg_upd"], fr["marg"] = fr["marg"], -1
    return cases


def selected_slots(obs):
    """three or four of the window slots that hold observations: the oldest, the middle one, the newest, from five on also the second"""
    n = len(obs)
    return sorted(set([obs[0], obs[n // 2], obs[-1]] + ([obs[1]] if n >= 5 else []))) if n >= 3 else []


def make_keyframe_loop(B, n_frames, F=24, seed=5, first_tri=False, **kw):
    """the two-update form with a key-frame cadence (KeyframeUpdate: two clones leave every other frame): neither update marginalises
    (fr["marg"] = fr["marg_upd"] = -1); behind every second camera frame the window's second and third clone leave through
    ingvio_nominal_tail (fr["tail_pos"] = [1, 2], else []), so the window grows by one clone and shrinks by one in turn.  No landmarks in
    the state.  The window bookkeeping of make_loop (one clone per frame) is redone here: the store's drop list, the append slot, the new
    clone's idx.  first_tri: as make_update_loop's, without the two tracks meant to fail."""
    cases = make_loop(B, n_frames, F=F, seed=seed, n_landmarks=0, **kw)
    for c in cases:
        win, n, leaving = [False] * len(c["table"].clones), c["P"].shape[0], []
        if first_tri:
            c["first_tri"] = True
        for f, fr in enumerate(c["frames"]):
            d = fr["delta"]
            if first_tri:
                d.pop("pf_track", None); d.pop("pf", None)
            d["drop"] = list(leaving)
            win = [w for i, w in enumerate(win) if i not in leaving]
            d["append"] = len(win)
            win.append(True)
            fr["new_idx"], fr["marg"], fr["marg_upd"] = n, -1, -1
            n += 6
            obs = [i for i, w in enumerate(win) if w]
            if "pf_track" in d:
                d["pf_track"], d["pf"] = list(range(N_LOST)), np.asarray(d["pf"])[:N_LOST].copy()
            lost = list(range(N_LOST)) if len(obs) >= 3 else []
            d["feat_track"], d["feat_anchor"], d["feat_dof"] = lost, [d["append"]] * len(lost), [len(obs) - 1] * len(lost)
            sel = selected_slots(obs)
            tracks = list(range(N_LOST, F)) if sel else []
            fr["upd"] = dict(feat_track=tracks, feat_anchor=[len(win) - 1] * len(tracks), feat_dof=[len(sel) - 1] * len(tracks),
                             feat_sel=np.full(len(tracks), np.uint64(sum(1 << s for s in sel)), dtype=np.uint64))
            leaving = [1, 2] if f % 2 == 1 else []
            fr["tail_pos"] = list(leaving)
            n -= 6 * len(leaving)
    return cases


def host_tail_drop(ctx, cases, tabs, f):
    """the key-frame cadence on the host: ingvio_marginalize of the clones at fr["tail_pos"], one by one, and the host tables' drop and shift"""
    for b, (c, t) in enumerate(zip(cases, tabs)):
        for slot in [t.clones[q] for q in c["frames"][f]["tail_pos"]]:
            idx = t.slots[slot]["idx"]
            ctx.marginalize(b, idx, 6)
            t.marginalize(idx)


def update_stage(ctx, cases, f, use_async=False, tri=True, marg=True, sel=True):
    """the stage call of camera frame f's second update (ingvio_update_stage_tracks_nominal); tri=False: the store's points;
    marg=False: nothing leaves the window; sel=False: every stored observation takes part"""
    frames = [c["frames"][f]["upd"] if sel else {k: v for k, v in c["frames"][f]["upd"].items() if k != "feat_sel"} for c in cases]
    return ctx.update_stage_tracks_nominal_prepare(0, [c["frames"][f]["marg_upd"] if marg else -1 for c in cases], frames, stage_args(cases)[0],
                                                   tri={} if tri else None, selected_variant=1 if sel else 0, use_async=use_async)


def host_update_frames(ctx, cases, clones, f, sel=True):
    """what ingvio_msckf_update_tri takes for camera frame f's second update, from the context's track store and the window's clones
    (per filter a list of dicts idx, R, p); -> (frames, tri_masks)"""
    frames, tri_masks = [], []
    for b, (c, cl) in enumerate(zip(cases, clones)):
        u = c["frames"][f]["upd"]
        mask, uv, _ = ctx.debug_tracks_read(b)
        tr = np.asarray(u["feat_track"], dtype=np.int64)
        full = mask[tr] & np.uint64((1 << len(cl)) - 1)
        frames.append(dict(c["frame"], clone_idx=[s["idx"] for s in cl], clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl]),
                           pf=np.zeros((len(tr), 3)), anchor=u["feat_anchor"], dof=u["feat_dof"], uv=uv[tr][:, :len(cl), :],
                           obs_mask=full & u["feat_sel"] if sel else full))
        tri_masks.append(full)
    return frames, tri_masks


def table_clones(nom):
    """the window's clones of one filter's table in the layout of ingvio_nominal_get / HostTable.as_dict()"""
    return [dict(idx=int(nom["idx"][s]), R=np.asarray(nom["val"][s][0:9]).reshape(3, 3), p=np.asarray(nom["val"][s][9:12])) for s in nom["clone_var"]]


def host_second_update(ctx, cases, clones, f, marg=True, sel=True):
    """ingvio_msckf_update_tri with tri_masks, then ingvio_marginalize; -> (dx, accept, gamma, rows, pf, tri_ok)"""
    frames, tri_masks = host_update_frames(ctx, cases, clones, f, sel)
    res = ctx.msckf_update_tri(0, frames, selected_variant=1 if sel else 0, stereo=bool(cases[0]["frame"].get("stereo", 1)), tri_masks=tri_masks)
    for b, c in enumerate(cases):
        if marg and c["frames"][f]["marg_upd"] >= 0:
            ctx.marginalize(b, c["frames"][f]["marg_upd"], 6)
    return res


class HostStore:
    """what a host that keeps its own map holds of one filter's tracks: masks [F], uv [F][c_max][4] and the points its own triangulations
    found; apply() replays a frame's delta (drop, free, append; as k_tracks_apply)"""

    def __init__(self, F, c_max):
        self.mask, self.uv, self.points, self.c_max = np.zeros(F, dtype=np.uint64), np.zeros((F, c_max, 4)), {}, c_max

    def apply(self, d):
        keep = [s for s in range(self.c_max) if s not in d.get("drop", [])]
        if len(keep) < self.c_max:
            self.uv[:, :len(keep)] = self.uv[:, keep]
            bits = np.stack([(self.mask >> np.uint64(s)) & np.uint64(1) for s in keep], axis=1)
            self.mask[:] = (bits << np.arange(len(keep), dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        self.mask[np.asarray(d.get("free", []), dtype=np.int64)] = 0
        tr = np.asarray(d["obs_track"], dtype=np.int64)
        self.uv[tr, d["append"]] = np.asarray(d["obs_uv"]).reshape(-1, 4)
        self.mask[tr] |= np.uint64(1 << d["append"])


def host_first_tri(ctx, cases, tfs, stores, tri=None, poses=None):
    """the first update's points on the host, in front of its stage: the host-fed ingvio_triangulate at the host tables' clones (tfs: the
    track frames of host_propagate) from every observation the host's own stores hold, the anchor's depth test of
    MapServerManager.cpp:290,325 in numpy; the points that succeeded go into the host's store model and travel with the frame's delta
    (pf_track / pf), a feature that failed is listed with an empty selection.  poses [B] of (clone_R, clone_p): the triangulation's clone
    poses where they are not the track frames' (a comparison on the very bits another form staged).
    -> (pf [B][f_max][3], tri_ok [B][f_max])"""
    frames = []
    poses = poses or [(tf["clone_R"], tf["clone_p"]) for tf in tfs]
    for c, tf, st, (cR, cp) in zip(cases, tfs, stores, poses):
        st.apply(tf)
        tr, n = np.asarray(tf["feat_track"], dtype=np.int64), len(tf["clone_idx"])
        full = st.mask[tr] & np.uint64((1 << n) - 1)
        frames.append(dict(c["frame"], clone_idx=tf["clone_idx"], clone_R=cR, clone_p=cp, pf=np.zeros((len(tr), 3)),
                           anchor=tf["feat_anchor"], dof=tf["feat_dof"], uv=st.uv[tr][:, :n, :], obs_mask=full))
    B = len(cases)
    pf, ok = np.zeros((B, ctx.f_max, 3)), np.zeros((B, ctx.f_max), dtype=np.int32)
    if any(len(tf["feat_track"]) for tf in tfs):
        pf, ok = ctx.triangulate(0, frames, stereo=bool(cases[0]["frame"].get("stereo", 1)), **(tri or {}))
        pf, ok = np.array(pf), np.array(ok)
    for b, (tf, st) in enumerate(zip(tfs, stores)):
        nf = len(tf["feat_track"])
        for j in range(nf):
            if ok[b, j] == 1:
                a = tf["feat_anchor"][j]
                if (np.asarray(poses[b][0][a]).reshape(3, 3).T @ (pf[b, j] - np.asarray(poses[b][1][a])))[2] <= 0.0:
                    ok[b, j], pf[b, j] = 2, 0.0
            if ok[b, j] == 1:
                st.points[int(tf["feat_track"][j])] = pf[b, j].copy()
        won = sorted({int(t) for j, t in enumerate(tf["feat_track"]) if ok[b, j] == 1})
        tf["pf_track"], tf["pf"] = won, np.array([st.points[t] for t in won]).reshape(-1, 3)
        sel = np.asarray(tf["feat_sel"], dtype=np.uint64) if tf.get("feat_sel") is not None else np.full(nf, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        tf["feat_sel"] = np.where(ok[b, :nf] == 1, sel, np.uint64(0)).astype(np.uint64)
    return pf, ok


def host_step_update(ctx, cases, tabs, f, points, lm_opts=None, stores=None, staged=None):
    """the reference loop of one camera frame, in the reference's order: host_propagate(marg=False) -> ingvio_frame_stage_tracks -> run ->
    fetch -> host boxPlus; ingvio_msckf_update_tri with tri_masks at the table's values; ingvio_marginalize; host boxPlus / drop / shift.
    points [B]: {track: point} the earlier frames' triangulations found, handed to the store with the first update's delta (what the
    device loop's run writes itself).  lm_opts (cases of closed_loop_lm.make_lm_loop): the landmark update behind the second MSCKF update
    and in front of the marginalisation (IngvioFilter.cpp:281-289), host-fed with the values both updates left.
    stores [B] of HostStore (cases with first_tri): the first update's points come from host_first_tri; its results then carry (pf, tri_ok).
    staged = (first, second), each [B] of (clone_R, clone_p): the clone tables another form staged for the two updates (staged_clones).
    Both triangulations then run on those very bits, and the second update, which ingvio_msckf_update_tri linearises at the clones it
    triangulates from, is formed at them: points compare exactly, and what is left between the forms is the arithmetic of the updates.
    ->((dx, accept, rows), (dx, accept, gamma, rows, pf, tri_ok)[, the landmark update's (dx, rows, accept, gamma, status)])"""
    steps, tfs = host_propagate(cases, tabs, f, marg=False)
    tri1 = host_first_tri(ctx, cases, tfs, stores, poses=staged[0] if staged else None) if stores is not None else None
    for tf, pts in zip(tfs, points):
        if tri1 is not None:                                             # (a track both updates triangulated: the later point, the first update's)
            pts = {**pts, **{int(t): p for t, p in zip(tf["pf_track"], tf["pf"])}}
            tf["pf_track"], tf["pf"] = [], np.zeros((0, 3))
        tr = list(tf.get("pf_track", [])) + sorted(pts)
        tf["pf"] = np.concatenate([np.asarray(tf.get("pf", np.zeros((0, 3)))).reshape(-1, 3), np.array([pts[t] for t in sorted(pts)]).reshape(-1, 3)])
        tf["pf_track"] = tr
    host_stage(ctx, cases, steps, tfs)
    ctx.frame_run()
    first = ctx.frame_fetch()
    if tri1 is not None:
        first = tuple(first) + tri1
    for b, t in enumerate(tabs):
        t.box_plus(first[0][b])
    clones = [[t.slots[s] for s in t.clones] for t in tabs]
    if staged:
        clones = [[dict(idx=s["idx"], R=R, p=p) for s, R, p in zip(cl, cR, cp)] for cl, (cR, cp) in zip(clones, staged[1])]
    second = host_second_update(ctx, cases, clones, f, marg=lm_opts is None)
    lm = None
    for b, t in enumerate(tabs):
        t.box_plus(second[0][b])
    if lm_opts is not None:
        from ingvio_amd import closed_loop_lm as clm
        clm.host_lm_stage(ctx, clm.host_frames(tabs, cases, f), lm_opts)
        ctx.landmark_run()
        lm = ctx.landmark_fetch()
        for b, (c, t) in enumerate(zip(cases, tabs)):
            ctx.marginalize(b, c["frames"][f]["marg_upd"], 6)
            t.box_plus(lm[0][b])
    for b, (c, t) in enumerate(zip(cases, tabs)):
        if c["frames"][f]["marg_upd"] >= 0:
            t.marginalize(c["frames"][f]["marg_upd"])
        points[b] = {int(tr): second[4][b, j].copy() for j, tr in enumerate(c["frames"][f]["upd"]["feat_track"]) if second[5][b, j] == 1}
    return (first, second) if lm is None else (first, second, lm)


def staged_clones(ctx):
    """[B] of (clone_R [n][3][3], clone_p [n][3]): the clone table of the frame ctx has staged (ingvio_debug_staged_frame)"""
    out = []
    for b in range(ctx.batch):
        sf = ctx.debug_staged_frame(b)
        n = sf["n_clones"]
        out.append((sf["clone_R"][:n].reshape(n, 3, 3).copy(), sf["clone_p"][:n].copy()))
    return out


def host_table_of(nom):
    """a HostTable with the values of one filter's ingvio_nominal_get"""
    slots = [None if k < 0 else dict(kind=int(k), idx=int(i), anchor=int(a), R=np.array(v[0:9]).reshape(3, 3), p=np.array(v[9:12]), v=np.array(v[12:15]))
             for k, i, a, v in zip(nom["kind"], nom["idx"], nom["anchor"], nom["val"])]
    return HostTable(slots, [int(s) for s in nom["clone_var"]], nom["v_ext"], nom["v_pose"], nom["v_bg"], nom["v_ba"], nom["gravity"])


def host_observations(cases, frames, c_max):
    """what a host that keeps its own map holds when camera frame f's second update is due, per frame and filter: (tracks' full masks,
    uv [n_feat][c_max][4]) - the store's deltas replayed in numpy (drop, free, append; as k_tracks_apply)"""
    out = {}
    F = 1 + max(max(c["frames"][f]["delta"]["obs_track"]) for c in cases for f in frames)
    state = [(np.zeros(F, dtype=np.uint64), np.zeros((F, c_max, 4))) for _ in cases]
    for f in frames:
        per = []
        for c, (mask, uv) in zip(cases, state):
            d = c["frames"][f]["delta"]
            keep = [s for s in range(c_max) if s not in d.get("drop", [])]
            if len(keep) < c_max:
                uv[:, :len(keep)] = uv[:, keep]
                bits = np.stack([(mask >> np.uint64(s)) & np.uint64(1) for s in keep], axis=1)
                mask[:] = (bits << np.arange(len(keep), dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            mask[np.asarray(d.get("free", []), dtype=np.int64)] = 0
            tr = np.asarray(d["obs_track"], dtype=np.int64)
            uv[tr, d["append"]] = np.asarray(d["obs_uv"]).reshape(-1, 4)
            mask[tr] |= np.uint64(1 << d["append"])
            ut = np.asarray(c["frames"][f]["upd"]["feat_track"], dtype=np.int64)
            per.append((mask[ut].copy(), uv[ut].copy()))
        out[f] = per
    return out


class UpdateRoundTrip(Form):
    """the second update through the host, as a late form of the plain loop (closed_loop.Form's interface): ingvio_nominal_get (a
    synchronisation), ingvio_msckf_update_tri with tri_masks at the table's values, ingvio_marginalize, boxPlus / drop / shift on the
    host, ingvio_nominal_set.  The observations are the host's own (host_observations); its points stay on the host."""
    late = True

    def __init__(self, cases, frames, c_max):
        self.obs = host_observations(cases, frames, c_max)

    def after(self, loop, i):
        ctx, cases, f = loop.ctx, loop.cases, loop.frames[i]
        nom = ctx.nominal_get()
        frames, tri_masks = [], []
        for c, nm, (full, uv) in zip(cases, nom, self.obs[f]):
            u, cl = c["frames"][f]["upd"], table_clones(nm)
            full = full & np.uint64((1 << len(cl)) - 1)
            frames.append(dict(c["frame"], clone_idx=[s["idx"] for s in cl], clone_R=np.stack([s["R"] for s in cl]), clone_p=np.stack([s["p"] for s in cl]),
                               pf=np.zeros((len(full), 3)), anchor=u["feat_anchor"], dof=u["feat_dof"], uv=uv[:, :len(cl), :], obs_mask=full & u["feat_sel"]))
            tri_masks.append(full)
        res = ctx.msckf_update_tri(0, frames, selected_variant=1, stereo=bool(cases[0]["frame"].get("stereo", 1)), tri_masks=tri_masks)
        ctx.marginalize(0, [c["frames"][f]["marg_upd"] for c in cases], 6)
        tabs = []
        for b, (c, nm) in enumerate(zip(cases, nom)):
            t = host_table_of(nm)
            t.box_plus(res[0][b])
            t.marginalize(c["frames"][f]["marg_upd"])
            tabs.append(t.as_dict())
        ctx.nominal_set(0, tabs)


def two_update_entries(frames):
    """the device loop's frame entries: camera frame f, then its second update"""
    out = []
    for f in frames:
        out += [f, UpdateEntry(f)]
    return out


def device_loop_update(ctx, cases, frames, pipelined, sync_every_call=False):
    """the device loop over the two kinds of frame from the table, the plain pipelined order over twice as many entries:
    run(i); ustage(i, async); fetch_begin(i); run_u(i); fetch_end(i); stage(i + 1, async); ...
    -> per camera frame ((dx, accept, rows), (dx, accept, rows, pf, tri_ok))"""
    out = DeviceLoop(ctx, cases, two_update_entries(frames), None, pipelined, sync_every_call, update_stage=update_stage).run()
    return [(out[2 * i], out[2 * i + 1]) for i in range(len(frames))]
