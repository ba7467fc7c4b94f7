"""The MSCKF anchor change and the invalid-feature erase in the closed loop of the device-resident nominal state (ingvio_tracks_maintain,
DESIGN 4.11) - harness code beside closed_loop_update.py, shared by tests/test_maintain_model.py, tests/test_maintain_schedule.py and
tests/test_gpu_tracks_maintain.py:
  - `host_maintain`, the step on a HostTable and a HostStore in the reference's order: changeMSCKFAnchor (KeyframeUpdate.cpp:280-328,
    SwMargUpdate.cpp:367-413) over the tracks anchored to a clone that leaves, then eraseInvalidFeatures (MapServerManager.cpp:456-491)
    over every track that holds a point, with the anchor bookkeeping a host keeps (`Anchors`);
  - `maintain_words`, the list ingvio_tracks_maintain takes for the same step, from integers alone;
  - `add_decoys`, decoy tracks on the loops of closed_loop_update.py placed from the known trajectory so that every verdict occurs;
  - `MaintainForm`, the call as a form of closed_loop.DeviceLoop: synchronous (a late form) or free-running (_begin behind run(i), _end
    behind run(i + 1)).
A store's `points` dict is has_point: a track is in it exactly while the reference's _isTri is set."""
import numpy as np

from ingvio_amd.capi import (MAINTAIN_ERASED_INVALID, MAINTAIN_ERASED_MOVE, MAINTAIN_ERASED_UNTRIANGULATED, MAINTAIN_KEEP, MAINTAIN_MOVED,
                             maintain_word)
from ingvio_amd.closed_loop import LM, SE3, SE23, VEC3, Form, HostTable, UpdateEntry

KEEP, MOVED, ERASED_UNTRIANGULATED, ERASED_MOVE, ERASED_INVALID = (MAINTAIN_KEEP, MAINTAIN_MOVED, MAINTAIN_ERASED_UNTRIANGULATED,
                                                                   MAINTAIN_ERASED_MOVE, MAINTAIN_ERASED_INVALID)
ERASED = (ERASED_UNTRIANGULATED, ERASED_MOVE, ERASED_INVALID)
MIN_DEPTH = 0.2                                                          # MapServerManager.cpp:476
MOVE_MIN_DEPTH = dict(sw=0.0, kf=0.3)                                    # SwMargUpdate.cpp:395 / KeyframeUpdate.cpp:311


def depth_at(R, p, pf):
    """(R^T (pf - p)).z in the kernel's order of operations: three differences, three products, two sums"""
    R, d = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(pf, dtype=np.float64) - np.asarray(p, dtype=np.float64)
    return float(R[0, 2] * d[0] + R[1, 2] * d[1] + R[2, 2] * d[2])


class Anchors:
    """the anchor bookkeeping of one filter's MSCKF tracks as a host keeps it: track -> the table slot of its anchor clone"""

    def __init__(self, slot_of=None):
        self.slot = dict(slot_of or {})

    def leaving(self, slots):
        return sorted(t for t, s in self.slot.items() if s in slots)


def erase(store, anchors, t):
    """MapServer::erase of an MSCKF track on the host model: observations, point and anchor go (as free_tracks)"""
    store.mask[t] = 0
    store.points.pop(t, None)
    anchors.slot.pop(t, None)


def host_maintain(table, store, anchors, leaving, move_min_depth, min_depth=MIN_DEPTH):
    """The step in the reference's order on table (HostTable), store (HostStore: mask, points) and anchors (Anchors): `leaving` are the
    table slots of the clones about to leave (they may already be gone from the table: only the newest clone's pose is read for them).
    -> {track: (verdict, depth)} of every track either step visited and decided on (depth None where none was formed)."""
    out = {}
    new = table.clones[-1]
    na = table.slots[new]
    gone = []
    for t in anchors.leaving(set(leaving)):                              # changeMSCKFAnchor
        if t in store.points:
            d = depth_at(na["R"], na["p"], store.points[t])
            if d <= move_min_depth:
                out[t] = (ERASED_MOVE, d); gone.append(t)
                continue
            anchors.slot[t] = new
            out[t] = (MOVED, d)
        else:
            out[t] = (ERASED_UNTRIANGULATED, None); gone.append(t)
    for t in gone:
        erase(store, anchors, t)
    gone = []
    for t in sorted(anchors.slot):                                       # eraseInvalidFeatures
        if t not in store.points:
            out.setdefault(t, (KEEP, None))
            continue
        a = table.slots[anchors.slot[t]]
        d = depth_at(a["R"], a["p"], store.points[t])
        if d <= min_depth:                                               # (a NaN depth keeps the track, MsckfUpdates.cpp:613)
            out[t] = (ERASED_INVALID, d); gone.append(t)
        else:
            out.setdefault(t, (KEEP, d))
    for t in gone:
        erase(store, anchors, t)
    return out


def host_landmarks(table, lm_slots, min_depth=MIN_DEPTH):
    """the report on in-state landmarks: ERASED_INVALID where the table's value lies at depth <= min_depth in its table anchor"""
    out = []
    for sl in lm_slots:
        s = table.slots[sl]
        a = table.slots[s["anchor"]]
        out.append(ERASED_INVALID if depth_at(a["R"], a["p"], s["p"]) <= min_depth else KEEP)
    return out


def maintain_words(clones, anchors, leaving):
    """the list of ingvio_tracks_maintain for host_maintain's step, from integers alone: clones the table's window list (slots) at the
    call's place in the stream, anchors an Anchors, leaving the slots of the clones that leave.  -> (tracks, words)"""
    pos = {s: q for q, s in enumerate(clones)}
    tracks = sorted(anchors.slot)
    words = []
    for t in tracks:
        mv = anchors.slot[t] in leaving
        words.append(maintain_word(t, len(clones) - 1 if mv else pos[anchors.slot[t]], mv))
    return tracks, words


def apply_verdicts(anchors, tracks, verdicts, new_slot):
    """the host's integer bookkeeping behind a call: moved tracks take the newest clone, erased ones leave the map; -> erased tracks"""
    gone = []
    for t, v in zip(tracks, verdicts):
        if v == MOVED:
            anchors.slot[t] = new_slot
        elif v in ERASED:
            anchors.slot.pop(t, None); gone.append(t)
    return gone


# ---- a random table (the single-call tests) --------------------------------------------------------------------------------------
def rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def make_table(rng, C, identity_ends=False, n_lm=0):
    """pose | bg | ba | extrinsics | C clones (| n_lm landmarks anchored round-robin); identity_ends: the first and the newest clone are
    the identity at the origin"""
    slots, idx = [], [0]

    def add(kind, size, R=None, p=None, anchor=-1):
        slots.append(dict(kind=kind, idx=idx[0], anchor=anchor, R=np.eye(3) if R is None else R, p=np.zeros(3) if p is None else np.asarray(p, dtype=float),
                          v=np.zeros(3)))
        idx[0] += size
        return len(slots) - 1
    v_pose, v_bg, v_ba, v_ext = add(SE23, 9, rot(rng), rng.normal(size=3)), add(VEC3, 3), add(VEC3, 3), add(SE3, 6, rot(rng))
    clones = []
    for q in range(C):
        ident = identity_ends and q in (0, C - 1)
        clones.append(add(SE3, 6, None if ident else rot(rng), None if ident else rng.normal(size=3)))
    lms = [add(LM, 3, p=rng.normal(size=3) * 4.0, anchor=clones[l % C]) for l in range(n_lm)]
    return HostTable(slots, clones, v_ext, v_pose, v_bg, v_ba, [0.0, 0.0, -9.8]), idx[0], lms


# ---- decoy tracks on the loops of closed_loop_update.py ----------------------------------------------------------------------------
DECOYS = 3
KEEPER, MOVER, INVALID = 0, 1, 2                                         # decoy j is track F + j
REAL, POISON_FRAME = 3, 2                                                # the update-listed track that is erased, and the camera frame behind which


def add_decoys(cases, F, mode="sw"):
    """Three decoy tracks F .. F + 2 per filter on the cases of make_update_loop(first_tri=True) (mode "sw": the window's second clone
    leaves with every second update) or make_keyframe_loop (mode "kf": the clones at fr["tail_pos"] leave), in place.  No update lists
    them; every frame's delta observes them (zero measurements) and seeds their points through pf_track, placed from the start table
    and the true trajectory metres from every threshold (the filters' poses follow the truth to centimetres; tests/test_maintain_model.py):
      F + KEEPER   anchored to the oldest clone (it never leaves), 8 m in front of it: KEEP in every call
      F + INVALID  anchored to the oldest clone, seeded 3 m or more BEHIND it in camera frames 0, 3, 6: ERASED_INVALID there; it is observed
                   again under the same number from the next frame on - the restarted track - and holds no point until the next seed
      F + MOVER    released and restarted in every frame, anchored to the window's second clone; when that clone leaves: no point
                   (ERASED_UNTRIANGULATED), a point 9 m in front of the newest clone (MOVED) or 3 m behind it (ERASED_MOVE), in turn,
                   starting at a class that differs from filter to filter
    And one track the updates DO list: track REAL, one of the first update's, anchored to the clone of its first observation.  The
    second update's delta of camera frame POISON_FRAME overwrites its point (triangulated by the first update of that frame, which
    accepted it) with one 3 m behind that anchor (seed_upd): the call behind that frame erases it (ERASED_INVALID).  The next first
    updates list it all the same - as a restarted track of one, then two observations its triangulation is refused and it drops out as
    accepted = 0; from three observations on it is accepted again.
    fr["decoy"] = dict(seed={track: point}, seed_upd={track: point}, free=[tracks], cls=None / 0 / 1 / 2, leave_pos=[window positions
    that leave]).  The stores must hold F + DECOYS tracks."""
    from ingvio_amd import synth
    for b, c in enumerate(cases):
        t0 = c["table"]
        a0 = t0.slots[t0.clones[0]]
        c["decoy_mode"], c["decoy_F"] = mode, F
        R0, p0 = synth.true_cam_pose(c["frames"][0]["t"])
        events = 0
        for f, fr in enumerate(c["frames"]):
            d = fr["delta"]
            leave_pos = [1] if mode == "sw" else list(fr["tail_pos"])
            seed, cls = {}, None
            if f == 0:
                seed[F + KEEPER] = a0["R"] @ np.array([0.3, -0.2, 8.0]) + a0["p"]
            if f % 3 == 0:
                seed[F + INVALID] = a0["R"] @ np.array([0.2, 0.1, -3.0 - b]) + a0["p"]
            if leave_pos:
                cls = (events + b) % 3
                events += 1
                Rn, pn = synth.true_cam_pose(fr["t"])
                if cls == 1:
                    seed[F + MOVER] = Rn @ np.array([0.1, 0.1, 9.0]) + pn
                elif cls == 2:
                    seed[F + MOVER] = Rn @ np.array([0.1, -0.1, -3.0]) + pn
            tracks = [F + j for j in range(DECOYS)]
            d["free"] = list(d.get("free", [])) + [F + MOVER]
            d["obs_track"] = list(d["obs_track"]) + tracks
            d["obs_uv"] = np.vstack([np.asarray(d["obs_uv"], dtype=np.float64).reshape(-1, 4), np.zeros((DECOYS, 4))])
            d["pf_track"] = list(d.get("pf_track", [])) + sorted(seed)
            d["pf"] = np.vstack([np.asarray(d.get("pf", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)] + [seed[t].reshape(1, 3) for t in sorted(seed)])
            seed_upd = {}
            if f == POISON_FRAME:
                seed_upd[REAL] = R0 @ np.array([0.1, 0.1, -3.0]) + p0
                fr["upd"] = dict(fr["upd"], pf_track=[REAL], pf=seed_upd[REAL].reshape(1, 3))
            fr["decoy"] = dict(seed=seed, seed_upd=seed_upd, free=[F + MOVER], cls=cls, leave_pos=leave_pos)
    return cases


class Book:
    """the integers a host keeps of one filter for the maintenance call: the table's slots and window list (closed_loop_tail._Ints: the
    stage takes the lowest free slot), the anchors of the decoys and of track REAL, and per track the clones (table slots) that hold
    an observation of it: obs - what the device's mask holds, by window position"""

    def __init__(self, c):
        from ingvio_amd.closed_loop_tail import _Ints
        self.ints, self.an, self.F, self.stages = _Ints(c["table"]), Anchors(), c["decoy_F"], 0
        self.tracked = [REAL] + [self.F + j for j in range(DECOYS)]
        self.obs, self.appended = {t: [] for t in self.tracked}, []
        self.columns, self.left = list(self.ints.clones), []             # the store's columns: the window of the last stage; clones gone since

    def mask(self, t):
        """the store's mask of track t as the bookkeeping has it: the store's columns are the window positions of the LAST STAGE - a
        clone that left since keeps its column, and its observations, until the next stage's drop list closes the rows up"""
        return sum(1 << self.columns.index(s) for s in self.obs[t])

    def assign(self):
        """what the stage of a camera frame does to the bookkeeping: the keeper and the restarted track hang on the oldest clone, the
        mover is released and restarted on the window's second clone"""
        cl = self.ints.clones
        self.an.slot.setdefault(REAL, cl[-1])                            # (a new or restarted track: the clone of its first observation)
        self.an.slot.setdefault(self.F + KEEPER, cl[0])
        self.an.slot.setdefault(self.F + INVALID, cl[0])
        self.an.slot[self.F + MOVER] = cl[1]

    def staged(self):
        self.ints.append_clone()
        self.stages += 1
        self.obs = {t: [s for s in o if s not in self.left] for t, o in self.obs.items()}      # the delta's drop list
        self.columns, self.left = list(self.ints.clones), []
        self.appended.append(self.ints.clones[-1])
        self.obs[self.F + MOVER] = []                                    # released by every frame's delta
        for t in self.tracked:                                           # every frame observes every tracked track
            self.obs[t].append(self.ints.clones[-1])
        self.assign()

    def leave(self, fr):
        """the clones at the frame's leave positions go; -> their table slots"""
        gone = [self.ints.clones[q] for q in fr["decoy"]["leave_pos"]]
        for sl in gone:
            self.ints.kind[sl], self.ints.anchor[sl] = None, -1
        self.ints.clones = [s for s in self.ints.clones if s not in gone]
        self.left += gone
        return gone

    def words(self, leaving):
        return maintain_words(self.ints.clones, self.an, leaving)

    def done(self, tracks, verdicts, new_slot, stages_then):
        """the verdicts of a call issued when `stages_then` stages had been counted and new_slot was the newest clone; verdicts that arrive
        behind a later stage (the free-running form) are followed by that stage's bookkeeping again: an erased track that was observed
        since is a restarted one"""
        for t in apply_verdicts(self.an, tracks, verdicts, new_slot):   # erased: mask = the observations since, anchor = the first of them
            self.obs[t] = [s for s in self.appended[stages_then:] if s in self.ints.clones]
            if t == REAL and self.obs[t]:
                self.an.slot[t] = self.obs[t][0]
        if self.stages != stages_then:
            self.obs[self.F + MOVER] = self.obs[self.F + MOVER][-1:]     # (the later stage released the mover, whatever the verdict)
            self.assign()


def decoy_points(store, fr):
    """a frame's delta on the host model's points: released tracks lose theirs, seeded ones get one"""
    for t in fr["decoy"]["free"]:
        store.points.pop(t, None)
    for t, p in list(fr["decoy"]["seed"].items()) + list(fr["decoy"]["seed_upd"].items()):
        store.points[t] = np.array(p, dtype=np.float64)


def decoy_form(cases, books, out, free_running=False):
    """the MaintainForm of the decoy loops over closed_loop_update.two_update_entries: behind every camera frame's second update the clones
    at its leave positions are taken off the bookkeeping (mode "sw": the update's run has marginalised it; mode "kf": one
    ingvio_nominal_tail drops them here) and one call lists the filter's decoys; out[f] = per filter (tracks, verdicts, depths)"""
    mode = cases[0]["decoy_mode"]

    def lists(loop, i):
        e = loop.frames[i]
        if not isinstance(e, UpdateEntry):
            return None
        blocks, ctxt = [], []
        gones = [bk.leave(c["frames"][e.f]) for c, bk in zip(cases, books)]
        if mode == "kf" and any(gones):                                  # the key-frame cadence: the clones leave through the tail, in front of the call
            loop.ctx.nominal_tail(0, [dict(marg_slot=g) for g in gones])
        for bk, gone in zip(books, gones):
            tracks, words = bk.words(gone)
            blocks.append(dict(tracks=words))
            ctxt.append((tracks, bk.ints.clones[-1], bk.stages))
        lists.pending[i] = ctxt
        return blocks
    lists.pending = {}

    def done(loop, i, res):
        per = []
        for bk, (tracks, new_slot, stages), r in zip(books, lists.pending.pop(i), res):
            bk.done(tracks, [int(v) for v in r["verdict"]], new_slot, stages)
            per.append((tracks, [int(v) for v in r["verdict"]], r["depth"]))
        out[loop.frames[i].f] = per

    class DecoyForm(MaintainForm):
        def staged(self, loop, i):
            for bk in books:
                bk.staged()
    return DecoyForm(lists, done, free_running, MOVE_MIN_DEPTH[mode])


# ---- the device loop's form ----------------------------------------------------------------------------------------------------------
class MaintainForm(Form):
    """ingvio_tracks_maintain behind every camera frame's last run, with `lists(loop, i)` -> per filter a dict(tracks=[words], lm_slot=[..])
    built from the host's integer bookkeeping (None: no call behind entry i), and `done(loop, i, results)` taking the verdicts.
    free_running=False: the synchronous call as a late form - fetch_begin(i); maintain(i); stage(i + 1); run(i + 1); fetch_end(i).
    free_running=True: _begin right behind run(i), _end right behind run(i + 1) (behind the last entry: at once) - the stage of entry
    i + 1 is built without entry i's verdicts (the contract in include/ingvio_hip.h)."""

    def __init__(self, lists, done, free_running=False, move_min_depth=0.0, min_depth=MIN_DEPTH):
        self.lists, self.done, self.free = lists, done, free_running
        self.late = not free_running
        self.move_min_depth, self.min_depth = move_min_depth, min_depth
        self.open = None                                                 # the entry whose _begin has not been ended

    def _end(self, loop):
        if self.open is not None:
            i, self.open = self.open, None
            self.done(loop, i, loop.ctx.tracks_maintain_end())

    def ran(self, loop, i):
        if not self.free:
            return
        self._end(loop)                                                  # entry i - 1's verdicts, behind run(i)
        blocks = self.lists(loop, i)
        if blocks is not None:
            loop.ctx.tracks_maintain_begin(0, blocks, self.move_min_depth, self.min_depth)
            self.open = i
            if i + 1 == len(loop.frames):
                self._end(loop)

    def after(self, loop, i):
        if self.free:
            return
        blocks = self.lists(loop, i)
        if blocks is not None:
            self.done(loop, i, loop.ctx.tracks_maintain(0, blocks, self.move_min_depth, self.min_depth))


# ---- a loop that never calls the maintenance exports (recorded on the library before them) -----------------------------------------
def non_user_arrays(B=3, nfr=4, F=24):
    """the pipelined two-update loop with triangulating first updates on a fresh context, nothing of this module called: every result
    of every entry, the final covariances, tables and track stores as one dict of arrays.  tests/golden/maintain_non_user_loop.npz holds
    them as the library computed them before k_tracks_apply and k_tracks_store_points kept the point flag and TrackStore grew
    (`python -m ingvio_amd.closed_loop_maintain record <path>` wrote it); the results must stay bit-identical."""
    from ingvio_amd import capi
    from ingvio_amd.closed_loop_update import device_loop_update, make_update_loop
    cases = make_update_loop(B, nfr, F, first_tri=True, windows=(5, 6, 7))
    n_max = max(c["P"].shape[0] for c in cases) + 6
    ctx = capi.Context(batch=B, n_max=((n_max + 15) // 16) * 16, c_max=12, f_max=F, m_max=64)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c["P"])
    ctx.tracks_create(F)
    ctx.nominal_create(48)
    ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    out = {}
    for f, (r1, r2) in enumerate(device_loop_update(ctx, cases, list(range(nfr)), True)):
        n1, n2 = len(cases[0]["frames"][f]["delta"]["feat_track"]), len(cases[0]["frames"][f]["upd"]["feat_track"])
        for u, (r, n) in enumerate(((r1, n1), (r2, n2))):
            for name, a in zip(("dx", "accept", "rows", "pf", "tri_ok"), r):
                out["f%d_u%d_%s" % (f, u, name)] = np.array(a[:, :n] if name in ("accept", "pf", "tri_ok") else a)
    for b, nom in enumerate(ctx.nominal_get()):
        out["P%d" % b], out["val%d" % b], out["idx%d" % b] = ctx.cov_get(b), np.array(nom["val"]), np.array(nom["idx"])
        mask, _, pf = ctx.debug_tracks_read(b)
        out["mask%d" % b], out["store_pf%d" % b] = mask, pf
    ctx.close()
    return out


if __name__ == "__main__":
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        np.savez_compressed(sys.argv[2], **non_user_arrays())
