"""Host model of the device-resident track store, written from the contract in include/ingvio_hip.h (ingvio_track_frame: "the delta on
the store, applied in this order: window slots that leave (the tracks' rows close up), tracks that were erased, the new clone's column
(one measurement per observed track), points that changed") and not from the kernels.

Per filter the model holds   obs: track -> {window slot: uv [4]}   and   points: track -> pf [3]   and applies a delta with dictionary
operations only; bits and the device's array layout appear in mask() / uv() / pf() / gather(), which exist for the comparison with
ingvio_debug_tracks_read and ingvio_debug_staged_frame.  Everything is integers and copied doubles, so the comparison is bit for bit."""
import numpy as np


def ragged_observations(rng, F, C, kmin=4):
    """per feature a sorted set of kmin .. C window slots (every feature its own observation set)"""
    out = []
    for _ in range(F):
        k = int(rng.integers(kmin, C + 1))
        out.append(np.sort(rng.choice(C, size=k, replace=False)))
    return out


class TrackStoreModel:
    def __init__(self, t_max, c_max):
        self.t_max, self.c_max = int(t_max), int(c_max)
        self.obs = {}
        self.points = {}

    def apply(self, d):
        """d: a delta as capi.make_track_frame takes it (drop, free, append, obs_track, obs_uv, pf_track, pf); other keys are ignored"""
        drop = [int(s) for s in d.get("drop", [])]
        if drop:                                                         # 1. slots that leave: the remaining ones renumber downward
            for t in list(self.obs):
                self.obs[t] = {s - len([g for g in drop if g < s]): m for s, m in self.obs[t].items() if s not in drop}
        for t in d.get("free", []):                                      # 2. erased tracks: their observations are forgotten
            self.obs[int(t)] = {}
        slot = int(d.get("append", -1))
        tr = [int(t) for t in d.get("obs_track", [])]
        if tr:                                                           # 3. the new clone's column
            assert 0 <= slot < self.c_max
            uv = np.asarray(d["obs_uv"], dtype=np.float64).reshape(len(tr), 4)
            for t, m in zip(tr, uv):
                self.obs.setdefault(t, {})[slot] = m.copy()
        pt = [int(t) for t in d.get("pf_track", [])]
        if pt:                                                           # 4. points that changed
            pf = np.asarray(d["pf"], dtype=np.float64).reshape(len(pt), 3)
            for t, p in zip(pt, pf):
                self.points[t] = p.copy()

    # ---- the device layout, for the comparison only ----
    def mask(self):
        m = np.zeros(self.t_max, dtype=np.uint64)
        for t, row in self.obs.items():
            m[t] = np.uint64(sum(2 ** s for s in row))
        return m

    def uv(self):
        u = np.zeros((self.t_max, self.c_max, 4))
        for t, row in self.obs.items():
            for s, x in row.items():
                u[t, s] = x
        return u

    def pf(self):
        p = np.zeros((self.t_max, 3))
        for t, x in self.points.items():
            p[t] = x
        return p

    def gather(self, feat_track, feat_anchor, feat_dof, feat_sel=None, f_max=None):
        """the arrays of the staged frame: anchor / dof / pf [F], obs_mask [f_max] (zero behind the F features), uv [F][c_max][4]
        and have [F][c_max]: the stored observations of each feature's track (where uv is defined)"""
        F = len(feat_track)
        f_max = F if f_max is None else f_max
        out = dict(n_feat=F, anchor=np.array(feat_anchor, dtype=np.int32).reshape(F), dof=np.array(feat_dof, dtype=np.int32).reshape(F),
                   obs_mask=np.zeros(f_max, dtype=np.uint64), pf=np.zeros((F, 3)), uv=np.zeros((F, self.c_max, 4)),
                   have=np.zeros((F, self.c_max), dtype=bool))
        for j, t in enumerate(int(t) for t in feat_track):
            row = self.obs.get(t, {})
            bits = sum(2 ** s for s in row)
            if feat_sel is not None:
                bits &= int(feat_sel[j])
            out["obs_mask"][j] = np.uint64(bits)
            out["pf"][j] = self.points.get(t, np.zeros(3))
            for s, x in row.items():
                out["uv"][j, s] = x; out["have"][j, s] = True
        return out


def bits_of(mask, c_max):
    """[n] uint64 -> [n][c_max] bool"""
    return ((np.asarray(mask, dtype=np.uint64)[:, None] >> np.arange(c_max, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def same_bits(a, b):
    """bit-equal doubles (no tolerance, -0.0 != 0.0)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_store_equal(read, want, c_max, what=""):
    """read / want: (mask, uv, pf) of one filter.  Masks and points equal everywhere; measurements bit-equal where the mask bit is set
    (closing a row up leaves stale values in the vacated columns, which no kernel reads)."""
    assert np.array_equal(read[0], want[0]), (what, "mask", np.flatnonzero(read[0] != want[0])[:8])
    have = bits_of(want[0], c_max)
    assert same_bits(read[1][have], want[1][have]), (what, "uv")
    assert same_bits(read[2], want[2]), (what, "pf")


def assert_frame_equal(got, want, c_max, what="", have=None):
    """got: Context.debug_staged_frame; want: another one, or TrackStoreModel.gather's dict (+ n_clones, clone_idx, clone_R, clone_p when
    the clone table is compared).  Counts, anchors, dofs, masks, points and the clone table equal; the mask rows behind the frame's
    features zero; measurements bit-equal where `have` (default: the staged obs_mask) is set."""
    F = int(want["n_feat"])
    assert got["n_feat"] == F, (what, got["n_feat"], F)
    fm = len(got["obs_mask"])
    wm = np.zeros(fm, dtype=np.uint64); wm[:len(want["obs_mask"])] = want["obs_mask"]
    assert np.array_equal(got["obs_mask"][:F], wm[:F]), (what, "obs_mask")
    assert not got["obs_mask"][F:].any() and not wm[F:].any(), (what, "mask rows behind the frame's features")
    for key in ("anchor", "dof"):
        assert np.array_equal(got[key][:F], np.asarray(want[key])[:F]), (what, key)
    assert same_bits(got["pf"][:F], np.asarray(want["pf"])[:F]), (what, "pf")
    if "n_clones" in want:
        n = int(want["n_clones"])
        assert got["n_clones"] == n, (what, "n_clones")
        assert np.array_equal(got["clone_idx"][:n], np.asarray(want["clone_idx"])[:n]), (what, "clone_idx")
        assert same_bits(got["clone_R"][:n].reshape(n, 9), np.asarray(want["clone_R"], dtype=np.float64).reshape(-1, 9)[:n]), (what, "clone_R")
        assert same_bits(got["clone_p"][:n].reshape(n, 3), np.asarray(want["clone_p"], dtype=np.float64).reshape(-1, 3)[:n]), (what, "clone_p")
    if have is None:
        have = bits_of(wm[:F], c_max)
    if F == 0:
        return
    wuv = np.asarray(want["uv"], dtype=np.float64)[:F].reshape(F, -1, 4)
    have = have[:, :wuv.shape[1]]
    assert not bits_of(wm[:F], c_max)[:, wuv.shape[1]:].any()
    assert same_bits(got["uv"][:F, :wuv.shape[1]][have], wuv[have]), (what, "uv")
