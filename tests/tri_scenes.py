"""Inputs for the triangulation tests (k_triangulate, ingvio_amd/csrc/kernels_tri.hip): scenes, observation-mask edge cases, and the
two oracle-only judgements the GPU tests lean on - which features sit on a branch boundary ("marginal") and which gate rejected a
feature.  CPU only: nothing here touches a device, so tests/test_tri_scenes.py can prove that the inputs bite before anything is run
on one, and tests/test_gpu_triangulation_classes.py asserts the same counts through the same functions.

A scene is a frame dict as Context.triangulate / msckf_update_tri take it.  Scenes and oracle results are cached per process and must
be treated as read-only; derive a variant with dict(frame) and fresh arrays."""
import collections
import functools

import numpy as np

from ingvio_amd import synth
from oracle import oracle as orc

TOL = 5e-7                      # the project's triangulation tolerance (tests/test_triangulation.py): relative, max(1, |pf|) scaled
N_EDGE = 8                      # features 0..7 of a scene with edges=True carry the shaped masks below
EDGE_NAMES = ("four", "five", "full", "low", "high", "no_newest", "dirty", "dirty_twin")


def _bits(slots):
    m = 0
    for s in slots:
        m |= 1 << int(s)
    return m


def n_obs(mask, C, stereo):
    """mono-equivalent observations of a mask in a window of C clones"""
    return (2 if stereo else 1) * bin(int(mask) & ((1 << C) - 1)).count("1")


# ---- mask shapers: each returns the mask of ONE feature in a window of C clones -------------------------------------------------
def mask_exactly_four(C, stereo):
    """4 mono-equivalent observations (mono: 4 clones, stereo: 2): one too few, Triangulator.cpp:183-187 - must fail"""
    k = 2 if stereo else 4
    return _bits(np.linspace(0, C - 1, k).round().astype(int))


def mask_just_enough(C, stereo):
    """5 mono observations / 6 from 3 stereo clones: the first count that passes the test"""
    k = 3 if stereo else 5
    return _bits(np.linspace(0, C - 1, k).round().astype(int))


def mask_full(C):
    """every clone observes: with C == c_max at 12 / 24 (4 lanes), 32 (16 lanes) a lane's register share is exactly full"""
    return (1 << C) - 1


def mask_lowest(C, k):
    return (1 << min(k, C)) - 1


def mask_highest(C, k):
    return mask_full(C) & ~((1 << max(C - k, 0)) - 1)


def mask_without_newest(C):
    """s_last < C - 1: the frame of the iteration is not the window's newest clone"""
    return mask_full(C) & ~(1 << (C - 1))


def mask_dirty(mask, C):
    """bits at and above C set: the staging and the kernel mask them off, the result is the clean mask's"""
    return (int(mask) | (0xFFFFFFFFFFFFFFFF << C)) & 0xFFFFFFFFFFFFFFFF


def apply_edges(frame, C, stereo, rng):
    """overwrites the masks of features 0..N_EDGE-1 (as many as the frame holds) in the order of EDGE_NAMES; the last two share
    their measurements, one with a dirty and one with the clean mask"""
    F = len(frame["obs_mask"])
    k_side = min(C, 3 if stereo else 6)
    base = _bits(np.sort(rng.choice(C, size=min(C, 7), replace=False)))
    masks = [mask_exactly_four(C, stereo), mask_just_enough(C, stereo), mask_full(C), mask_lowest(C, k_side), mask_highest(C, k_side),
             mask_without_newest(C), mask_dirty(base, C), base]
    for j, m in enumerate(masks[:F]):
        frame["obs_mask"][j] = np.uint64(m)
    if F >= N_EDGE:
        frame["uv"][N_EDGE - 1] = frame["uv"][N_EDGE - 2]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def make_scene(seed, C, F, stereo, noise, edges=True, away=None):
    """F features seen from C clones at times 1.0 + 0.1 i on synth's trajectory (true camera poses), synth.make_features' observations
    plus Gaussian noise of `noise` (normalised coordinates), ragged masks with 1..C observing clones.  No covariance, no context.
    away = slot: that clone's camera is turned round (about its y axis) and observes nothing - an anchor there looks away from every
    point."""
    rng = np.random.default_rng([0x7A1, seed, C, F, int(stereo)])
    times = [1.0 + 0.1 * i for i in range(C)]
    poses = [synth.true_cam_pose(t) for t in times]
    _, uv, _ = synth.make_features(rng, times, F, stereo=stereo)
    uv = uv + rng.normal(0.0, noise, uv.shape)
    if not stereo:
        uv[:, :, 2:] = 0.0
    mask = np.zeros(F, dtype=np.uint64)
    for j in range(F):
        k = int(rng.integers(1, C + 1))
        mask[j] = np.uint64(_bits(rng.choice(C, size=k, replace=False)))
    Rlr, tlr = synth.t_cl2cr()
    R = np.stack([p[0] for p in poses]); p = np.stack([p[1] for p in poses])
    fr = dict(clone_idx=(21 + 6 * np.arange(C)).astype(np.int32), clone_R=R, clone_p=p, pf=np.zeros((F, 3)),
              anchor=np.zeros(F, dtype=np.int32), obs_mask=mask, uv=np.ascontiguousarray(uv), stereo=1 if stereo else 0,
              R_cl2cr=Rlr, t_cl2cr=tlr, noise=synth.PARAMS["visual_noise"], chi2_table=synth.chi2_table())
    if edges:
        apply_edges(fr, C, stereo, rng)
    if away is not None:
        fr["clone_R"][away] = R[away] @ np.diag([-1.0, 1.0, -1.0])
        fr["obs_mask"] &= ~np.uint64(1 << away)
    fr["dof"] = np.array([max(1, bin(int(m) & ((1 << C) - 1)).count("1") - 1) for m in fr["obs_mask"]], dtype=np.int32)
    return fr


@functools.lru_cache(maxsize=None)
def scene(seed, C, F, stereo, noise, edges=True, away=None):
    return make_scene(seed, C, F, stereo, noise, edges, away)


def state_size(C):
    """rows of a state that holds the C clones of a scene (clone_idx = 21 + 6 i)"""
    return 21 + 6 * C


# ---- the oracle on a feature ----------------------------------------------------------------------------------------------------
def oracle_feature(fr, j, uv=None, **params):
    return orc.triangulate(fr["clone_R"], fr["clone_p"], int(fr["obs_mask"][j]), fr["uv"][j] if uv is None else uv, bool(fr["stereo"]),
                           fr["R_cl2cr"], fr["t_cl2cr"], **params)


def close(pa, pb):
    return bool(np.linalg.norm(np.asarray(pa) - np.asarray(pb)) <= TOL * max(1.0, float(np.linalg.norm(pb))))


def marginal(fr, j, params, scales=(1, -1, 2, -2)):
    """decided by the oracle alone: its flag changes, or its point moves by more than the parity tolerance, when every measurement of
    the feature is scaled by 1 + s 2^-48 - the feature sits on a branch boundary that rounding may cross either way"""
    ok0, pf0 = oracle_feature(fr, j, **params)
    for s in scales:
        ok, pf = oracle_feature(fr, j, uv=fr["uv"][j] * (1.0 + s * 2.0 ** -48), **params)
        if ok != ok0 or not close(pf, pf0):
            return True
    return False


def attribute(fr, j, params):
    """the gate behind an oracle rejection, found by relaxing one parameter at a time (None for an accepted feature)"""
    if oracle_feature(fr, j, **params)[0]:
        return None
    p = dict(params)
    p["trans_thres"] = 0.0
    if oracle_feature(fr, j, **p)[0]:
        return "parallax"
    p["max_depth"] = 1e9; p["min_depth"] = -1e9
    if oracle_feature(fr, j, **p)[0]:
        return "depth"
    p["conv_precision"] = 1e-2; p["outer_loop_max_iter"] = 100
    if oracle_feature(fr, j, **p)[0]:
        return "convergence"
    if n_obs(fr["obs_mask"][j], len(fr["clone_R"]), fr["stereo"]) <= 4:
        return "few"
    return "other"


class Judged:
    """the oracle's verdict on every feature of a scene under one parameter set"""

    def __init__(self, fr, params):
        F = len(fr["obs_mask"])
        self.ok = np.zeros(F, dtype=bool); self.pf = np.zeros((F, 3)); self.marginal = np.zeros(F, dtype=bool); self.gate = [None] * F
        for j in range(F):
            self.ok[j], self.pf[j] = oracle_feature(fr, j, **params)
            self.marginal[j] = marginal(fr, j, params)
            self.gate[j] = attribute(fr, j, params)

    def count(self, gate):
        return sum(g == gate for g in self.gate)


@functools.lru_cache(maxsize=None)
def _judged(key, pkey):
    return Judged(scene(*key), dict(pkey))


def judged(key, params=None):
    """key: the arguments of scene(); cached"""
    return _judged(tuple(key), tuple(sorted((params or {}).items())))


def tally(keys, params=None, versus=None):
    """over several scenes: dict(features, accepted, marginal, <gate>: rejections, differs: features whose verdict under params is
    not the verdict under the parameters `versus` (None: the defaults) - flag, or point beyond the tolerance)"""
    out = dict(features=0, accepted=0, marginal=0, parallax=0, depth=0, convergence=0, few=0, other=0, differs=0)
    for key in keys:
        jd = judged(key, params); j0 = judged(key, versus)
        out["features"] += len(jd.ok); out["accepted"] += int(jd.ok.sum()); out["marginal"] += int(jd.marginal.sum())
        for g in ("parallax", "depth", "convergence", "few", "other"):
            out[g] += jd.count(g)
        out["differs"] += sum(1 for j in range(len(jd.ok)) if jd.ok[j] != j0.ok[j] or not close(jd.pf[j], j0.pf[j]))
    return out


# ---- the cases of tests/test_gpu_triangulation_classes.py -------------------------------------------------------------------------
NOISE = 3e-3
F_DEF = 96
CMAXES = (11, 12, 13, 24, 25, 32, 33, 36)


def partial_windows(c_max):
    """three windows that do not fill a c_max context (22 in a 30-clone context, 9 in a 12-clone one)"""
    return max(9, int(round(0.73 * c_max))), c_max - 1, max(9, c_max - 4)


def class_keys(stereo, c_max, full):
    """section a: the four distinct (C, F) frames that a batch of a c_max context cycles through - different C (partial windows) and
    different F per filter, F = 0 and F no multiple of 8 included"""
    if full:
        shapes = [(c_max, F_DEF), (c_max, 61), (c_max, 0), (c_max, F_DEF)]
    else:
        c1, c2, c3 = partial_windows(c_max)
        shapes = [(c1, F_DEF), (c2, 37), (c1, 0), (c3, F_DEF)]
    return [(100 + 10 * i + (0 if full else 5), C, F, stereo, NOISE) for i, (C, F) in enumerate(shapes)]


def instantiation(stereo, c_max, nb, F=F_DEF):
    """launch_triangulate's choice, restated from its rule: (stereo, NOBS, lanes per feature); NOBS 0 is the cursor path"""
    eyes = 2 if stereo else 1
    if nb * F <= 2048:
        return (stereo, 4 if eyes * c_max <= 64 else 0, 16)
    return (stereo, 6 if eyes * c_max <= 24 else 0, 4)


# section b.  A case is (name, parameters that differ from the defaults, noise, windows it runs at) and what it claims of the oracle,
# over the 576 features of a (stereo, C) pair: the gate classes with at least 10 rejections each ({C: classes}), the least number of
# features whose verdict differs from the verdict under the defaults (flag, or point beyond the tolerance: a kernel that ignored the
# parameter would get them wrong), the least accepted share.  That share is 30 % except where the parameters themselves forbid it:
# one outer iteration cannot reach conv_precision (2 of 600 features accepted); depths are drawn uniformly from 2..20 m, so max_depth 8
# keeps a third of them and the 4..8 m window 22 %, of which the too-few-observation features (up to 35 % in a mono window of 11
# clones) go off: floors 0.33 x 0.6 = 20 % and 0.22 x 0.6 -> 10 %.
# The parallax gate needs a window as short as the threshold: trans_thres 0.3 bites at 11 clones (2 m of path) only, 1.2 accepts
# nothing there and runs at 30 clones.  conv_precision 1e-10 changes a verdict only where the last step lies between 1e-10 and
# 5e-7, which the iteration's quadratic end leaves to a few features: it runs on the noisy scene, where the end is slower.
# The exit test (kernels_tri.hip, "outer >= outer_loop_max_iter && inner >= inner_loop_max_iter"; Triangulator.cpp:259-265) reads
# `inner` after it was reset to 0, so its first clause fires only with inner_loop_max_iter 0: "outer2_inner0" rejects the features
# that converge in their last allowed pass and differs from "outer2" there; "outer2_inner1" accepts them again - a kernel that did
# not reset the counter would reject them - and differs from "outer2_inner0" there.
NOISY = 2e-2
ALL_C = (11, 30)
GateCase = collections.namedtuple("GateCase", "name params noise windows gates differs share versus")


def _gc(name, params, gates=(), differs=5, share=0.30, noise=NOISE, windows=ALL_C, gates_at=ALL_C, versus=None):
    g = {C: ("few",) + (tuple(gates) if C in gates_at else ()) for C in windows}
    return GateCase(name, params, noise, windows, g, differs, share, versus)


GATE_CASES = (
    _gc("defaults", {}, differs=0),
    _gc("trans0.3", dict(trans_thres=0.3), ("parallax",), gates_at=(11,), differs=0),
    _gc("trans0.6", dict(trans_thres=0.6), ("parallax",), differs=10),
    _gc("trans1.2", dict(trans_thres=1.2), ("parallax",), windows=(30,), differs=10),
    _gc("maxdepth8", dict(max_depth=8.0), ("depth",), differs=10, share=0.20),
    _gc("mindepth4", dict(min_depth=4.0), ("depth",), differs=10),
    _gc("depth4to8", dict(max_depth=8.0, min_depth=4.0), ("depth",), differs=10, share=0.10),
    _gc("outer2", dict(outer_loop_max_iter=2), ("convergence",), differs=10),
    _gc("outer0", dict(outer_loop_max_iter=0), ("convergence",), differs=10, share=0.0),
    _gc("inner0", dict(inner_loop_max_iter=0)),
    _gc("inner1_damp1e3", dict(inner_loop_max_iter=1, init_damping=1e3)),
    _gc("huber1e-4", dict(huber_epsilon=1e-4), ("convergence",), differs=10),
    _gc("huber10", dict(huber_epsilon=10.0)),
    _gc("damp1e-8", dict(init_damping=1e-8)),
    _gc("damp1e6", dict(init_damping=1e6), differs=10),
    _gc("conv1e-10", dict(conv_precision=1e-10), ("convergence",), noise=NOISY),
    _gc("conv1e-3", dict(conv_precision=1e-3), differs=10),
    _gc("noisy", {}, ("convergence",), noise=NOISY, differs=0),
    _gc("outer2_inner0", dict(outer_loop_max_iter=2, inner_loop_max_iter=0), ("convergence",), differs=10, share=0.0,
        versus=dict(outer_loop_max_iter=2)),
    _gc("outer2_inner1", dict(outer_loop_max_iter=2, inner_loop_max_iter=1), ("convergence",), differs=10,
        versus=dict(outer_loop_max_iter=2, inner_loop_max_iter=0)),
)
GATE_PAIRS = ((True, 11), (False, 11), (True, 30), (False, 30))
N_GATE_FRAMES = 6


def gate_keys(stereo, C, noise=NOISE):
    """section b: the six frames (576 features) of a (stereo, C) pair: a batch of 2 takes them in three calls, a batch of 24 holds
    them four times"""
    return [(200 + i, C, F_DEF, stereo, noise) for i in range(N_GATE_FRAMES)]


def assert_bites(keys, case, C):
    """the class counts a case claims, asserted on the oracle alone; returns the tally"""
    t = tally(keys, case.params, case.versus)
    for g in case.gates[C]:
        assert t[g] >= 10, (case.name, C, g, t)
    assert t["differs"] >= case.differs, (case.name, C, t)
    assert t["accepted"] >= case.share * t["features"], (case.name, C, t)
    assert t["marginal"] <= 0.01 * t["features"], (case.name, C, t)
    return t


# section c: a window whose clone AWAY looks the other way; every fourth feature is anchored there
AWAY = 5


def behind_keys(stereo):
    return [(300 + i, 11, F_DEF, stereo, NOISE, True, AWAY) for i in range(2)]


def behind_frame(key):
    fr = dict(scene(*key))
    fr["anchor"] = np.where(np.arange(len(fr["obs_mask"])) % 4 == 0, AWAY, 0).astype(np.int32)
    return fr


def anchor_depth(fr, j, pf):
    """(R_a^T (p_f - p_a)).z: the depth of a point in the (left) camera of the feature's anchor clone"""
    a = int(fr["anchor"][j])
    return float((np.asarray(fr["clone_R"][a]).reshape(3, 3).T @ (np.asarray(pf) - np.asarray(fr["clone_p"][a])))[2])


def nan_frame(fr, seed=5):
    """section e: every even feature gets a NaN in one component of one OBSERVED measurement"""
    rng = np.random.default_rng(seed)
    out = dict(fr); uv = fr["uv"].copy()
    C = len(fr["clone_R"])
    for j in range(0, len(fr["obs_mask"]), 2):
        obs = [s for s in range(C) if (int(fr["obs_mask"][j]) >> s) & 1]
        uv[j, obs[int(rng.integers(len(obs)))], int(rng.integers(4 if fr["stereo"] else 2))] = np.nan
    out["uv"] = uv
    return out
