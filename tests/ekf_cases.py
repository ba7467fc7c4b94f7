"""Cases and the 80-bit reference of the generic EKF update (ingvio_ekf_update, ingvio_ekf_update_batch, ingvio_chi2_gamma,
ingvio_chi2_gamma_multi).  No GPU here: tests/test_ekf_reference_model.py holds the float64 oracle against this reference on every
case, tests/test_gpu_ekf_routes.py holds the kernels against it.

Every input is generated from a seed derived from the case's own fields; inputs and expected values are computed once per process,
shared between the tests and handed out read-only."""
import functools
import zlib
from typing import NamedTuple

import numpy as np

LD = np.longdouble


# ---- the reference --------------------------------------------------------------------------------------------------------
def _cols(vidx, vsize):
    return np.concatenate([np.arange(i, i + s) for i, s in zip(vidx, vsize)]).astype(np.int64)


def _noise_matrix(R, m):
    R = np.asarray(R, dtype=LD)
    if R.ndim == 0 or (R.size == 1 and m != 1):
        return np.eye(m, dtype=LD) * R.reshape(())
    if R.ndim == 1:
        return np.diag(R)
    return R


def cholesky_ld(S):
    """lower Cholesky factor of S, column by column in np.longdouble (numpy's linalg has no longdouble); None when a pivot is
    not positive"""
    m = S.shape[0]
    L = np.zeros((m, m), dtype=LD)
    for j in range(m):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < m:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward_ld(L, B):
    """L^-1 B by forward substitution, row by row"""
    V = np.zeros(B.shape, dtype=LD)
    for j in range(L.shape[0]):
        V[j] = (B[j] - L[j, :j] @ V[:j]) / L[j, j]
    return V


def reference_update(P, vidx, vsize, H, res, R):
    """StateManager::ekfUpdate minus boxPlus and whitenResidual in np.longdouble (64-bit mantissa):
    PH^T = P[:, cols] H^T, S = H PH^T[cols] + R = L L^T, V = L^-1 (PH^T)^T, z = L^-1 res;
    P+ = sym(P - V^T V), dx = V^T z, gamma = z^T z.  Returns (P+, dx, gamma) rounded to float64, or None when S is not positive
    definite."""
    P = np.asarray(P, dtype=LD)
    H = np.atleast_2d(np.asarray(H, dtype=LD))
    res = np.asarray(res, dtype=LD).reshape(-1)
    m = H.shape[0]
    cols = _cols(vidx, vsize)
    PHt = P[:, cols] @ H.T                                  # n x m
    S = H @ PHt[cols] + _noise_matrix(R, m)
    S = (S + S.T) / 2
    L = cholesky_ld(S)
    if L is None:
        return None
    V = forward_ld(L, PHt.T.copy())                         # m x n
    z = forward_ld(L, res[:, None])[:, 0]
    Pn = P - V.T @ V
    Pn = (Pn + Pn.T) / 2
    return Pn.astype(np.float64), (V.T @ z).astype(np.float64), float(z @ z)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def var_order(n, nc):
    """(vidx, vsize) naming nc of n columns: the whole state as one block when nc == n, a single scalar column when nc == 1, otherwise
    up to four blocks of unequal size with a gap between any two, listed in non-ascending order"""
    if nc == n:
        return [0], [n]
    if nc == 1:
        return [n // 2], [1]
    gap = n - nc
    k = min(4, nc, gap + 1)
    base = nc // k
    sizes = [base] * k
    sizes[0] += nc - base * k
    if k > 1 and sizes[-1] > 1:                             # unequal sizes
        sizes[-1] -= 1; sizes[0] += 1
    gaps = [0] + [1] * (k - 1)
    spare = gap - (k - 1)
    gaps[0] = spare // 3                                    # the first block need not start at column 0
    if k > 1:
        gaps[1] += spare // 3
    vidx, at = [], 0
    for g, s in zip(gaps, sizes):
        at += g
        vidx.append(at)
        at += s
    assert at <= n
    order = {1: [0], 2: [1, 0], 3: [1, 2, 0], 4: [2, 0, 3, 1]}[k]
    return [vidx[i] for i in order], [sizes[i] for i in order]


def make_case(rng, n, m, vo, vs, r_kind, cond):
    """P0 = 1e-2 Q diag(logspace(0, -log10 cond)) Q^T, H ~ N(0, 1), res ~ 0.1 N(0, 1); R a scalar ("scalar"), a diagonal ("diag")
    in [0.5, 2] 1e-2 or a full SPD matrix ("full")"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    P = 1e-2 * (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T
    P = (P + P.T) / 2
    nc = int(np.sum(vs))
    H = rng.standard_normal((m, nc))
    res = 0.1 * rng.standard_normal(m)
    if r_kind == "scalar":
        R = np.float64(1e-2 * rng.uniform(0.5, 2.0))
    elif r_kind == "diag":
        R = 1e-2 * rng.uniform(0.5, 2.0, m)
    else:
        A = rng.standard_normal((m, m))
        R = 1e-2 * (A @ A.T / m + 0.5 * np.eye(m))
        R = (R + R.T) / 2
    return dict(P=P, vidx=list(vo), vsize=list(vs), H=H, res=res, R=R)


class Case(NamedTuple):
    n: int              # state size the covariance is set with
    m: int              # rows
    nc: int             # columns named by var_order
    r_kind: str         # "scalar" / "diag" / "full"
    cond: float
    marg: bool = False  # columns [21, 27) are marginalised before the update (the covariance moves to the other ping-pong half)
    tag: str = ""       # distinguishes cases of equal shape (another seed)

    @property
    def name(self):
        return "n%d-m%d-nc%d-%s%s%s" % (self.n, self.m, self.nc, self.r_kind, "-marg" if self.marg else "", "-" + self.tag if self.tag else "")


def case(n, m, nc, r_kind, marg=False, tag="", cond=None):
    """cond 1e6 up to 142 rows, 1e2 above: the reference formula itself must stay determined to a tenth of what the kernels are held
    to (tests/test_ekf_reference_model.py)"""
    if cond is None:
        cond = 1e6 if m <= 142 else 1e2
    return Case(n, m, n - 6 if (marg and nc == n) else nc, r_kind, cond, marg, tag)


MARG_IDX, MARG_SIZE = 21, 6


def _frozen(*arrs):
    for a in arrs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """dict(P: what cov_set takes, prior: what the update sees, vidx, vsize, H, res, R)"""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    n_live = c.n - MARG_SIZE if c.marg else c.n
    vo, vs = var_order(n_live, c.nc)
    d = make_case(rng, c.n, c.m, vo, vs, c.r_kind, c.cond)
    keep = np.r_[0:MARG_IDX, MARG_IDX + MARG_SIZE:c.n] if c.marg else np.arange(c.n)
    d["prior"] = np.ascontiguousarray(d["P"][np.ix_(keep, keep)])
    _frozen(*d.values())
    return d


@functools.lru_cache(maxsize=None)
def expected(c):
    """(P+, dx, gamma) of the case by the 80-bit reference"""
    d = inputs(c)
    out = reference_update(d["prior"], d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
    assert out is not None, c
    _frozen(*out)
    return out


def rel(A, B):
    return float(np.linalg.norm(np.asarray(A) - np.asarray(B)) / max(np.linalg.norm(np.asarray(B)), 1e-300))


# ---- the matrix ------------------------------------------------------------------------------------------------------------
S, D, F = "scalar", "diag", "full"

# LDS route, single call.  Context(batch=4, n_max=160, c_max=11, m_max=64): mld = 80, the single call stays on k_ekf_core up to
# m = max(m_max, 6 c_max) = 66.  (m, nc, n, r_kind); nc = 0 stands for the whole state.
_LDS = [
    (1, 1, 49, S), (1, 16, 47, D), (2, 17, 48, F), (4, 15, 63, S), (5, 33, 64, D), (15, 16, 65, F),
    (16, 16, 127, S), (16, 16, 49, D), (16, 16, 128, F), (16, 17, 129, S), (16, 17, 47, D), (16, 17, 160, F),
    (17, 16, 48, S), (17, 16, 63, D), (17, 16, 64, F), (17, 17, 65, S), (17, 17, 127, D), (17, 17, 128, F),
    (31, 15, 129, D), (32, 33, 160, F), (33, 1, 49, S), (63, 0, 47, D), (64, 33, 65, F), (65, 17, 128, S),
    (66, 0, 160, D), (66, 0, 49, F), (66, 0, 129, S), (15, 15, 160, S), (2, 0, 63, D), (4, 1, 64, F), (5, 16, 48, F),
    (64, 16, 127, D),
]
LDS_CASES = [case(n, m, nc or n, k) for (m, nc, n, k) in _LDS]

# LDS route at its capacity: a context whose single call keeps up to 144 rows on k_ekf_core (ingvio_ctx_create refuses m_max > 128;
# c_max = 24 gives max(m_max, 6 c_max) = 144).  The kernel's LDS is (m + 1)^2 8 + 4 nc + 16 dynamic bytes plus 256 static ones:
# 160 KB hold m = 141 with any nc; m = 142 does not fit with any (counting the dynamic bytes alone, 142 rows over up to 58 columns
# seemed to fit and the dispatch was refused by the hardware).
CAP_LDS_CASES = [case(160, 80, 33, D), case(160, 128, 160, F), case(160, 141, 160, F), case(160, 141, 17, S)]
CAP_DENSE_CASES = [case(160, 142, 17, S), case(160, 143, 58, D)]
CAP_EDGE = case(160, 142, 58, D)            # dense; so are the same rows with a 59th, all-zero column: the same posterior

# Dense, register-resident: one fresh Context(batch=2, n_max, c_max=3, m_max=16) per tile class (the workspace only grows, its row
# capacity is m rounded up to 32 and picks the class).  class -> (n_max, [cases in running order])
DENSE_REG = {
    4: (49, [case(49, 20, 17, S), case(49, 32, 49, D), case(49, 33, 16, F), case(49, 49, 33, S), case(49, 64, 49, D)]),
    8: (160, [case(49, 65, 49, S), case(49, 96, 33, D), case(49, 97, 17, F), case(49, 128, 49, S)]),
    12: (117, [case(117, 129, 66, D), case(117, 161, 117, F), case(117, 192, 33, S)]),
    14: (129, [case(129, 193, 129, F), case(129, 224, 66, D)]),
    16: (160, [case(129, 225, 66, S), case(129, 255, 129, D), case(129, 256, 33, F)]),
}
DENSE_REG_SMALL = case(129, 67, 66, D)      # after class 16's cases, in the same context: a small system in a large workspace

# Dense, sweep: one Context(batch=2, n_max=160, c_max=3, m_max=16), in this order
SWEEP_CASES = [case(129, 257, 66, S), case(117, 288, 117, D), case(49, 289, 33, F), case(160, 513, 66, D)]
SWEEP_SMALL = case(129, 70, 33, D)
SWEEP_MAX = case(160, 1024, 66, S)          # float64 oracle only: the 80-bit reference takes several seconds at 1024 rows
SWEEP_OVER = case(160, 1025, 66, S)         # E_CAPACITY

# second ping-pong half: ingvio_marginalize(b, [21], 6) first; route -> case
PINGPONG = {"lds": case(129, 33, 33, D, marg=True), "reg": case(129, 100, 129, F, marg=True), "sweep": case(117, 260, 66, S, marg=True)}

# a shrunken state: n = n_max first, then n = 49 into the same filter, then a dense-route update
SHRUNK_BIG, SHRUNK = case(129, 33, 33, S, tag="big"), case(49, 100, 49, D, tag="shrunk")

# batch, LDS: nb = 5 at b0 = 1 in a context of 7 (n_max=160, c_max=11, m_max=64: mld = 80, no m_max check in the batch call)
BATCH_LDS = {k: [case(47, 1, 1, k, tag="b"), case(64, 16, 17, k, tag="b"), case(65, 17, 16, k, tag="b"), case(129, 66, 33, k, tag="b"),
                 case(160, 80, 160, k, tag="b")] for k in (S, D)}

# k_ekf_core's LDS is sized by the most rows and the most columns of the whole call: each of these fits, the pair does not
BATCH_LDS_SIZING = [case(160, 141, 17, D, tag="z"), case(600, 2, 600, D, tag="z")]

# batch, dense
BATCH_MIXED = [case(117, 40, 33, D, tag="b"), case(160, 256, 66, D, tag="b"), case(129, 130, 129, D, tag="b")]      # class 16
# nb = 9, n_max = 128: (n, m, nc)
BATCH_GEMM64 = [case(n, m, nc, D, tag="g") for (n, m, nc) in
                [(100, 100, 33), (103, 104, 66), (106, 108, 106), (109, 112, 33), (112, 116, 66), (115, 120, 115), (118, 124, 33),
                 (121, 128, 66), (128, 130, 128)]]
# nb = 29, n_max = 256: live n = 48 .. 64, m = 257 .. 287
def _split_case(i):
    n = 48 + (5 * i) % 17
    return case(n, 257 + (11 * i) % 32, (17, 33, n)[i % 3], S, tag="s%d" % i)


BATCH_SPLIT = [_split_case(i) for i in range(29)]
BATCH_SPLIT_LD = (0, 7, 8, 28)              # against the 80-bit reference; the rest against the float64 oracle

# S not positive definite: route -> shape (the noise is replaced by the test)
NOT_PD = {"lds": case(65, 17, 17, S, tag="npd"), "reg": case(65, 70, 33, S, tag="npd"), "sweep": case(65, 260, 33, S, tag="npd")}

_NPD_M = {"lds": 17, "reg": 70, "sweep": 260}
# in a batch the failing filter sits between these two, which must be updated correctly: route -> noise kind -> (before, after)
NOT_PD_NEIGHBOURS = {r: {k: (case(49, m, 17, k, tag="npd-a"), case(63, m, 33, k, tag="npd-b")) for k in (S, D)} for r, m in _NPD_M.items()}


def not_pd_noise(m, kind):
    """a noise that makes S = H P H^T + R indefinite whatever the prior of these cases (H P H^T stays below 1 on the diagonal):
    "scalar" -10; "diag" / "full" 1e-2 with -5 at a late pivot, so that the factorisation fails after sound columns"""
    if kind == "scalar":
        return np.float64(-10.0)
    r = np.full(m, 1e-2)
    r[max(m - 3, 0)] = -5.0
    return r if kind == "diag" else np.diag(r)


# gates.  (m, nc, n, r_kind) in the LDS context; nc = 0: the whole state
_GATE = [(1, 1, 65, S), (1, 45, 65, D), (2, 16, 65, F), (15, 17, 65, S), (16, 16, 65, D), (16, 17, 160, F), (17, 16, 65, F),
         (17, 17, 65, S), (33, 45, 65, D), (33, 1, 65, F), (64, 45, 160, S), (64, 16, 65, D), (64, 17, 65, F), (2, 0, 65, D), (15, 1, 65, D)]
GATE_CASES = [case(n, m, nc or n, k, tag="gate") for (m, nc, n, k) in _GATE]
GATE_FIT = case(160, 128, 19, D, tag="gate")        # 8 (nc m + (m + 1)^2) = 152584 <= 150 KB = 153600; nc = 20 gives 153608


def gate_multi_blocks(P, nblk=40, seed=40):
    """nblk gates of mixed (m, nc) against one prior: list of (vidx, vsize, H, res)"""
    rng = np.random.default_rng(seed)
    n = P.shape[0]
    ms = [1, 2, 3, 4, 6, 8, 15, 16, 17, 20]
    ncs = [1, 3, 9, 11, 15, 16, 17, 33, 45, n]
    out = []
    for g in range(nblk):
        m, nc = ms[g % len(ms)], ncs[(g * 7 + g // 10) % len(ncs)]
        vo, vs = var_order(n, nc)
        out.append((vo, vs, rng.standard_normal((m, nc)), 0.1 * rng.standard_normal(m)))
    return out


def reference_cases():
    """every case whose GPU tolerance is taken against the 80-bit reference"""
    out = list(LDS_CASES) + CAP_LDS_CASES + CAP_DENSE_CASES + [CAP_EDGE]
    for _, cs in DENSE_REG.values():
        out += cs
    out += [DENSE_REG_SMALL] + SWEEP_CASES + [SWEEP_SMALL] + list(PINGPONG.values()) + [SHRUNK_BIG, SHRUNK]
    for cs in BATCH_LDS.values():
        out += cs
    out += BATCH_LDS_SIZING + BATCH_MIXED + BATCH_GEMM64 + [BATCH_SPLIT[i] for i in BATCH_SPLIT_LD] + GATE_CASES + [GATE_FIT]
    for kinds in NOT_PD_NEIGHBOURS.values():
        for pair in kinds.values():
            out += pair
    return out
