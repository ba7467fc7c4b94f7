"""Host model of the odometry record (ingvio_odom_begin / _end, kernels_odom.hip): numpy only, built from the table layout
that ingvio_nominal_get and closed_loop.HostTable.as_dict() share and from the full covariance.  odom_model() returns the dict that
capi.Context.odom_end() returns; the GPU tests compare the two, tests/test_odom_model.py pins the Jacobians against the oracle."""
import numpy as np

COV, EUCL, DIAG = 1, 2, 4
ALL = COV | EUCL | DIAG
NONFINITE, NEG_DIAG, ABSENT = 1, 2, 4
SE23, SE3, VEC3, SCALAR = 0, 1, 2, 3


def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def jacobians(p, v):
    """(J_p [6][9], J_v [3][9]) from the error coordinates (d_theta, d_p, d_v) of the extended pose to the Euclidean errors (position,
    orientation) and velocity in the world frame.  The retraction is R' = Gamma0(dth) R, p' = Gamma0(dth) p + Gamma1(dth) dp, v alike
    (PoseState.cpp:174-186), so to first order delta p = dp - [p]x dth, delta v = dv - [v]x dth; dth is a world-axis rotation already."""
    Jp, Jv = np.zeros((6, 9)), np.zeros((3, 9))
    Jp[0:3, 0:3] = -skew(p); Jp[0:3, 3:6] = np.eye(3); Jp[3:6, 0:3] = np.eye(3)
    Jv[0:3, 0:3] = -skew(v); Jv[0:3, 6:9] = np.eye(3)
    return Jp, Jv


def odom_model(nom, P, n, gnss_slots=None, what=ALL):
    """nom: one filter's table (kind, idx, val [n_var][15], v_ext, v_pose, v_bg, v_ba); P: its covariance (at least n x n); gnss_slots [6]:
    the table slots of ingvio_nominal_set_gnss (None: none registered)"""
    kind, idx, val = np.asarray(nom["kind"]), np.asarray(nom["idx"]), np.asarray(nom["val"], dtype=np.float64).reshape(-1, 15)
    P = np.asarray(P, dtype=np.float64)
    if what & EUCL:
        what |= COV
    status = 0

    def variable(slot, need, size):
        """-> (idx, value [15]) of the variable, (-1, zeros) where it is absent"""
        nonlocal status
        if 0 <= slot < len(kind) and kind[slot] == need and idx[slot] >= 0 and idx[slot] + size <= n:
            return int(idx[slot]), val[slot]
        status |= ABSENT
        return -1, np.zeros(15)
    i_pose, x_pose = variable(nom["v_pose"], SE23, 9)
    i_bg, x_bg = variable(nom["v_bg"], VEC3, 3)
    i_ba, x_ba = variable(nom["v_ba"], VEC3, 3)
    _, x_ext = variable(nom["v_ext"], SE3, 6)
    out = dict(n=int(n), R_i2w=x_pose[0:9].reshape(3, 3).copy(), p=x_pose[9:12].copy(), v=x_pose[12:15].copy(), bg=x_bg[9:12].copy(),
               ba=x_ba[9:12].copy(), R_c2i=x_ext[0:9].reshape(3, 3).copy(), p_c2i=x_ext[9:12].copy(), gnss=np.zeros(6), gnss_mask=0,
               cov_err=np.zeros((15, 15)), cov_pose=np.zeros((6, 6)), cov_vel=np.zeros((3, 3)), diag_min=0.0, diag_max=0.0)
    for s in range(6):
        slot = -1 if gnss_slots is None else int(gnss_slots[s])
        if 0 <= slot < len(kind) and kind[slot] == SCALAR:
            out["gnss"][s] = val[slot, 9]
            out["gnss_mask"] |= 1 << s
    if what & COV:
        cols = np.concatenate([np.arange(i, i + m) if i >= 0 else np.full(m, -1) for i, m in ((i_pose, 9), (i_bg, 3), (i_ba, 3))])
        have = cols >= 0
        out["cov_err"][np.ix_(have, have)] = P[np.ix_(cols[have], cols[have])]
    if what & EUCL:
        S = out["cov_err"][0:9, 0:9]
        Jp, Jv = jacobians(out["p"], out["v"])
        for key, J in (("cov_pose", Jp), ("cov_vel", Jv)):
            C = J @ S @ J.T
            out[key] = np.triu(C) + np.triu(C, 1).T                       # the upper triangle mirrored, as the kernel does
    if what & DIAG and n > 0:
        d = np.diagonal(P)[:n]
        out["diag_min"], out["diag_max"] = float(np.fmin.reduce(d)), float(np.fmax.reduce(d))
        if out["diag_min"] < 0.0:
            status |= NEG_DIAG
    values = np.concatenate([out[k].ravel() for k in ("R_i2w", "p", "v", "bg", "ba", "R_c2i", "p_c2i", "gnss")])
    if not (np.all(np.isfinite(values)) and np.all(np.isfinite(out["cov_err"]))):
        status |= NONFINITE
    out["status"] = status
    return out


def eucl_bound(rec):
    """entrywise |J| |S| |J|^T of a record's two congruences: the scale of the dot-product rounding bound the tests use"""
    S = np.abs(rec["cov_err"][0:9, 0:9])
    Jp, Jv = jacobians(rec["p"], rec["v"])
    return np.abs(Jp) @ S @ np.abs(Jp).T, np.abs(Jv) @ S @ np.abs(Jv).T
