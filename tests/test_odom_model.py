"""The host model of the odometry record (ingvio_amd/odom.py), pinned without a GPU: its Jacobians against central differences of the
oracle's SE2(3) retraction, and the gather of cov_err with its status bits on hand-made tables."""
import numpy as np
import pytest

from ingvio_amd import odom

H = 1e-5


def rot(w):
    th = np.linalg.norm(w)
    K = odom.skew(w / th)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * K @ K


def rot_log(M):
    """the world-axis rotation vector of a rotation close to the identity"""
    w = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])      # sin(th) * axis
    s = np.linalg.norm(w)
    return w if s < 1e-12 else w * (np.arcsin(s) / s)


def poses():
    rng = np.random.default_rng(20251)
    out = []
    for i in range(20):
        angle = 10.0 ** rng.uniform(-3.0, np.log10(3.0))                  # 1e-3 .. 3 rad
        axis = rng.normal(size=3)
        scale_p, scale_v = 10.0 ** rng.uniform(0.0, 3.0), 10.0 ** rng.uniform(0.0, 3.0)      # |p|, |v| up to 1e3
        p, v = rng.normal(size=3), rng.normal(size=3)
        out.append((rot(angle * axis / np.linalg.norm(axis)), scale_p * p / np.linalg.norm(p), scale_v * v / np.linalg.norm(v)))
    out[0] = (out[0][0], 1e3 * np.array([0.6, -0.8, 0.0]), 1e3 * np.array([0.0, 0.6, 0.8]))      # the largest magnitudes
    return out


@pytest.mark.parametrize("case", range(20))
def test_jacobians_against_the_oracle_retraction(case):
    """J_p, J_v against central differences (h = 1e-5) of oracle.se23_update, taken on the Euclidean p' - p, v' - v and on the world-axis
    rotation log(R' R^T).  Tolerance 1e-8 * max(1, |p|, |v|): truncation h^2 |p| / 6 ~ 2e-11 |p| and rounding eps |p| / h ~ 2e-11 |p|
    lie a factor 100 below it, a wrong sign or a missing term far above."""
    from oracle import oracle as orc
    R, p, v = poses()[case]
    Jp, Jv = odom.jacobians(p, v)
    num_p, num_v = np.zeros((6, 9)), np.zeros((3, 9))
    for k in range(9):
        d = np.zeros(9)
        d[k] = H
        Rp, pp, vp = orc.se23_update(R, p, v, d)
        Rm, pm, vm = orc.se23_update(R, p, v, -d)
        num_p[0:3, k] = ((np.asarray(pp) - p) - (np.asarray(pm) - p)) / (2 * H)
        num_p[3:6, k] = (rot_log(np.asarray(Rp).reshape(3, 3) @ R.T) - rot_log(np.asarray(Rm).reshape(3, 3) @ R.T)) / (2 * H)
        num_v[:, k] = ((np.asarray(vp) - v) - (np.asarray(vm) - v)) / (2 * H)
    tol = 1e-8 * max(1.0, np.linalg.norm(p), np.linalg.norm(v))
    print("case %d: |p| %.3g |v| %.3g  max err J_p %.3g J_v %.3g  tol %.3g" % (case, np.linalg.norm(p), np.linalg.norm(v),
                                                                            np.abs(num_p - Jp).max(), np.abs(num_v - Jv).max(), tol))
    assert np.abs(num_p - Jp).max() <= tol
    assert np.abs(num_v - Jv).max() <= tol


def table(layout, n_extra=0):
    """layout: (kind, idx) per slot in order ext, pose, bg, ba, then anything else; values are distinct numbers"""
    kind = [k for k, _ in layout]
    idx = [i for _, i in layout]
    val = np.arange(15.0 * len(layout)).reshape(len(layout), 15) + 0.25
    return dict(kind=kind, idx=idx, anchor=[-1] * len(layout), val=val, clone_var=[], v_ext=0, v_pose=1, v_bg=2, v_ba=3, gravity=np.zeros(3))


def spd(n, seed):
    A = np.random.default_rng(seed).normal(size=(n, n))
    return A @ A.T + n * np.eye(n)


def test_cov_err_is_the_plain_sub_block_for_permuted_idx():
    # extrinsics first, the pose at 6, a scalar, bg behind it, a clone in between, ba last
    nom = table([(odom.SE3, 0), (odom.SE23, 6), (odom.VEC3, 16), (odom.VEC3, 25), (odom.SCALAR, 15), (odom.SE3, 19)])
    n = 28
    P = spd(n, 1)
    r = odom.odom_model(nom, P, n, gnss_slots=[-1, 4, -1, -1, -1, -1])
    cols = list(range(6, 15)) + [16, 17, 18] + [25, 26, 27]
    assert np.array_equal(r["cov_err"], P[np.ix_(cols, cols)])
    assert r["status"] == 0 and r["n"] == n
    assert r["gnss_mask"] == 2 and r["gnss"][1] == nom["val"][4, 9] and not r["gnss"][[0, 2, 3, 4, 5]].any()
    assert np.array_equal(r["p"], nom["val"][1, 9:12]) and np.array_equal(r["R_c2i"], nom["val"][0, 0:9].reshape(3, 3))
    Jp, Jv = odom.jacobians(r["p"], r["v"])
    assert np.allclose(r["cov_pose"], Jp @ P[6:15, 6:15] @ Jp.T, rtol=1e-13) and np.array_equal(r["cov_pose"], r["cov_pose"].T)
    assert np.allclose(r["cov_vel"], Jv @ P[6:15, 6:15] @ Jv.T, rtol=1e-13) and np.array_equal(r["cov_vel"], r["cov_vel"].T)
    assert r["diag_min"] == np.diagonal(P).min() and r["diag_max"] == np.diagonal(P).max()
    # the position block of cov_pose is Var(dp - [p]x dth), the orientation block is the d_theta block itself
    assert np.array_equal(r["cov_pose"][3:6, 3:6], np.triu(P[6:9, 6:9]) + np.triu(P[6:9, 6:9], 1).T)


@pytest.mark.parametrize("how", ["slot", "beyond_n"])
def test_absent_variable_gives_bit_4_and_zero_rows(how):
    nom = table([(odom.SE3, 15), (odom.SE23, 0), (odom.VEC3, 9), (odom.VEC3, 12)])
    n = 21
    if how == "slot":
        nom["v_bg"] = -1
    else:
        nom["idx"][2] = 19                                               # idx + 3 > n
    P = spd(n, 2)
    r = odom.odom_model(nom, P, n)
    assert r["status"] == odom.ABSENT
    assert not r["bg"].any() and not r["cov_err"][9:12, :].any() and not r["cov_err"][:, 9:12].any()
    keep = list(range(9)) + [12, 13, 14]
    assert np.array_equal(r["cov_err"][np.ix_(keep, keep)], P[np.ix_(keep, keep)])      # the rest of the record is valid
    assert np.array_equal(r["ba"], nom["val"][3, 9:12])


def test_masks_and_status_bits():
    nom = table([(odom.SE3, 15), (odom.SE23, 0), (odom.VEC3, 9), (odom.VEC3, 12)])
    n = 24
    P = spd(n, 3)
    P[22, 22] = -1.0                                                     # outside the 15 x 15 block
    r = odom.odom_model(nom, P, n)
    assert r["status"] == odom.NEG_DIAG and r["diag_min"] == -1.0
    r = odom.odom_model(nom, P, n, what=odom.COV)
    assert r["status"] == 0 and r["diag_min"] == 0.0 and r["diag_max"] == 0.0 and not r["cov_pose"].any() and r["cov_err"].any()
    r = odom.odom_model(nom, P, n, what=0)
    assert not r["cov_err"].any() and r["p"].any()
    r = odom.odom_model(nom, P, n, what=odom.EUCL)                        # implies COV
    assert r["cov_err"].any() and r["cov_pose"].any() and r["cov_vel"].any()
    P[3, 4] = np.inf
    assert odom.odom_model(nom, P, n, what=odom.COV)["status"] == odom.NONFINITE
