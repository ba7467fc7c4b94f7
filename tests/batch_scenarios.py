"""Scenario builder of tests/test_gpu_batch_paths.py: the per-filter (prior, step, frame, info) of a batch whose filters differ in
state size, observation sets and role, built on the ORACLE's covariance so that the same inputs exist with and without a GPU
(tests/test_batch_scenarios.py checks on the CPU that every scenario is what it claims to be).

Roles of a filter inside one launch of the frame update:
  ordinary   ragged observations, random anchors, marginalises its oldest clone (the fused out-of-place write-back + flip)
  inplace    the same, marg_idx = -1: updated in place, no flip, n grows by six per step
  rejected   every feature refused (dof = 0, chi2_table[0] = 0) while the filter still marginalises: the write-back only compacts
             the prior into the other half
  empty      no observation at all; the first one of a batch marginalises, the second one does not (nothing to do at all), ..."""
import numpy as np

ROLES = ("ordinary", "inplace", "rejected", "empty")
N_GNSS = 6


def state_size(C, n_lm):
    """N at update time (after propagate + clone): 21 + GNSS scalars + landmark blocks + window"""
    return 21 + N_GNSS + 3 * n_lm + 6 * C


def ragged(frame, C, stereo, rng, selected=False):
    """Ragged observation sets and random anchors (the generators of test_window_size_classes_vs_oracle and, for the
    Selected-timestamp variant, test_twelve_clone_window_vs_oracle / test_large_window_selected_variant_and_cap)."""
    F = len(frame["dof"])
    kmin = min(C, 3 if stereo else 5)
    kend = min(C + 1, 5) if (selected and stereo and C <= 16) else C + 1
    mask = np.zeros(F, dtype=np.uint64); dof = np.zeros(F, dtype=np.int32)
    obs_of = []
    for j in range(F):
        k = int(rng.integers(kmin, max(kend, kmin + 1)))
        obs = np.sort(rng.choice(C, size=k, replace=False))
        obs_of.append(obs)
        mask[j] = np.uint64(sum(1 << int(o) for o in obs)); dof[j] = k - 1
    frame = dict(frame); frame["obs_mask"] = mask; frame["dof"] = dof
    anchor = rng.integers(0, C, size=F).astype(np.int32)
    if selected:                                         # half the anchors observe the feature themselves (quirk Q10 bites there)
        for j in range(1, F, 2):
            anchor[j] = int(obs_of[j][0])
    frame["anchor"] = anchor
    return frame


def build_filter(orc, seed, C, F, n_lm, stereo, role="ordinary", nth=0, selected=False, ld=None):
    """One filter: synth.build_case on oracle.Cov (the prior after C - 1 propagate + clone cycles), the frame made ragged, the role
    applied.  `nth`: how many filters of the same role came before it in the batch."""
    from ingvio_amd import synth
    assert role in ROLES
    ld = ld or ((state_size(C, n_lm) + 15) // 16) * 16
    flt, step, frame, info = synth.build_case(lambda P: orc.Cov(P, ld=ld), orc.imu_transition, seed=seed, F=F, C=C, n_gnss=N_GNSS,
                                              n_landmarks=n_lm, stereo=stereo)
    frame = ragged(frame, C, stereo, np.random.default_rng(20000 + seed), selected)
    step = dict(step)
    if role == "inplace" or (role == "empty" and nth % 2 == 1):
        step["marg_idx"] = -1
    if role == "rejected":
        frame["dof"] = np.zeros_like(frame["dof"])
    if role == "empty":
        frame["obs_mask"] = np.zeros_like(frame["obs_mask"])
    info = dict(info, role=role, n_lm=n_lm, C=C, F=F, stereo=stereo, flt=flt)
    assert info["N_update"] == state_size(C, n_lm)
    return flt.cov.P, step, frame, info


def uniform_desc(C, stereo, nb, F=40, lm_max=10, selected=False):
    """every filter ordinary, the landmark count cycling through 0 .. lm_max (so the state sizes differ all the same)"""
    return dict(C=C, stereo=stereo, F=F, selected=selected, roles=["ordinary"] * nb, lm=[(3 * b) % (lm_max + 1) for b in range(nb)])


def mixed_desc(C, stereo, nb, F=40, lm_max=14, grow=6, selected=False):
    """The mixed batch: filter 0 at the largest state (n_max of the context), filter 1 at the smallest (no landmark block: with
    lm_max = 14 its tile count is low enough that the second workgroup of its share of a k_info_apply launch is idle), the others
    in between; three filters of every eight take the three other roles.  A filter that does not
    marginalise keeps `grow` landmark blocks (3 `grow` states) of head room, so that consecutive steps fit the context."""
    roles, lm = [], []
    for b in range(nb):
        role = {5: "inplace", 6: "rejected", 7: "empty"}.get(b % 8, "ordinary")
        n = lm_max if b == 0 else (0 if b == 1 else (5 * b + b // 7) % (lm_max + 1))
        if role in ("inplace", "empty"):
            n = min(n, max(lm_max - grow, 0))
        roles.append(role); lm.append(n)
    return dict(C=C, stereo=stereo, F=F, selected=selected, roles=roles, lm=lm)


def build_batch(orc, seed, desc):
    """-> [(prior, step, frame, info)] of a batch; desc: dict(C, stereo, F, roles [nb], lm [nb], selected)"""
    seen = dict.fromkeys(ROLES, 0)
    out = []
    for b, (role, n_lm) in enumerate(zip(desc["roles"], desc["lm"])):
        out.append(build_filter(orc, seed + b, desc["C"], desc["F"], n_lm, desc["stereo"], role, seen[role], desc.get("selected", False)))
        seen[role] += 1
    return out


def n_max_of(cases):
    return max(c[3]["N_update"] for c in cases)


def prior_at_update(orc, case, ld):
    """the covariance the update itself acts on: the prior after the frame's propagation and clone (for ingvio_msckf_update)"""
    prior, step, frame, info = case
    oc = orc.Cov(prior, ld=ld)
    for Phi, G, dt in zip(step["Phi"], step["G"], step["dt"]):
        oc.propagate(Phi, G, dt, step["sigma"], step["enable_gnss"], step["gnss_idx"], step["sigma_cb"], step["sigma_rw"])
    oc.augment(step["R_i2w"])
    return oc.P


def oracle_steps(orc, cases, ld, steps=1, **kw):
    """`steps` consecutive orc.frame_update of every filter: [step][filter] -> (P, dx, accept, n)"""
    ocs = [orc.Cov(c[0], ld=ld) for c in cases]
    out = []
    for _ in range(steps):
        row = []
        for oc, (prior, step, frame, info) in zip(ocs, cases):
            dx, acc, gam, m = orc.frame_update(oc, step, frame, **dict(dict(max_accept=0, compress_rule=1), **kw))
            row.append((oc.P, dx, acc, oc.n))
        out.append(row)
    return out
