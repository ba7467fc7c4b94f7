"""The frame update's FULL-BATCH kernels away from the one shape the benchmark uses.

launch_factored / launch_bigwin pick the write-back and the Gram chunking by the number of filters in the launch:
  windows <= 16 clones   nb <= 64: k_apply_T_flat<NC> + k_apply_sym_flat<NC>       nb > 64: k_info_apply<NC, 1> (NC 36 / 66 / 72 / 96), which
                         also flips the ping-pong halves and shrinks n through the arrival counter flip_cnt; with an in-frame GNSS
                         stage k_post_cols<NC> + k_info_apply<NC, 1, 16>
  windows 17 .. 36       nb < 4: k_apply_T + k_apply_sym      nb >= 4: k_apply_T64b + k_apply_sym64b (fpx = ceil(nb / 8) filters per XCD)
                         T does not fit the solve workspace: k_info_apply_big
  Gram chunks            G = 512 / B (<= 16) per filter: k_chunk_sum in front of the solve where G > 1; B >= 257: one chunk
Every case here runs through the C ABI of the product library against the oracle on EVERY filter of the batch (scenarios:
tests/batch_scenarios.py, checked without a GPU by tests/test_batch_scenarios.py).  ingvio_frame_run always covers the whole
context, so the size of a frame launch is the context's batch; launches over a sub-range of a context go through
ingvio_msckf_update (the update alone, on the covariance at update time).

Tolerances are the suite's own: accept masks, rows, n and symmetry exact; windows <= 16, one step from a restored prior:
posterior 1e-11 (TIGHT), dx 1e-8; consecutive steps and windows 17 .. 36: 1e-10 / 1e-7; in-frame GNSS 1e-11 / 1e-9."""
import numpy as np
import pytest

import batch_scenarios as bs
from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-11
NB = 70                       # > 64 (the full-batch kernels), not a multiple of 8 (their grids are padded to nb8 = 72)

_cache = {}


def batch(orc, seed, desc):
    key = (seed, desc["C"], desc["stereo"], desc["F"], desc.get("selected", False), tuple(desc["roles"]), tuple(desc["lm"]))
    if key not in _cache:
        _cache[key] = bs.build_batch(orc, seed, desc)
    return _cache[key]


def make_ctx(cases, c_max=None, batch_size=None, slack=0):
    from ingvio_amd import capi
    C, F = cases[0][3]["C"], cases[0][3]["F"]
    return capi.Context(batch=batch_size or len(cases), n_max=bs.n_max_of(cases) + slack, c_max=c_max or C, f_max=F, m_max=64)


def stage(ctx, cases, **kw):
    for b, c in enumerate(cases):
        ctx.cov_set(b, c[0])
    ctx.snapshot()
    s0 = cases[0][1]
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], s0["sigma"], 1, s0["sigma_cb"], s0["sigma_rw"], **kw)


def fetch(ctx, nb):
    dx, acc, rows = ctx.frame_fetch()
    return dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b) for b in range(nb)]


def check(cases, res, want, tol_P, tol_dx, tag=""):
    """every filter of the batch against the oracle; returns the worst (posterior, dx) error"""
    dx, acc, rows, Ps = res
    worst = [0.0, 0.0]
    for b, (Pw, dxw, accw, nw) in enumerate(want):
        info = cases[b][3]
        F, C = info["F"], info["C"]
        who = (tag, b, info["role"], info["N_update"])
        assert np.array_equal(acc[b, :F], accw), (who, np.flatnonzero(acc[b, :F] != accw))
        assert Ps[b].shape[0] == nw, (who, Ps[b].shape[0], nw)
        assert rows[b] == (6 * C if accw.any() else 0), (who, rows[b])
        assert np.array_equal(Ps[b], Ps[b].T), who
        eP = rel_err(Ps[b], Pw)
        if accw.any():
            ed = rel_err(dx[b, :len(dxw)], dxw)
        else:
            assert not dx[b, :len(dxw)].any() and not dxw.any(), who
            ed = 0.0
        assert eP < tol_P and ed < tol_dx, (who, eP, ed)
        worst = [max(worst[0], eP), max(worst[1], ed)]
    print("%s: %d filters, worst posterior %.1e dx %.1e" % (tag, len(want), worst[0], worst[1]))
    return worst


def run_restored_twice(ctx, cases, want, tol_P=TIGHT, tol_dx=1e-8, tag=""):
    """frame_run(restore_prior) against the oracle, then once more (the strip-restore shortcut where every filter marginalises):
    bit-identical"""
    nb = len(cases)
    ctx.frame_run(restore_prior=True)
    r1 = fetch(ctx, nb)
    check(cases, r1, want, tol_P, tol_dx, tag)
    ctx.frame_run(restore_prior=True)
    r2 = fetch(ctx, nb)
    for a, b_ in zip(r1[:3], r2[:3]):
        assert np.array_equal(a, b_), tag
    for b in range(nb):
        assert np.array_equal(r1[3][b], r2[3][b]), (tag, b)
    return r1


# ---- windows up to 16 clones, more than 64 filters per launch -------------------------------------------------------------------
@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("C", [4, 6, 9, 11, 12, 13, 16])
def test_full_batch_window_classes_vs_oracle(orc, C, stereo):
    """k_info_apply<36 | 66 | 72 | 96, 1> with its fused flip (and k_chunk_sum: 70 filters = 7 Gram chunks per filter): 70 ragged
    filters of 0 .. 10 landmark blocks, stereo and mono, at the maximum of every apply / solve class and below it (4 -> 36, 9 -> 66,
    13 -> 96), restored prior, run twice."""
    cases = batch(orc, 100 * C + (0 if stereo else 50), bs.uniform_desc(C, stereo, NB))
    ctx = make_ctx(cases)
    want = bs.oracle_steps(orc, cases, ctx.ldp)[0]
    stage(ctx, cases)
    run_restored_twice(ctx, cases, want, tag="C=%d %s" % (C, "stereo" if stereo else "mono"))
    ctx.close()


@pytest.mark.parametrize("C,stereo", [(11, True), (11, False), (16, True), (16, False)])
def test_mixed_batch_vs_oracle(orc, C, stereo):
    """k_info_apply<66 | 96, 1> on the mixed batch: per-filter n (the arrival count of the flip, ceil(nt / 8), differs: 1 and 2), a
    filter whose second workgroup is idle, one at n_max, marg_idx = -1 (no flip, in place) next to flipping neighbours, all-rejected
    filters (!upd && fused: the prior compacted into the other half) and filters with nothing to do.  Restored prior, twice (with
    marg_idx = -1 in the batch the second restore is a full one)."""
    cases = batch(orc, 1000 * C + (0 if stereo else 500), bs.mixed_desc(C, stereo, NB))
    ctx = make_ctx(cases)
    want = bs.oracle_steps(orc, cases, ctx.ldp)[0]
    stage(ctx, cases)
    run_restored_twice(ctx, cases, want, tag="mixed C=%d %s" % (C, "stereo" if stereo else "mono"))
    ctx.close()


@pytest.mark.parametrize("C,stereo", [(11, True), (16, False)])
def test_mixed_batch_three_steps_without_restore(orc, C, stereo):
    """k_info_apply's in-kernel flip decides where the NEXT step reads: three frame_run(restore_prior=False) on the mixed batch (both
    halves; the filters that do not marginalise stay in their half and grow by six per step - the scenario leaves them head room),
    the oracle applied sequentially."""
    cases = batch(orc, 1000 * C + (0 if stereo else 500), bs.mixed_desc(C, stereo, NB))
    ctx = make_ctx(cases)
    want = bs.oracle_steps(orc, cases, ctx.ldp, steps=3)
    stage(ctx, cases)
    ctx.restore()
    for it in range(3):
        ctx.frame_run(restore_prior=False)
        check(cases, fetch(ctx, NB), want[it], 1e-10, 1e-7, "mixed C=%d step %d" % (C, it))
    ctx.close()


def test_full_batch_selected_variant_vs_oracle(orc):
    """k_info_apply<72, 1> behind the UNREDUCED solve of the Selected-timestamp variant (quirk Q10), 12 clones, mixed batch."""
    cases = batch(orc, 12000, bs.mixed_desc(12, True, NB, selected=True))
    ctx = make_ctx(cases)
    want = bs.oracle_steps(orc, cases, ctx.ldp, selected_variant=1)[0]
    stage(ctx, cases, selected_variant=1)
    run_restored_twice(ctx, cases, want, tag="selected C=12")
    ctx.close()


def test_full_batch_accept_cap_vs_oracle(orc):
    """k_info_apply<66, 1> behind the accepted-feature cap (max_accept = 20, compress_rule = 0: the as-written rule), 70 filters."""
    cases = batch(orc, 1100, bs.uniform_desc(11, True, NB))
    ctx = make_ctx(cases)
    want = bs.oracle_steps(orc, cases, ctx.ldp, max_accept=20, compress_rule=0)[0]
    assert all(w[2].sum() <= 20 for w in want) and any(w[2].sum() == 20 for w in want)
    stage(ctx, cases, max_accept=20, compress_rule=0)
    run_restored_twice(ctx, cases, want, tag="cap 20")
    ctx.close()


@pytest.mark.parametrize("B,stereo", [(260, False), (130, True)])
def test_gram_chunk_counts_vs_oracle(orc, B, stereo):
    """The Gram chunking at class 66 away from 16 (few filters), 7 (the tests above) and config 4's one chunk on full, stereo frames:
    260 filters = ONE chunk holding all features of a filter (no k_chunk_sum) on the mixed, ragged, MONO batch; 130 filters = 3 chunks.
    k_info_apply<66, 1> with 33 / 17 groups of eight filters."""
    assert (512 // B) == (1 if B == 260 else 3)
    cases = batch(orc, 5000 + B, bs.mixed_desc(11, stereo, B))
    ctx = make_ctx(cases)
    want = bs.oracle_steps(orc, cases, ctx.ldp)[0]
    stage(ctx, cases)
    run_restored_twice(ctx, cases, want, tag="B=%d" % B)
    ctx.close()


def update_only(ctx, b0, cases, priors, **kw):
    """ingvio_msckf_update over filters [b0, b0 + len(cases)) on the covariance at update time"""
    for i, P in enumerate(priors):
        ctx.cov_set(b0 + i, P)
    dx, acc, gam, rows = ctx.msckf_update(b0, [c[2] for c in cases], **kw)
    return dx.copy(), acc.copy(), rows.copy(), [ctx.cov_get(b0 + i) for i in range(len(cases))], gam.copy()


def oracle_update_only(orc, cases, priors, ld, **kw):
    want = []
    for c, P in zip(cases, priors):
        oc = orc.Cov(P, ld=ld)
        dx, acc, gam, m = oc.msckf_update(c[2], **dict(dict(max_accept=0, compress_rule=1), **kw))
        want.append((oc.P, dx, acc, oc.n))
    return want


def test_sub_range_launch_vs_oracle(orc):
    """k_info_apply<66, 1> (no marginalisation: in place, no flip) launched over filters [5, 75) of a context of 80: the offsets of
    Apart, Asum, pc_base, T and the result slots by b0.  The seventy match the oracle, the ten outside keep their covariance bit for
    bit."""
    cases = batch(orc, 11000, bs.mixed_desc(11, True, NB))
    ctx = make_ctx(cases, batch_size=80)
    priors = [bs.prior_at_update(orc, c, ctx.ldp) for c in cases]
    rng = np.random.default_rng(5)
    outside = {}
    for b in list(range(5)) + list(range(75, 80)):
        n = 40 + b
        A = rng.standard_normal((n, n)); outside[b] = A @ A.T / n + 0.05 * np.eye(n)
        ctx.cov_set(b, outside[b])
    res = update_only(ctx, 5, cases, priors)
    check(cases, res[:4], oracle_update_only(orc, cases, priors, ctx.ldp), TIGHT, 1e-8, "sub-range [5, 75) of 80")
    for b, P in outside.items():
        assert ctx.n(b) == P.shape[0] and np.array_equal(ctx.cov_get(b), P), b
    ctx.close()


@pytest.mark.parametrize("C,stereo", [(4, True), (6, False), (11, True), (11, False), (12, True), (16, True), (16, False)])
def test_few_filter_launches_equal_the_full_batch_launch(orc, C, stereo):
    """The same 70 filters of one context (so the same 7 Gram chunks) updated in ONE launch (k_info_apply<NC, 1>) and in launches of 35
    (k_apply_T_flat<NC> + k_apply_sym_flat<NC>): both paths add the K = NC products of T = Pc M and of T Pc^T in the same MFMA order, so
    posterior, dx, gamma, masks and rows are bit-identical, for every class."""
    cases = batch(orc, 1000 * C + (0 if stereo else 500), bs.mixed_desc(C, stereo, NB)) if C in (11, 16) else \
        batch(orc, 100 * C + (0 if stereo else 50), bs.uniform_desc(C, stereo, NB))
    ctx = make_ctx(cases)
    priors = [bs.prior_at_update(orc, c, ctx.ldp) for c in cases]
    full = update_only(ctx, 0, cases, priors)
    few = [update_only(ctx, b0, cases[b0:b0 + 35], priors[b0:b0 + 35]) for b0 in (0, 35)]
    check(cases, full[:4], oracle_update_only(orc, cases, priors, ctx.ldp), TIGHT, 1e-8, "update only C=%d" % C)
    worst = 0.0
    for h, b0 in enumerate((0, 35)):
        for k in (0, 1, 2, 4):
            assert np.array_equal(few[h][k], full[k][b0:b0 + 35], equal_nan=(k == 4)), (C, stereo, b0, k)
        for i in range(35):
            worst = max(worst, rel_err(few[h][3][i], full[3][b0 + i]))
            assert np.array_equal(few[h][3][i], full[3][b0 + i]), (C, stereo, b0 + i, rel_err(few[h][3][i], full[3][b0 + i]))
    ctx.close()


@pytest.mark.parametrize("strong_reject", [0, 1])
def test_full_batch_in_frame_gnss_vs_oracle(orc, strong_reject):
    """k_post_cols<66> + k_info_apply<66, 1, 16> at 70 filters (the config-3 line of the benchmark runs them at 512, the suite at 5):
    the GNSS update of the frame folded into the MSCKF write-back.  Every third filter has no GNSS block (gm = 0) next to filters
    with one; two filters reject every feature (the downdate alone rides on the compaction); with strong_reject filter 1's block is
    refused as a whole.  Pattern and tolerances of test_config3_in_frame_gnss_vs_oracle[small]."""
    from ingvio_amd import capi, host, synth
    desc = bs.uniform_desc(11, True, NB, lm_max=14)
    desc["roles"][10] = desc["roles"][41] = "rejected"
    cases = batch(orc, 11500, desc)
    ctx = make_ctx(cases)
    table = cases[0][2]["chi2_table"]
    blocks = []
    for b, c in enumerate(cases):
        g = synth.make_gnss(np.random.default_rng(940 + b), c[3]["flt"], outliers=(5,) if b % 2 == 0 else (1, 6))
        blocks.append(None if b % 3 == 2 else (g, host.gnss_rows(g)))
    if strong_reject:                                    # filter 1: gross residuals on <= 14 rows, no row may pass on its own merit
        g, (v, s_, H, r, Rd) = blocks[1]
        blocks[1] = (g, (v, s_, H[:12], np.full(12, 500.0), Rd[:12]))
    stage(ctx, cases)
    ctx.gnss_stage(0, [None if blk is None else blk[1] for blk in blocks], table, gate_rows=not strong_reject, strong_reject=bool(strong_reject),
                   in_frame=True)
    first = None
    for rep in range(2):
        ctx.frame_run(restore_prior=True)
        dxv, acc, rows, Ps = fetch(ctx, NB)
        dxg, used, keep, gam, st = ctx.gnss_fetch()
        if rep == 1:
            assert np.array_equal(dxv, first[0]) and np.array_equal(dxg, first[1]) and all(np.array_equal(Ps[b], first[2][b]) for b in range(NB))
            break
        first = (dxv, dxg, Ps)
        n_rej = 0
        for b, (prior, step, frame, info) in enumerate(cases):
            F, n_post = info["F"], info["N_update"] - 6
            oc = orc.Cov(prior, ld=ctx.ldp)
            dxo, acco, gamo, m = orc.frame_update(oc, step, frame, max_accept=0, compress_rule=1)
            assert np.array_equal(acc[b, :F], acco), b
            if acco.any():
                assert rel_err(dxv[b, :n_post + 6], dxo) < 1e-9 and rows[b] == 66, b
            else:
                assert info["role"] == "rejected" and not dxv[b, :n_post + 6].any() and rows[b] == 0, b
            if blocks[b] is None:
                assert used[b] == 0 and not dxg[b].any(), (b, used[b])
            else:
                g, (vidx, vsize, Hc, rc, Rdc) = blocks[b]
                if not strong_reject:
                    go = dict(g); go.update(chi2_test=1, chi2_table=table)
                    Ho, ro, Rdo, vio, vso = orc.gnss_rows(oc, go)
                    kept = np.flatnonzero(keep[b, :len(rc)])
                    assert used[b] == len(ro) == len(kept) and np.array_equal(rc[kept], ro), b
                else:
                    Ho, ro, Rdo, vio, vso = Hc, rc, Rdc, vidx, vsize
                blk_ok = not (strong_reject and len(ro) <= 14) or oc.whiten(vio, vso, Ho, ro, Rdo) < table[len(ro)]
                if blk_ok:
                    dxo2, _ = oc.ekf_update(vio, vso, Ho, ro, Rdo)
                    assert st[b] == 0 and rel_err(dxg[b, :n_post], dxo2) < 1e-9 and not dxg[b, n_post:].any(), (b, st[b])
                else:
                    n_rej += 1
                    assert b == 1 and st[b] == capi.REJECTED and not dxg[b].any(), (b, st[b])
            assert Ps[b].shape[0] == n_post and rel_err(Ps[b], oc.P) < 1e-11 and np.array_equal(Ps[b], Ps[b].T), (b, rel_err(Ps[b], oc.P))
        assert n_rej == (1 if strong_reject else 0)
    ctx.close()


# ---- windows of 17 .. 36 clones, four or more filters per launch ----------------------------------------------------------------
def big_desc(C, stereo, nb, F=48, lm_max=8, selected=False, lm=None):
    """large-window batch: mixed state sizes (filter 0 the largest), filter 1 without marginalisation (4 blocks of head room), filter
    2 rejecting every feature"""
    roles = ["ordinary"] * nb
    lm = list(lm) if lm else [lm_max if b == 0 else (3 * b + 1) % (lm_max + 1) for b in range(nb)]
    if nb > 1:
        roles[1] = "inplace"; lm[1] = min(lm[1], lm[0] - 4)
    if nb > 2:
        roles[2] = "rejected"
    return dict(C=C, stereo=stereo, F=F, selected=selected, roles=roles, lm=lm)


@pytest.mark.parametrize("nb,C,c_max,stereo,selected", [(4, 17, 17, False, 0), (9, 22, 30, True, 0), (12, 30, 30, True, 0), (9, 36, 36, False, 0),
                                                        (12, 17, 17, True, 0), (4, 36, 36, True, 0), (9, 24, 24, True, 1)])
def test_large_window_batches_vs_oracle(orc, nb, C, c_max, stereo, selected):
    """k_apply_T64b + k_apply_sym64b (what the config-5 line of the benchmark measures): 4, 9 and 12 filters per launch (fpx 1 and 2,
    not multiples of 8), 17 .. 36 clones, one context class above its window, stereo and mono, ragged, random anchors, mixed state
    sizes, one filter with marg_idx = -1, one rejecting everything; the Selected-timestamp variant once.  Restored prior twice, then
    two consecutive steps without restore."""
    cases = batch(orc, 200 * C + nb, big_desc(C, stereo, nb, selected=bool(selected)))
    ctx = make_ctx(cases, c_max=c_max)
    kw = dict(selected_variant=selected)
    want = bs.oracle_steps(orc, cases, ctx.ldp, steps=2, **kw)
    stage(ctx, cases, **kw)
    tag = "nb=%d C=%d/%d %s" % (nb, C, c_max, "stereo" if stereo else "mono")
    run_restored_twice(ctx, cases, want[0], 1e-10, 1e-7, tag)
    ctx.restore()
    for it in range(2):
        ctx.frame_run(restore_prior=False)
        check(cases, fetch(ctx, nb), want[it], 1e-10, 1e-7, tag + " step %d" % it)
    ctx.close()


BIG_APPLY = {20: (492, [115, 100, 60, 115, 30]), 24: (771, [200, 170, 120, 200, 40])}


@pytest.mark.parametrize("nb", [1, 2, 5])
@pytest.mark.parametrize("c_max", [20, 24])
def test_long_state_large_window_vs_oracle(orc, c_max, nb):
    """k_info_apply_big: launch_bigwin keeps T = Pc M in the solve workspace's X2 | Y2 region only if it fits,
        ldt * BIG_NC <= 2 * ld2 * n32    with ldt = ceil32(n_max), BIG_NC = 216, n32 = ceil32(6 c_max), ld2 = 3 n32 + 32 (BigWs),
    and otherwise takes the one-launch write-back that keeps a tile row of T in LDS.  c_max = 20: n32 = 128, ld2 = 416: 106496 doubles,
    ldt <= 480; n_max = 492 -> ldt = 512, 110592: does not fit.  c_max = 24: n32 = 160, ld2 = 512: 163840, ldt <= 736; n_max = 771 ->
    ldt = 800, 172800: does not fit.  1, 2 and 5 filters of different sizes (filter 0 at n_max), with and without marginalisation,
    one rejecting everything."""
    n_max, lms = BIG_APPLY[c_max]
    n32 = (6 * c_max + 31) // 32 * 32
    assert ((n_max + 31) // 32 * 32) * 216 > 2 * (3 * n32 + 32) * n32 and bs.state_size(c_max, lms[0]) == n_max
    cases = batch(orc, 900 * c_max, big_desc(c_max, True, 5, lm=lms))[:nb]
    ctx = make_ctx(cases)
    assert ctx.n_max == n_max
    want = bs.oracle_steps(orc, cases, ctx.ldp)[0]
    stage(ctx, cases)
    run_restored_twice(ctx, cases, want, 1e-10, 1e-7, "c_max=%d n_max=%d nb=%d" % (c_max, n_max, nb))
    ctx.close()


def test_large_window_few_filter_launches_against_one_launch(orc):
    """Five 22-clone filters of one context updated in one launch (k_apply_T64b + k_apply_sym64b) and in launches of 2 + 2 + 1 (k_apply_T
    + k_apply_sym): 32- and 64-blocks split K differently, so no bit-identity - the large-window bound between the two, and each
    against the oracle."""
    cases = batch(orc, 200 * 22 + 5, big_desc(22, True, 5))
    ctx = make_ctx(cases)
    priors = [bs.prior_at_update(orc, c, ctx.ldp) for c in cases]
    want = oracle_update_only(orc, cases, priors, ctx.ldp)
    one = update_only(ctx, 0, cases, priors)
    check(cases, one[:4], want, 1e-10, 1e-7, "five in one launch")
    for b0, k in ((0, 2), (2, 2), (4, 1)):
        few = update_only(ctx, b0, cases[b0:b0 + k], priors[b0:b0 + k])
        check(cases[b0:b0 + k], few[:4], want[b0:b0 + k], 1e-10, 1e-7, "launch of %d at %d" % (k, b0))
        assert np.array_equal(few[1], one[1][b0:b0 + k]) and np.array_equal(few[2], one[2][b0:b0 + k])
        for i in range(k):
            assert rel_err(few[3][i], one[3][b0 + i]) < 1e-10, (b0 + i, rel_err(few[3][i], one[3][b0 + i]))
            if want[b0 + i][2].any():
                n = len(want[b0 + i][1])
                assert rel_err(few[0][i, :n], one[0][b0 + i, :n]) < 1e-7, b0 + i
    ctx.close()
