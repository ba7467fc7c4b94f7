"""k_info_apply_res (ingvio_set_apply_resident): the fused frame step's write-back with the filter's whole P[:, window]
resident in LDS - one workgroup of eight waves per filter, T formed transposed straight into the sweep's A fragments, one workgroup
barrier, then a free-running sweep.  Every T element and every tile is the same sequence of MFMAs over the same operand pairs in the
same k order as in k_info_apply, so the same staged frame, run from the same snapshot with the switch off and on, must give posterior,
dx, accept mask, rows and n EQUAL BIT FOR BIT; ingvio_last_apply_form says which kernel ran (0 / 1).  The status words and the device's
cur / n are not readable through the frame ABI: a negative diagonal shows in the posterior that is compared, and the in-kernel flip
(cur ^= 1, n -= 6 on the device) decides where the NEXT step reads - the three-step case compares after every step.

Batches sit just above the few-filter path (65 .. 72 filters) so that the batch kernels run; a few distinct cases are staged
round-robin.  States are small except where the shape is the point (N = 255 fills all 16 tile rows of sPc; the bench shape N = 249)."""
import functools

import numpy as np
import pytest

import batch_scenarios as bs
from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-11           # tests/test_gpu_parity.py, the fused frame step against the oracle: covariance
DX_TOL = 1e-9           # ... and dx (test_full_n249_batch_vs_oracle)
KEYS = ("dx", "acc", "rows", "n")


def _build(specs, B, c_max, n_max, F_max=None, seed0=700, split_window=False):
    """specs: (C, F, n_gnss, n_landmarks) of the distinct cases; filter b of the batch of B runs case b % len(specs).  Returns
    (ctx, cases [B], priors [K]) with the snapshot taken at the priors.  split_window: the oldest clone's block is moved in front of
    the (one) landmark block of the prior, so that the window's columns are NOT one contiguous block."""
    from ingvio_amd import capi, host, synth
    K = len(specs)
    ctx = capi.Context(batch=B, n_max=n_max, c_max=c_max, f_max=F_max or max(max(s[1] for s in specs), 4), m_max=64)
    distinct = []
    for b, (C, F, ng, nl) in enumerate(specs):
        flt, step, frame, info = synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=seed0 + b, F=F, C=C,
                                                  n_gnss=ng, n_landmarks=nl, stereo=True, outlier_every=7)
        distinct.append((flt, step, frame, info))
    priors = [ctx.cov_get(b) for b in range(K)]
    if split_window:
        for b, (C, F, ng, nl) in enumerate(specs):
            assert ng == 0 and nl == 1
            flt, step, frame, info = distinct[b]
            n = priors[b].shape[0]
            perm = np.r_[0:21, 24:30, 21:24, 30:n]                    # [imu | clone 0 | landmark | clones 1 ..]
            priors[b] = np.ascontiguousarray(priors[b][np.ix_(perm, perm)])
            frame = dict(frame); step = dict(step)
            idx = frame["clone_idx"].copy(); assert idx[0] == 24 and step["marg_idx"] == 24
            idx[0] = 21; frame["clone_idx"] = idx; step["marg_idx"] = 21
            distinct[b] = (flt, step, frame, info)
    for b in range(B):
        ctx.cov_set(b, priors[b % K])
    ctx.snapshot()
    return ctx, [distinct[b % K] for b in range(B)], priors


def _fetch(ctx):
    form = ctx.last_apply_form()
    dx, acc, rows = ctx.frame_fetch()
    nb = dx.shape[0]
    return dict(dx=dx.copy(), acc=acc.copy(), rows=rows.copy(), n=np.array([ctx.n(b) for b in range(nb)]),
                P=[ctx.cov_get(b) for b in range(nb)], form=form)


def _run(ctx, on):
    ctx.set_apply_resident(on)
    ctx.frame_run(restore_prior=True)
    return _fetch(ctx)


def _pair(ctx, steps, frames, sigma, gnss=False, forms=(0, 1), **opts):
    """the same staged frame from the same snapshot, switch off then on; returns (off, on)"""
    ctx.frame_stage(0, steps, frames, sigma, *((1, 0.2, 0.2) if gnss else ()), **opts)
    off = _run(ctx, False)
    on = _run(ctx, True)
    assert (off["form"], on["form"]) == forms, (off["form"], on["form"])
    return off, on


def _pair_cases(ctx, cases, gnss=False, forms=(0, 1)):
    return _pair(ctx, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"], gnss, forms)


def _assert_bit_equal(off, on):
    for k in KEYS:
        assert np.array_equal(off[k], on[k]), k
    for b, (Pa, Pb) in enumerate(zip(off["P"], on["P"])):
        assert Pa.shape == Pb.shape and np.array_equal(Pa, Pb), (b, Pa.shape, Pb.shape)
        assert np.isfinite(Pa).all() and np.array_equal(Pa, Pa.T), b


def _assert_updated(off, cases, priors):
    """the update did something: features accepted, rows stacked, a correction, a posterior below the prior's trace"""
    K = len(priors)
    for b, case in enumerate(cases):
        F = case[2]["pf"].shape[0]
        assert off["acc"][b, :F].sum() > 0 and off["rows"][b] > 0 and np.abs(off["dx"][b]).max() > 0, b
        assert np.isfinite(off["dx"][b]).all()
        assert off["n"][b] == priors[b % K].shape[0], b               # + 6 (clone) - 6 (marginalised)


SHAPES = {
    # name: (specs, B, c_max, n_max, n after the step)
    "odd_tiles_one_row_last": ([(3, 9, 0, 0)] * 3, 65, 6, 48, 33),        # N = 39, no = 33: nt = 3, the middle row unpaired, one row in the last tile
    "class36": ([(6, 9, 0, 0)] * 3, 66, 6, 64, 51),                       # N = 57, nt = 4
    "class66_partial_last": ([(11, 12, 0, 0)] * 3, 67, 11, 96, 81),       # N = 87, no = 81
    "class66_full_tiles": ([(11, 12, 0, 5)] * 3, 68, 11, 112, 96),        # N = 102, no = 96: no predicated tile off the diagonal
    "largest_state": ([(11, 12, 6, 54)] * 2, 65, 11, 256, 249),           # N = 255 in a 256-wide context: nt = 16, all of sPc
    "window_below_class": ([(8, 10, 0, 0)] * 3, 69, 11, 80, 63),          # C = 8 in class 11: M zero-padded, Pc from the copy
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_bit_equal(name):
    specs, B, c_max, n_max, n_post = SHAPES[name]
    ctx, cases, priors = _build(specs, B, c_max, n_max)
    off, on = _pair_cases(ctx, cases, gnss=specs[0][2] > 0)
    ctx.close()
    _assert_bit_equal(off, on)
    _assert_updated(off, cases, priors)
    assert (off["n"] == n_post).all(), off["n"]


@functools.lru_cache(maxsize=None)
def _bench_shape():
    ctx, cases, priors = _build([(11, 150, 6, 52)] * 2, 72, 11, 256, seed0=0)
    off, on = _pair_cases(ctx, cases, gnss=True)
    ld = ctx.ldp
    ctx.close()
    return cases, priors, off, on, ld


def test_bench_shape_bit_equal():
    """N = 249, 150 stereo features, 11 clones, 72 filters"""
    cases, priors, off, on, ld = _bench_shape()
    _assert_bit_equal(off, on)
    _assert_updated(off, cases, priors)
    assert (off["n"] == 243).all()


def test_bench_shape_against_oracle(orc):
    """the switched-on side of the bench shape against the oracle's frame update, at the tolerances of test_full_n249_batch_vs_oracle
    (the distinct cases: the others are copies of them)"""
    cases, priors, off, on, ld = _bench_shape()
    for b in range(len(priors)):
        flt, step, frame, info = cases[b]
        oc = orc.Cov(priors[b], ld=ld)
        dxo, acco, gamo, m = orc.frame_update(oc, step, frame, max_accept=0, compress_rule=1)
        assert np.array_equal(on["acc"][b, :150], acco) and np.array_equal(acco == 0, info["outlier"])
        assert on["n"][b] == 243 and on["rows"][b] == 66
        P = on["P"][b]
        eP, ed = rel_err(P, oc.P), rel_err(on["dx"][b, :249], dxo)
        print("filter %d: posterior %.2e dx %.2e" % (b, eP, ed))
        assert eP < TIGHT and ed < DX_TOL
        assert np.array_equal(P, P.T) and np.diag(P).min() > 0


def test_non_contiguous_window():
    """The fused step takes clone_idx as the caller gives it: a state ordered [imu | clone 0 | landmark | clones 1 ..] presents a window
    whose columns are not one block, so the solve copies them (pc_base < 0) and the write-back reads P_c from the copy."""
    ctx, cases, priors = _build([(6, 9, 0, 1)] * 3, 66, 6, 64, split_window=True)
    idx = cases[0][2]["clone_idx"]
    assert (np.diff(idx) != 6).any()
    off, on = _pair_cases(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on)
    _assert_updated(off, cases, priors)
    assert (off["n"] == 54).all()


# ---- the mixed batch of tests/batch_scenarios.py: per-filter n, marg_idx = -1 (in place, no flip) beside flipping neighbours,
# ---- all-rejected filters (no update, the marginalisation's compaction alone) and filters with nothing to do at all
NB = 70


@functools.lru_cache(maxsize=None)
def _mixed_cases():
    from oracle import oracle
    oracle.build()
    return bs.build_batch(oracle, 11000, bs.mixed_desc(11, True, NB))


def _mixed_ctx(**kw):
    from ingvio_amd import capi
    cases = _mixed_cases()
    ctx = capi.Context(batch=NB, n_max=kw.get("n_max", bs.n_max_of(cases)), c_max=11, f_max=cases[0][3]["F"], m_max=64)
    for b, c in enumerate(cases):
        ctx.cov_set(b, c[0])
    ctx.snapshot()
    return ctx, cases


def _mixed_pair(ctx, cases, forms=(0, 1)):
    s0 = cases[0][1]
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], s0["sigma"], 1, s0["sigma_cb"], s0["sigma_rw"])
    off = _run(ctx, False)
    on = _run(ctx, True)
    assert (off["form"], on["form"]) == forms, (off["form"], on["form"])
    return off, on


def test_mixed_sizes_and_filters_without_update():
    ctx, cases = _mixed_ctx()
    off, on = _mixed_pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on)
    roles = [c[3]["role"] for c in cases]
    assert {"ordinary", "inplace", "rejected", "empty"} <= set(roles)
    assert len(set(off["n"])) > 4                                           # different n in one launch
    for b, (prior, step, frame, info) in enumerate(cases):
        N = info["N_update"]
        if info["role"] in ("rejected", "empty"):                           # no update: dx = 0, and with a marginalisation only the compaction
            assert off["rows"][b] == 0 and not off["dx"][b].any(), b
            assert off["n"][b] == (N if step["marg_idx"] < 0 else N - 6), b
        else:
            assert off["rows"][b] == 66 and np.abs(off["dx"][b]).max() > 0, b
            assert off["n"][b] == (N if info["role"] == "inplace" else N - 6), b


def test_three_consecutive_steps():
    """frame_run(restore_prior=False) three times: the in-kernel flip decides where the next step reads; compared after each step"""
    res = {}
    for on in (False, True):
        ctx, cases = _mixed_ctx()
        s0 = cases[0][1]
        ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], s0["sigma"], 1, s0["sigma_cb"], s0["sigma_rw"])
        ctx.set_apply_resident(on)
        ctx.restore()
        out = []
        for it in range(3):
            ctx.frame_run(restore_prior=False)
            out.append(_fetch(ctx))
        ctx.close()
        res[on] = out
    for it in range(3):
        assert (res[False][it]["form"], res[True][it]["form"]) == (0, 1), it
        _assert_bit_equal(res[False][it], res[True][it])
    assert not np.array_equal(res[False][0]["n"], res[False][2]["n"])       # the states moved on (the in-place filters grow)
    assert np.abs(res[False][2]["dx"]).max() > 0


# ---- fallbacks: k_info_apply (or the few-filter kernels) whatever the switch says, with equal results -----------------------------
@pytest.mark.parametrize("kind", ["gnss_fold", "twelve_clones", "few_filters", "wide_context"])
def test_fallbacks_keep_the_old_kernel(kind):
    if kind == "gnss_fold":
        from ingvio_amd import host, synth
        ctx, cases, priors = _build([(11, 12, 6, 2)] * 3, 66, 11, 112)
        blocks = []
        for b, c in enumerate(cases):
            g = synth.make_gnss(np.random.default_rng(940 + b % 3), c[0])
            blocks.append((g, host.gnss_rows(g)))
        s0 = cases[0][1]
        ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], s0["sigma"], 1, 0.2, 0.2)
        ctx.gnss_stage(0, [blk[1] for blk in blocks], cases[0][2]["chi2_table"], gate_rows=True, strong_reject=False, in_frame=True)
        off = _run(ctx, False)
        g_off = [np.array(a).copy() for a in ctx.gnss_fetch()]
        on = _run(ctx, True)
        g_on = [np.array(a).copy() for a in ctx.gnss_fetch()]
        assert ctx.debug_gnss_fused_last() == 2                             # the epoch did ride on the write-back
        assert (off["form"], on["form"]) == (0, 0)
        for a, b_ in zip(g_off, g_on):
            assert np.array_equal(a, b_)
        assert np.abs(g_off[0]).max() > 0
    elif kind == "twelve_clones":
        ctx, cases, priors = _build([(12, 12, 0, 0)] * 3, 66, 12, 96)
        off, on = _pair_cases(ctx, cases, forms=(0, 0))
    elif kind == "few_filters":
        ctx, cases, priors = _build([(11, 12, 0, 0)] * 3, 64, 11, 96)
        off, on = _pair_cases(ctx, cases, forms=(0, 0))
    else:
        ctx, cases, priors = _build([(11, 12, 0, 0)] * 3, 66, 11, 272)
        assert ctx.ldp > 256
        off, on = _pair_cases(ctx, cases, forms=(0, 0))
    ctx.close()
    _assert_bit_equal(off, on)
    _assert_updated(off, cases, priors)
