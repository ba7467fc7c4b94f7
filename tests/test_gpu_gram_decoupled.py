"""k_feat_gram3 in its reduced form (ingvio_set_gram_decoupled): the fused frame step's Gram stage of the window classes 6
and 11 with the wave pairs of a workgroup decoupled - operand panel and sparse scratch double-buffered, one barrier per batch, the
tiles of the rank-3 product dealt over the four waves by a table.  Every entry of the chunk partials is the same sum in the same order
as in the reduced k_feat_gram2, so the same staged frame, run from the same snapshot with the switch off and on, must give the
posterior, dx, the accept mask, the row count and n EQUAL BIT FOR BIT; ingvio_last_gram_form says which kernel ran (1 / 2).  One case
is also held against the oracle, so that the pair is not only compared with itself.

The number of chunks follows the batch (512 / B, at most 16), so the shapes of the kernel's pipeline - one full batch of eight
features, both buffers, a short last batch, several chunks, empty chunks - need batches of up to 512 filters.  A handful of distinct
cases are built and staged round-robin over the batch; windows stay at N <= 87."""
import functools

import numpy as np
import pytest

from conftest import rel_err
from test_gpu_gram_reduced import _ragged

pytestmark = pytest.mark.gpu

TIGHT = 1e-11           # tests/test_gpu_parity.py, the fused frame step against the oracle: covariance
DX_TOL = 1e-9           # ... and dx (test_full_n249_batch_vs_oracle)


def _build(specs, B, c_max, stereo=True, ragged=False, n_max=96, seed0=500, outlier_every=7):
    """specs: (C, F) of the distinct cases; filter b of the batch of B runs case b % len(specs).  Returns (ctx, cases [B], priors [K])
    with the snapshot taken at the priors."""
    from ingvio_amd import capi, host, synth
    K = len(specs)
    ctx = capi.Context(batch=B, n_max=n_max, c_max=c_max, f_max=max(max(F for _, F in specs), 4), m_max=64)
    distinct = []
    for b, (C, F) in enumerate(specs):
        flt, step, frame, info = synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=seed0 + b, F=F, C=C,
                                                  n_gnss=0, n_landmarks=0, stereo=stereo, outlier_every=outlier_every)
        if ragged:
            frame = _ragged(frame, C, F, stereo, 9000 + seed0 + b)
        distinct.append((flt, step, frame, info))
    priors = [ctx.cov_get(b) for b in range(K)]
    for b in range(K, B):
        ctx.cov_set(b, priors[b % K])
    ctx.snapshot()
    return ctx, [distinct[b % K] for b in range(B)], priors


def _run(ctx, on):
    ctx.set_gram_decoupled(on)
    ctx.frame_run(restore_prior=True)
    form = ctx.last_gram_form()
    dx, acc, rows = ctx.frame_fetch()
    nb = dx.shape[0]
    return dict(dx=dx.copy(), acc=acc.copy(), rows=rows.copy(), n=np.array([ctx.n(b) for b in range(nb)]),
                P=[ctx.cov_get(b) for b in range(nb)], form=form)


def _pair(ctx, cases, forms=(1, 2), **opts):
    """the same staged frame from the same snapshot, switch off then on (the reduced form allowed in both); returns (off, on)"""
    ctx.set_gram_reduced(True)
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"], **opts)
    off = _run(ctx, False)
    on = _run(ctx, True)
    assert (off["form"], on["form"]) == forms, (off["form"], on["form"])
    return off, on


def _assert_bit_equal(off, on, cases):
    for k in ("dx", "acc", "rows", "n"):
        assert np.array_equal(off[k], on[k]), k
    for b, (Pa, Pb) in enumerate(zip(off["P"], on["P"])):
        assert Pa.shape == Pb.shape and np.array_equal(Pa, Pb), b
    for b, case in enumerate(cases):                                 # the update did something: features accepted, rows stacked
        F = case[2]["pf"].shape[0]
        assert off["acc"][b, :F].sum() > 0 and off["rows"][b] > 0 and np.abs(off["dx"][b]).max() > 0, b
        assert np.isfinite(off["dx"][b]).all() and np.isfinite(off["P"][b]).all()


K1 = 4                  # distinct cases of the one-chunk batches


@functools.lru_cache(maxsize=None)
def _case20():
    """B = 512 (one chunk), class 11, C = 11, stereo, F = 20 with two outliers: three batches, the last one short; shared with the oracle case"""
    ctx, cases, priors = _build([(11, 20)] * K1, 512, 11)
    off, on = _pair(ctx, cases)
    ld = ctx.ldp
    ctx.close()
    return cases, priors, off, on, ld


@pytest.mark.parametrize("F", [8, 16, 17])
def test_one_chunk_full_batches(F):
    """B = 512: one chunk per filter.  No outliers, so F = 8 is exactly one full batch (the producers build nothing inside the loop),
    16 two full batches (both buffers), 17 a third batch of one feature (stacked rows 3..23 of the refilled buffer cleared)."""
    ctx, cases, _ = _build([(11, F)] * K1, 512, 11, outlier_every=0, seed0=520 + F)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)
    assert (off["acc"][:K1, :F].sum(axis=1) == F).any(), off["acc"][:K1, :F].sum(axis=1)      # the shape the case is named for
    assert (off["rows"] == 66).all()


def test_one_chunk_three_batches_last_short():
    cases, priors, off, on, ld = _case20()
    _assert_bit_equal(off, on, cases)
    assert (off["rows"] == 66).all() and (off["acc"][:, :20].sum(axis=1) > 16).all()      # more than two batches of eight


def test_several_chunks():
    """B = 64: eight chunks per filter; F = 150 with every 7th feature an outlier leaves ~129 used features, 17 per chunk: three
    batches per chunk, the last one short"""
    ctx, cases, _ = _build([(11, 150)] * 3, 64, 11, seed0=540)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)
    used = off["acc"][:, :150].sum(axis=1)
    assert ((used > 8 * 16) & (used <= 8 * 24)).all(), used              # ceil(used / 8) in 17..24: three batches per chunk


def test_empty_chunks():
    """B = 3: sixteen chunks per filter, at most five used features - one per chunk, eleven chunks empty (one barrier each role)"""
    ctx, cases, _ = _build([(11, 5)] * 3, 3, 11, seed0=560)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)


def test_mixed_window_sizes_reference_mid_panel():
    """C = 8 and C = 11 in the SAME launch: the reference slot is per filter and, for C = 8, sits in the middle of the class-11 panel.
    Ragged observation sets; the four fixed shapes of _ragged must all be among the used features."""
    ctx, cases, _ = _build([(8, 12), (11, 12), (8, 12), (11, 12)], 4, 11, ragged=True, seed0=300)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)
    assert list(off["n"]) == [63, 81, 63, 81]
    assert off["acc"][:, :4].all(), off["acc"][:, :4]


def test_mixed_window_sizes_one_chunk():
    """the same mix at B = 512: the ragged features of a filter in ONE chunk, two batches"""
    ctx, cases, _ = _build([(8, 12), (11, 12), (8, 12), (11, 12)], 512, 11, ragged=True, seed0=300)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)
    assert off["acc"][:4, :4].all(), off["acc"][:4, :4]


def test_class6_two_window_sizes():
    ctx, cases, _ = _build([(6, 9), (4, 9), (6, 9)], 512, 6, ragged=True, seed0=300)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)
    assert list(off["n"][:3]) == [51, 39, 51]


def test_mono_class11():
    ctx, cases, _ = _build([(11, 12)] * 2, 512, 11, stereo=False, ragged=True, seed0=300)
    off, on = _pair(ctx, cases)
    ctx.close()
    _assert_bit_equal(off, on, cases)


def test_capped_accept_list_without_compression():
    """max_accept = 3 with compress_rule = 0: the capped list of used features feeds the kernel"""
    ctx, cases, _ = _build([(11, 12)] * 2, 512, 11, seed0=300)
    off, on = _pair(ctx, cases, max_accept=3, compress_rule=0)
    ctx.close()
    _assert_bit_equal(off, on, cases)
    assert (off["acc"][:, :12].sum(axis=1) == 3).all()


@pytest.mark.parametrize("kind", ["class12", "selected_variant", "fourteen_clones"])
def test_fallbacks_keep_their_form(kind):
    """Class 12 (144 slot-anchor pairs) keeps the reduced k_feat_gram2; the Selected-timestamp variant and a 14-clone window (N = 105,
    so n_max = 112) keep the full form - whatever the switch says, with equal results."""
    if kind == "class12":
        ctx, cases, _ = _build([(12, 9)] * 2, 2, 12, seed0=300)
        off, on = _pair(ctx, cases, forms=(1, 1))
    elif kind == "selected_variant":
        ctx, cases, _ = _build([(11, 9)] * 2, 2, 11, seed0=300)
        off, on = _pair(ctx, cases, forms=(0, 0), selected_variant=1)
    else:
        ctx, cases, _ = _build([(14, 9)] * 2, 2, 14, n_max=112, seed0=300)
        off, on = _pair(ctx, cases, forms=(0, 0))
    ctx.close()
    _assert_bit_equal(off, on, cases)


def test_reduced_switch_off_gives_the_full_form():
    """ingvio_set_gram_reduced(0) wins: the full k_feat_gram2 with the decoupled switch on, and the parity hook reads [A | b]"""
    ctx, cases, _ = _build([(11, 9)] * 2, 2, 11, seed0=300)
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
    ctx.set_gram_reduced(False)
    full = _run(ctx, True)
    A, bvec = ctx.debug_msckf_info(0)
    ctx.set_gram_reduced(True)
    on = _run(ctx, True)
    ctx.close()
    assert full["form"] == 0 and on["form"] == 2
    assert A.shape == (66, 66) and np.abs(A[60:, :]).max() > 0
    _assert_bit_equal(full, on, cases)


def test_decoupled_step_against_oracle(orc):
    """the F = 20 one-chunk case with the switch on against the oracle's frame update, at the tolerances of the fused frame step in
    test_gpu_parity.py (the distinct cases: the others are copies of them)"""
    cases, priors, off, on, ld = _case20()
    for b in range(K1):
        flt, step, frame, info = cases[b]
        oc = orc.Cov(priors[b], ld=ld)
        dxo, acco, gamo, m = orc.frame_update(oc, step, frame, max_accept=0, compress_rule=1)
        assert np.array_equal(on["acc"][b, :20], acco) and np.array_equal(acco == 0, info["outlier"])
        assert on["n"][b] == 81 and on["rows"][b] == 66
        P = on["P"][b]
        assert rel_err(P, oc.P) < TIGHT and rel_err(on["dx"][b, :87], dxo) < DX_TOL
        assert np.array_equal(P, P.T) and np.diag(P).min() > 0
