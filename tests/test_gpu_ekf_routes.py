"""The generic EKF update (ingvio_ekf_update, ingvio_ekf_update_batch, ingvio_chi2_gamma, ingvio_chi2_gamma_multi) on every solver
route and tile boundary, against the 80-bit reference of tests/ekf_cases.py.

Routes (ingvio_last_update_form): LDS (k_ekf_core + k_downdate), dense register-resident (k_gemm / k_gemm64, k_add_noise,
k_lm_factor<NTM> + k_lm_carry<NTM>, k_downdate64), dense sweep (k_chol_first / k_chol_step, k_chol_carried when split, k_lm_finish).
Every test asserts the form it means to exercise: a case that lands on another route fails.

Tolerances, relative to the reference: P+ 1e-11 on the LDS route, 1e-10 on the dense routes; dx 1e-9; gamma 1e-9 max(1, gamma).
tests/test_ekf_reference_model.py shows the formula itself determined to 1e-12 on each of these cases.  Every update also leaves
P == P^T bit for bit and every other filter of the context bit-identical."""
import ctypes as C

import numpy as np
import pytest

import ekf_cases as ec

pytestmark = pytest.mark.gpu

TIGHT = 1e-11           # LDS route
DENSE = 1e-10           # dense routes
TOL_DX = 1e-9
TOL_GAMMA = 1e-9

WORST = {}              # route -> [rel P+, rel dx] worst seen so far in this run (shown in every assertion message)
WORST_GAMMA = [0.0]
ORACLE = "float64 oracle"      # third entry of an expected value that oracle_update made (the reference's is its gamma)


def _capi():
    from ingvio_amd import capi
    return capi


def _fill(ctx, seed=5):
    """a distinct covariance in every filter, so that 'the others are untouched' compares real content"""
    rng = np.random.default_rng(seed)
    for b in range(ctx.batch):
        n = max(21, ctx.n_max - 7 * b - 3)
        A = rng.standard_normal((n, n))
        ctx.cov_set(b, 1e-2 * (A @ A.T / n + 0.1 * np.eye(n)))


def _others(ctx, lo, hi=None):
    hi = lo + 1 if hi is None else hi
    return {b: ctx.cov_get(b) for b in range(ctx.batch) if not lo <= b < hi}


def _others_same(ctx, before):
    return all(ctx.n(b) == P.shape[0] and np.array_equal(ctx.cov_get(b), P) for b, P in before.items())


def _route_name(form):
    capi = _capi()
    return {capi.UPDATE_LDS: "lds", capi.UPDATE_DENSE_REG: "dense_reg", capi.UPDATE_DENSE_SWEEP: "dense_sweep"}[form & 3]


def _check(label, form, P, dx, want, tol):
    """P+ and dx against (P+, dx, ...) of the reference (or of oracle_update); records the worst errors per route"""
    eP, ex = ec.rel(P, want[0]), ec.rel(dx, want[1])
    w = WORST.setdefault(_route_name(form) + (" (float64 oracle)" if want[2] is ORACLE else ""), [0.0, 0.0])
    w[0], w[1] = max(w[0], eP), max(w[1], ex)
    msg = "%s: rel P+ %.2e (< %.0e) rel dx %.2e (< %.0e); worst per route so far %s" % (label, eP, tol, ex, TOL_DX, WORST)
    assert np.array_equal(P, P.T), msg
    assert eP < tol and ex < TOL_DX, msg


def _set(ctx, b, c):
    d = ec.inputs(c)
    ctx.cov_set(b, d["P"])
    if c.marg:
        ctx.marginalize(b, [ec.MARG_IDX], ec.MARG_SIZE)
    return d


def run_single(ctx, b, c, form, tol, want=None):
    d = _set(ctx, b, c)
    before = _others(ctx, b)
    dx, rc = ctx.ekf_update(b, d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
    got = ctx.last_update_form()
    assert rc == 0 and got == form, "%s: rc %d, form 0x%x, meant 0x%x" % (c.name, rc, got, form)
    P = ctx.cov_get(b)
    _check(c.name, form, P, dx, want or ec.expected(c), tol)
    assert _others_same(ctx, before), c.name
    return P, dx


def run_batch(ctx, b0, cases, diag, form, tol, wants=None):
    blocks = []
    for i, c in enumerate(cases):
        d = _set(ctx, b0 + i, c)
        blocks.append((d["vidx"], d["vsize"], d["H"], d["res"], d["R"]))
    before = _others(ctx, b0, b0 + len(cases))
    dx, st = ctx.ekf_update_batch(b0, blocks, diag=diag)
    got = ctx.last_update_form()
    assert not st.any() and got == form, "status %s, form 0x%x, meant 0x%x" % (st, got, form)
    out = []
    for i, c in enumerate(cases):
        n = ctx.n(b0 + i)
        P = ctx.cov_get(b0 + i)
        _check("%s (filter %d of the batch)" % (c.name, i), form, P, dx[i, :n], wants[i] if wants else ec.expected(c), tol)
        out.append(P)
    assert _others_same(ctx, before)
    return out


def oracle_update(orc, c):
    d = ec.inputs(c)
    oc = orc.Cov(d["prior"])
    dx, _ = oc.ekf_update(d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
    return oc.P, dx, ORACLE


def raw_update(ctx, b, d, R):
    """ingvio_ekf_update without the wrapper's exception: (rc, dx) with dx pre-filled, to see what an error return wrote"""
    capi = _capi()
    H = np.asfortranarray(d["H"], dtype=np.float64)
    m = H.shape[0]
    Rb, kind = ctx._R(R, m)
    vi, vs, r = capi.i32(d["vidx"]), capi.i32(d["vsize"]), capi.f64(d["res"])
    dx = np.full(ctx.n(b), 7.0)
    rc = ctx.L.ingvio_ekf_update(ctx.h, b, capi._i(vi), capi._i(vs), len(vi), capi._d(H), m, m, capi._d(r), capi._d(Rb), kind, capi._d(dx))
    return rc, dx


def raw_update_batch(ctx, b0, blocks, diag):
    """ingvio_ekf_update_batch without the wrapper's exception: (rc, dx [nb, ldp], status [nb])"""
    capi = _capi()
    nb = len(blocks)
    arr = (capi.UpdateBlock * nb)(); keep = []
    for g, (vidx, vsize, H, res, R) in enumerate(blocks):
        H = np.asfortranarray(np.atleast_2d(H), dtype=np.float64)
        vi, vs, r, Rv = capi.i32(vidx), capi.i32(vsize), capi.f64(res), capi.f64(np.atleast_1d(R))
        keep.append((H, vi, vs, r, Rv))
        arr[g].vidx = capi._i(vi); arr[g].vsize = capi._i(vs); arr[g].k = len(vi); arr[g].H = capi._d(H); arr[g].ldh = H.shape[0]
        arr[g].m = H.shape[0]; arr[g].res = capi._d(r); arr[g].R = capi._d(Rv)
    dx = np.full((nb, ctx.ldp), 7.0); st = np.full(nb, 99, dtype=np.int32)
    rc = ctx.L.ingvio_ekf_update_batch(ctx.h, b0, nb, arr, 1 if diag else 0, capi._d(dx), capi._i(st))
    return rc, dx, st


def _dense_ctx(n_max, batch=2):
    """the single call leaves k_ekf_core above max(m_max, 6 c_max) = 18 rows, the batch call above mld = 48 rows"""
    ctx = _capi().Context(batch=batch, n_max=n_max, c_max=3, f_max=8, m_max=16)
    _fill(ctx)
    return ctx


@pytest.fixture(scope="module")
def ctx_lds():
    ctx = _capi().Context(batch=4, n_max=160, c_max=11, f_max=8, m_max=64)
    _fill(ctx)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx_cap():
    """a single call keeps up to max(m_max, 6 c_max) = 144 rows on the LDS route: only ekf_core_fits sends rows away"""
    ctx = _capi().Context(batch=2, n_max=160, c_max=24, f_max=8, m_max=128)
    _fill(ctx)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx_batch():
    ctx = _capi().Context(batch=7, n_max=160, c_max=11, f_max=8, m_max=64)
    _fill(ctx)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nworst errors against the 80-bit reference per route [rel P+, rel dx]: %s; gamma %.2e" % (WORST, WORST_GAMMA[0]))


# ---- LDS route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.LDS_CASES, ids=lambda c: c.name)
def test_lds_single(ctx_lds, c):
    """k_ekf_core on both sides of its nc <= 16 and m <= 16 register paths, partial 16-row groups up to m = 66 under mld = 80, live
    n around the 16 x 16 downdate tiles"""
    run_single(ctx_lds, 1, c, _capi().UPDATE_LDS, TIGHT)


def test_lds_capacity(ctx_cap):
    """k_ekf_core's S, column map and 256 static bytes in 160 KB of LDS: 141 rows are the last on the LDS route with any number of
    columns, 142 and 143 rows take the dense route.  (Counting the dynamic bytes alone, 142 rows over up to 58 columns were sent to
    k_ekf_core, whose dispatch the hardware refused: m = 142 with 17, 58 and 59 columns stay here as cases.)"""
    capi = _capi()
    dense = capi.update_form(capi.UPDATE_DENSE_REG, ntm=12)
    for c in ec.CAP_LDS_CASES:
        run_single(ctx_cap, 0, c, capi.UPDATE_LDS, TIGHT)
    for c in ec.CAP_DENSE_CASES:
        run_single(ctx_cap, 0, c, dense, DENSE)
    P_58, dx_58 = run_single(ctx_cap, 0, ec.CAP_EDGE, dense, DENSE)
    # the same rows over 59 columns, the 59th (a state column outside var_order) with a zero column of H: the same posterior
    d = dict(ec.inputs(ec.CAP_EDGE))
    named = set(ec._cols(d["vidx"], d["vsize"]).tolist())
    free = next(j for j in range(ec.CAP_EDGE.n) if j not in named and j - 1 not in named and j + 1 not in named)
    d["vidx"] = d["vidx"] + [free]; d["vsize"] = d["vsize"] + [1]
    d["H"] = np.hstack([d["H"], np.zeros((ec.CAP_EDGE.m, 1))])
    ctx_cap.cov_set(0, d["P"])
    before = _others(ctx_cap, 0)
    dx, rc = ctx_cap.ekf_update(0, d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
    assert rc == 0 and ctx_cap.last_update_form() == dense, hex(ctx_cap.last_update_form())
    P = ctx_cap.cov_get(0)
    _check("m142-nc59", dense, P, dx, ec.expected(ec.CAP_EDGE), DENSE)
    assert ec.rel(P, P_58) < 2 * DENSE and ec.rel(dx, dx_58) < 2 * TOL_DX and _others_same(ctx_cap, before)


def test_batch_lds_sized_by_the_whole_call():
    """the batch call launches k_ekf_core once, its LDS sized by the most rows and the most columns of the call: 141 rows in one filter
    and 600 columns in another fit one by one and not together - the call takes the dense route"""
    capi = _capi()
    ctx = capi.Context(batch=2, n_max=608, c_max=24, f_max=8, m_max=128)
    try:
        run_batch(ctx, 0, ec.BATCH_LDS_SIZING, True, capi.update_form(capi.UPDATE_DENSE_REG, ntm=12), DENSE)
    finally:
        ctx.close()


# ---- dense, register-resident ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntm", sorted(ec.DENSE_REG))
def test_dense_register_resident(ntm):
    """one fresh context per tile class: k_lm_factor<NTM> / k_lm_carry<NTM> with full and partial last 16-row tiles, n = n_max and n
    well below it, the three noise kinds through k_add_noise"""
    capi = _capi()
    n_max, cases = ec.DENSE_REG[ntm]
    ctx = _dense_ctx(n_max)
    try:
        for c in cases:
            run_single(ctx, 1, c, capi.update_form(capi.UPDATE_DENSE_REG, ntm=ntm), DENSE)
        if ntm == 16:       # the workspace only grows: a small system in the 256-row workspace, over identity-padded rows
            run_single(ctx, 1, ec.DENSE_REG_SMALL, capi.update_form(capi.UPDATE_DENSE_REG, ntm=16), DENSE)
    finally:
        ctx.close()


# ---- dense, sweep ----------------------------------------------------------------------------------------------------------------
def test_dense_sweep(orc):
    capi = _capi()
    sweep = capi.update_form(capi.UPDATE_DENSE_SWEEP)
    ctx = _dense_ctx(160)
    try:
        for c in ec.SWEEP_CASES:
            run_single(ctx, 0, c, sweep, DENSE)
        run_single(ctx, 0, ec.SWEEP_SMALL, sweep, DENSE)      # the workspace stays above 256 rows: 70 rows still take the sweep
        # 1024 rows, the most the route takes: against the float64 oracle only (the 80-bit reference takes several seconds here)
        run_single(ctx, 0, ec.SWEEP_MAX, sweep, DENSE, want=oracle_update(orc, ec.SWEEP_MAX))
        d = _set(ctx, 0, ec.SWEEP_OVER)
        before = _others(ctx, -1)
        with pytest.raises(capi.IngvioError) as e:
            ctx.ekf_update(0, d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
        assert e.value.code == capi.E_CAPACITY and _others_same(ctx, before)
    finally:
        ctx.close()


# ---- the covariance in the second ping-pong half, a shrunken state ------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lds", "reg", "sweep"])
def test_second_pingpong_half(ctx_lds, route):
    """ingvio_marginalize moves the filter's covariance to the other half of its buffer pair: the dense routes' products read it
    through a_sel, the downdates through the view"""
    capi = _capi()
    c = ec.PINGPONG[route]
    if route == "lds":
        run_single(ctx_lds, 2, c, capi.UPDATE_LDS, TIGHT)
        return
    ctx = _dense_ctx(160)
    try:
        form = capi.update_form(capi.UPDATE_DENSE_REG, ntm=8) if route == "reg" else capi.update_form(capi.UPDATE_DENSE_SWEEP)
        run_single(ctx, 1, c, form, DENSE)
    finally:
        ctx.close()


def test_shrunken_state():
    """n = n_max, an update, then n = 49 into the same filter: beyond the live n the buffer holds an old posterior, not zeros"""
    capi = _capi()
    ctx = _dense_ctx(129)
    try:
        run_single(ctx, 1, ec.SHRUNK_BIG, capi.update_form(capi.UPDATE_DENSE_REG, ntm=4), DENSE)
        run_single(ctx, 1, ec.SHRUNK, capi.update_form(capi.UPDATE_DENSE_REG, ntm=8), DENSE)
    finally:
        ctx.close()


# ---- batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "diag"])
def test_batch_lds(ctx_batch, kind):
    """nb = 5 at b0 = 1 in a context of 7: m = 1, 16, 17, 66, 80 with a different n and var_order per filter.  The batch call has no
    m_max check: 80 rows run on k_ekf_core here and on the dense route in a single call - the same posterior"""
    capi = _capi()
    cases = ec.BATCH_LDS[kind]
    Ps = run_batch(ctx_batch, 1, cases, kind == "diag", capi.UPDATE_LDS, TIGHT)
    P1, _ = run_single(ctx_batch, 5, cases[4], capi.update_form(capi.UPDATE_DENSE_REG, ntm=8), DENSE)
    assert ec.rel(P1, Ps[4]) < TIGHT + DENSE


def test_batch_dense_mixed_tile_counts():
    """m = (40, 256, 130) in one call: three tile counts in the class-16 kernel"""
    capi = _capi()
    ctx = _dense_ctx(160, batch=4)
    try:
        run_batch(ctx, 1, ec.BATCH_MIXED, True, capi.update_form(capi.UPDATE_DENSE_REG, ntm=16), DENSE)
    finally:
        ctx.close()


def test_batch_dense_gemm64():
    """nine filters, n_max = 128: both products on k_gemm64"""
    capi = _capi()
    ctx = _dense_ctx(128, batch=9)
    try:
        run_batch(ctx, 0, ec.BATCH_GEMM64, True, capi.update_form(capi.UPDATE_DENSE_REG, ntm=12, gemm64=True), DENSE)
    finally:
        ctx.close()


def test_batch_dense_split_sweep(orc):
    """29 filters of 257 .. 287 rows in a 288-row workspace with n_max = 256: 29 x 9 carried row blocks >= 256, the sweep splits
    (k_chol_carried).  Filters 0, 7, 8, 28 against the 80-bit reference, the rest against the float64 oracle (host time)"""
    capi = _capi()
    ctx = _dense_ctx(256, batch=29)
    try:
        wants = [ec.expected(c) if i in ec.BATCH_SPLIT_LD else oracle_update(orc, c) for i, c in enumerate(ec.BATCH_SPLIT)]
        run_batch(ctx, 0, ec.BATCH_SPLIT, False, capi.update_form(capi.UPDATE_DENSE_SWEEP, gemm64=True, split=True), DENSE, wants=wants)
    finally:
        ctx.close()


# ---- S not positive definite ------------------------------------------------------------------------------------------------------------
def _npd_ctx(route, ctx_batch):
    return (ctx_batch, False) if route == "lds" else (_dense_ctx(65, batch=4), True)


def _npd_form(route):
    capi = _capi()
    return {"lds": capi.UPDATE_LDS, "reg": capi.update_form(capi.UPDATE_DENSE_REG, ntm=8), "sweep": capi.update_form(capi.UPDATE_DENSE_SWEEP)}[route]


@pytest.mark.parametrize("kind", ["scalar", "full"])
@pytest.mark.parametrize("route", ["lds", "reg", "sweep"])
def test_not_pd_single(ctx_batch, route, kind):
    """INGVIO_E_NOT_PD: the filter's covariance bit-identical, dx zero (ingvio_hip.h)"""
    capi = _capi()
    c = ec.NOT_PD[route]
    ctx, own = _npd_ctx(route, ctx_batch)
    try:
        d = _set(ctx, 1, c)
        before = _others(ctx, -1)
        rc, dx = raw_update(ctx, 1, d, ec.not_pd_noise(c.m, kind))
        assert rc == capi.E_NOT_PD and ctx.last_update_form() == _npd_form(route), (rc, hex(ctx.last_update_form()))
        assert not dx.any() and _others_same(ctx, before)
        run_single(ctx, 1, c, _npd_form(route), TIGHT if route == "lds" else DENSE)      # and the context goes on working
    finally:
        if own:
            ctx.close()


@pytest.mark.parametrize("kind", ["scalar", "diag"])
@pytest.mark.parametrize("route", ["lds", "reg", "sweep"])
def test_not_pd_batch(ctx_batch, route, kind):
    """the failing filter between two sound ones: its status INGVIO_E_NOT_PD, its covariance bit-identical, its dx zero; the
    neighbours updated as if alone"""
    capi = _capi()
    bad = ec.NOT_PD[route]
    first, last = ec.NOT_PD_NEIGHBOURS[route][kind]
    ctx, own = _npd_ctx(route, ctx_batch)
    try:
        blocks = []
        for i, c in enumerate((first, bad, last)):
            d = _set(ctx, 1 + i, c)
            blocks.append((d["vidx"], d["vsize"], d["H"], d["res"], ec.not_pd_noise(c.m, kind) if c is bad else d["R"]))
        before = {b: ctx.cov_get(b) for b in range(ctx.batch) if b not in (1, 3)}      # the failing filter 2 and those outside the call
        rc, dx, st = raw_update_batch(ctx, 1, blocks, kind == "diag")
        form = _npd_form(route)
        assert rc == capi.E_NOT_PD and list(st) == [0, capi.E_NOT_PD, 0] and ctx.last_update_form() == form, (rc, st, hex(ctx.last_update_form()))
        assert not dx[1].any() and _others_same(ctx, before)
        for i, c in ((0, first), (2, last)):
            _check("%s beside a failing filter" % c.name, form, ctx.cov_get(1 + i), dx[i, :c.n], ec.expected(c), TIGHT if route == "lds" else DENSE)
    finally:
        if own:
            ctx.close()


# ---- gates ------------------------------------------------------------------------------------------------------------------------------
def _gamma_ok(label, g, want):
    e = abs(g - want) / max(1.0, want)
    WORST_GAMMA[0] = max(WORST_GAMMA[0], e)
    assert e < TOL_GAMMA, "%s: gamma %r against %r, error %.2e (< %.0e max(1, gamma)); worst so far %.2e" % (label, g, want, e, TOL_GAMMA, WORST_GAMMA[0])


@pytest.mark.parametrize("c", ec.GATE_CASES, ids=lambda c: c.name)
def test_chi2_gamma(ctx_lds, c):
    d = _set(ctx_lds, 3, c)
    before = _others(ctx_lds, -1)
    g = ctx_lds.chi2_gamma(3, d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
    _gamma_ok(c.name, g, ec.expected(c)[2])
    assert _others_same(ctx_lds, before)              # a gate writes no covariance, the gated filter's included


def test_chi2_gamma_multi(ctx_lds):
    """40 gates of mixed (m, nc) in one launch, each against the reference and against the single call"""
    c = ec.GATE_CASES[0]
    d = _set(ctx_lds, 3, c)
    blocks = ec.gate_multi_blocks(d["P"])
    var = 0.0123
    before = _others(ctx_lds, -1)
    gam = ctx_lds.chi2_gamma_multi(3, blocks, var)
    assert len({(b[2].shape) for b in blocks}) >= 30
    for i, (vo, vs, H, res) in enumerate(blocks):
        want = ec.reference_update(d["P"], vo, vs, H, res, np.float64(var))[2]
        _gamma_ok("block %d (m %d, nc %d)" % (i, *H.shape), gam[i], want)
        single = ctx_lds.chi2_gamma(3, vo, vs, H, res, var)
        assert abs(single - gam[i]) < TOL_GAMMA * max(1.0, want), (i, single, gam[i])
    assert _others_same(ctx_lds, before)


def test_chi2_gamma_capacity(ctx_cap):
    """8 (nc m + (m + 1)^2) <= 150 KB: at m = 128 nineteen columns fit, twenty are refused with nothing written"""
    capi = _capi()
    c = ec.GATE_FIT
    d = _set(ctx_cap, 1, c)
    before = _others(ctx_cap, -1)
    g = ctx_cap.chi2_gamma(1, d["vidx"], d["vsize"], d["H"], d["res"], d["R"])
    _gamma_ok(c.name, g, ec.expected(c)[2])
    gm = ctx_cap.chi2_gamma_multi(1, [(d["vidx"], d["vsize"], d["H"], d["res"])], 0.02)
    _gamma_ok(c.name + " (multi)", gm[0], ec.reference_update(d["P"], d["vidx"], d["vsize"], d["H"], d["res"], np.float64(0.02))[2])
    # one more column
    named = set(ec._cols(d["vidx"], d["vsize"]).tolist())
    free = next(j for j in range(c.n) if j not in named)
    vo, vs = d["vidx"] + [free], d["vsize"] + [1]
    H = np.asfortranarray(np.hstack([d["H"], np.ones((c.m, 1))]))
    Rb, kind = ctx_cap._R(d["R"], c.m)
    out = C.c_double(-3.0)
    vi, vsz, r = capi.i32(vo), capi.i32(vs), capi.f64(d["res"])
    rc = ctx_cap.L.ingvio_chi2_gamma(ctx_cap.h, 1, capi._i(vi), capi._i(vsz), len(vi), capi._d(H), c.m, c.m, capi._d(r), capi._d(Rb), kind, C.byref(out))
    assert rc == capi.E_CAPACITY and out.value == -3.0
    with pytest.raises(capi.IngvioError) as e:
        ctx_cap.chi2_gamma_multi(1, [(vo, vs, H, d["res"])], 0.02)
    assert e.value.code == capi.E_CAPACITY and _others_same(ctx_cap, before)
