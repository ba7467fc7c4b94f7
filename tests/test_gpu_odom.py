"""Odometry output of the device-resident loop (include/ingvio_hip.h: ingvio_odom_begin / _end, ingvio_cov_get_marginal_batch;
kernels_odom.hip).  Every comparison goes through the C ABI against ingvio_nominal_get + ingvio_cov_get on a synchronised
context, fed to the host model ingvio_amd/odom.py (pinned on the CPU by tests/test_odom_model.py):
  values, cov_err, the diagonal's extremes, n, the GNSS scalars   bit for bit
  cov_pose, cov_vel                                               within 64 eps (|J| |S| |J|^T) entrywise - the dot-product bound of sums
                                                                  of <= 18 terms with room for fused operations - and exactly symmetric
  records of the pipelined loop against those of the serial loop  bit for bit, every field"""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from ingvio_amd import closed_loop as cl
from ingvio_amd import closed_loop_gnss as cg
from ingvio_amd import closed_loop_lm as clm
from ingvio_amd import closed_loop_tail as clt
from ingvio_amd import closed_loop_update as clu
from ingvio_amd import odom
from ingvio_amd.closed_loop_odom import OdomForm
from nominal_helpers import device_state, refused, same_state, table_ctx

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
F = 24
EXACT = ("R_i2w", "p", "v", "bg", "ba", "R_c2i", "p_c2i", "gnss", "cov_err", "diag_min", "diag_max")
SE23, SE3, VEC3, SCALAR, LM = cl.SE23, cl.SE3, cl.VEC3, cl.SCALAR, cl.LM


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).reshape(-1).view(np.uint64)


def same_bits(a, b, what=""):
    """two records of the device, every field bit for bit"""
    assert (a["n"], a["status"], a["gnss_mask"]) == (b["n"], b["status"], b["gnss_mask"]), what
    for k in EXACT + ("cov_pose", "cov_vel"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def against_model(dev, ref, what="", eucl=True):
    """a record of the device against odom_model of the getters' data"""
    assert (dev["n"], dev["status"], dev["gnss_mask"]) == (ref["n"], ref["status"], ref["gnss_mask"]), (what, dev["status"], ref["status"])
    for k in EXACT:
        assert np.array_equal(bits(dev[k]), bits(ref[k])), (what, k)
    if not eucl:
        return 0.0
    worst = 0.0
    for k, bound in zip(("cov_pose", "cov_vel"), odom.eucl_bound(ref)):
        err = np.abs(dev[k] - ref[k])
        assert np.all(err <= 64 * EPS * bound), (what, k, float((err / np.maximum(bound, 1e-300)).max() / EPS))
        assert np.array_equal(bits(dev[k]), bits(dev[k].T)), (what, k)
        if bound.max() > 0:
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max() / EPS))
    return worst


def model_records(ctx, what=odom.ALL, b0=0, nb=None):
    """odom_model of ingvio_nominal_get + ingvio_cov_get (both synchronise)"""
    nb = ctx.batch - b0 if nb is None else nb
    nom, slots = ctx.nominal_get(b0, nb), ctx.nominal_get_gnss(b0, nb)
    return [odom.odom_model(nom[i], ctx.cov_get(b0 + i), ctx.n(b0 + i), slots[i], what) for i in range(nb)]


def records(ctx, b0=0, nb=None, what=odom.ALL):
    ctx.odom_begin(b0, nb, what)
    return ctx.odom_end()


# ---- 1. the record against the getters ---------------------------------------------------------------------------------------------
def spd(n, rng):
    A = rng.normal(size=(n, n))
    return A @ A.T / n + np.diag(rng.uniform(0.5, 2.0, n))


def make_table(layout, roles, rng):
    """layout: (kind, idx) per slot; roles: v_ext, v_pose, v_bg, v_ba; every SE3 slot other than the extrinsics is a window clone"""
    n = len(layout)
    val = np.zeros((n, 15))
    for s, (kind, _) in enumerate(layout):
        if kind in (SE23, SE3):
            val[s, 0:9] = np.linalg.qr(rng.normal(size=(3, 3)))[0].reshape(9)
        val[s, 9:12] = rng.normal(size=3) * 50.0
        if kind == SE23:
            val[s, 12:15] = rng.normal(size=3) * 5.0
        if kind == SCALAR:
            val[s, 10:12] = 0.0
    clones = [s for s, (kind, _) in enumerate(layout) if kind == SE3 and s != roles["v_ext"]]
    return dict(kind=[k for k, _ in layout], idx=[i for _, i in layout], anchor=[-1] * n, val=val, clone_var=clones, gravity=[0.0, 0.0, -9.8], **roles)


STD = dict(v_pose=0, v_bg=1, v_ba=2, v_ext=3)


def standard(n_clones, extra=()):
    return [(SE23, 0), (VEC3, 9), (VEC3, 12), (SE3, 15)] + [(SE3, 21 + 6 * q) for q in range(n_clones)] + list(extra)


def set_filters(ctx, tables, ns, rng):
    ctx.nominal_create(32)
    ctx.nominal_set(0, tables)
    for b, n in enumerate(ns):
        ctx.cov_set(b, spd(n, rng))


@pytest.fixture(scope="module")
def filters():
    """seven filters of one context (c_max 12, n_max 256): n = 21 without a clone, 39, 87, 249 (the diagonal scan loops, ldp != n), one with
    the extrinsics first, the pose at idx 6, bg behind a scalar and ba last, one with three GNSS scalars registered, one with v_bg = -1;
    and two filters with n = 141 in a context with c_max 20 (the large-window layout)"""
    from ingvio_amd import capi
    rng = np.random.default_rng(77)
    ctx = capi.Context(batch=7, n_max=256, c_max=12, f_max=8, m_max=32)
    tabs = [make_table(standard(0), STD, rng), make_table(standard(3), STD, rng), make_table(standard(11), STD, rng),
            make_table(standard(12), STD, rng),
            make_table([(SE3, 0), (SE23, 6), (SCALAR, 15), (VEC3, 16), (SE3, 19), (VEC3, 25)], dict(v_ext=0, v_pose=1, v_bg=3, v_ba=5), rng),
            make_table(standard(0, [(SCALAR, 21), (SCALAR, 22), (SCALAR, 23)]), STD, rng),
            make_table(standard(0), dict(STD, v_bg=-1), rng)]
    ns = [21, 39, 87, 249, 28, 24, 21]
    set_filters(ctx, tabs, ns, rng)
    ctx.nominal_set_gnss(5, [[4, -1, 5, -1, -1, 6]])
    assert ctx.ldp != 249
    big = capi.Context(batch=2, n_max=160, c_max=20, f_max=8, m_max=32)
    set_filters(big, [make_table(standard(20), STD, rng) for _ in range(2)], [141, 141], rng)
    yield ctx, big, ns
    ctx.close(); big.close()


def test_record_equals_the_getters(filters):
    ctx, big, ns = filters
    for name, c in (("c_max 12", ctx), ("c_max 20", big)):
        ref, dev = model_records(c), records(c)
        assert len(dev) == c.batch
        for b, (d, r) in enumerate(zip(dev, ref)):
            worst = against_model(d, r, (name, b))
            print("%s filter %d: n %d status %d, congruences within %.2f eps |J||S||J|^T" % (name, b, d["n"], d["status"], worst))
            assert d["status"] == (odom.ABSENT if (c is ctx and b == 6) else 0), (name, b)
            assert d["diag_min"] > 0 and d["cov_pose"].any() and d["cov_vel"].any()
    dev = records(ctx)
    assert [d["n"] for d in dev] == ns
    assert dev[5]["gnss_mask"] == 0b100101 and dev[5]["gnss"][[0, 2, 5]].all() and not dev[5]["gnss"][[1, 3, 4]].any()
    assert not dev[6]["bg"].any() and not dev[6]["cov_err"][9:12].any() and dev[6]["ba"].any() and dev[6]["cov_err"][12:15, 12:15].any()
    assert not dev[6]["cov_err"][:, 9:12].any()


def test_partial_range_leaves_the_rest_of_out_alone(filters):
    from ingvio_amd import capi
    ctx = filters[0]
    ref = model_records(ctx, b0=2, nb=3)
    raw = (capi.Odom * 7)()
    C.memset(raw, 0xAB, C.sizeof(raw))
    ctx.odom_begin(2, 3)
    dev = ctx.odom_end(raw)
    assert len(dev) == 3
    for i in range(3):
        against_model(dev[i], ref[i], i)
    tail = bytes(raw)[3 * C.sizeof(capi.Odom):]
    assert tail == b"\xab" * len(tail)


@pytest.mark.parametrize("what", [0, odom.COV, odom.EUCL, odom.DIAG, odom.COV | odom.DIAG])
def test_fields_that_were_not_requested_are_zero(filters, what):
    ctx = filters[0]
    ref, dev = model_records(ctx, what), records(ctx, what=what)
    for b, (d, r) in enumerate(zip(dev, ref)):
        against_model(d, r, (what, b))
        assert d["p"].any()
        assert d["cov_err"].any() == bool(what & (odom.COV | odom.EUCL))
        assert d["cov_pose"].any() == bool(what & odom.EUCL) and d["cov_vel"].any() == bool(what & odom.EUCL)
        assert (d["diag_max"] != 0.0) == bool(what & odom.DIAG)


# ---- 2. status ---------------------------------------------------------------------------------------------------------------------
def test_status_bits_from_plain_data():
    from ingvio_amd import capi
    rng = np.random.default_rng(78)
    ctx = capi.Context(batch=3, n_max=48, c_max=11, f_max=8, m_max=32)
    Ps = [spd(39, rng) for _ in range(3)]
    Ps[1][30, 30] = -0.25                                                # outside the 15 x 15 block
    Ps[2][4, 10] = Ps[2][10, 4] = np.inf                                 # inside it
    ctx.nominal_create(16)
    ctx.nominal_set(0, [make_table(standard(3), STD, rng) for _ in range(3)])
    for b, P in enumerate(Ps):
        ctx.cov_set(b, P)
    dev, ref = records(ctx), model_records(ctx)
    assert [d["status"] for d in dev] == [0, odom.NEG_DIAG, odom.NONFINITE]
    assert dev[1]["diag_min"] == -0.25
    for b in range(3):
        against_model(dev[b], ref[b], b, eucl=b != 2)
    ctx.close()


# ---- 3. the closed loop ------------------------------------------------------------------------------------------------------------
def run_loop(ctx, cases, n_frames, pipelined, form, getters=False):
    """-> (frame results, records per frame or None, model records per frame (getters), final state)"""
    loop = cl.DeviceLoop(ctx, cases, range(n_frames), form, pipelined=pipelined)
    loop.start()
    frames, recs, refs = [], [], []
    for f in range(n_frames):
        out = loop.frame(f)
        if isinstance(form, OdomForm):
            fr, res = out
            inner, rec = res if isinstance(res, tuple) else (None, res)
            frames.append((fr, inner)); recs.append(rec)
        else:
            frames.append((out[0], out[1]) if isinstance(out[0], tuple) else (out, None))
        if getters:
            refs.append(model_records(ctx))
    return frames, recs, refs, device_state(ctx, len(cases))


def same_frames(cases, a, b):
    for f, ((fa, _), (fb, _)) in enumerate(zip(a, b)):
        assert np.array_equal(bits(fa[0]), bits(fb[0])) and np.array_equal(fa[2], fb[2]), f
        for i, c in enumerate(cases):                                    # accept flags exist for the frame's features only
            nf = len(c["frames"][f]["delta"]["feat_track"])
            assert np.array_equal(fa[1][i, :nf], fb[1][i, :nf]), (f, i)


def test_pipelined_loop_records_equal_the_serial_loop():
    """8 filters x 8 frames, windows 5 ... 11, k in {1, 9, 10, 33}: the record of frame i is taken behind run(i) and in front of the
    asynchronous stage of frame i + 1, whose IMU steps advance R, p and v in the table"""
    B, N = 8, 8
    cases = cl.make_loop(B, N)
    assert sorted({c["C"] for c in cases}) == list(range(5, 12))
    ctx = table_ctx(cases, F)
    fs, rs, ref, ss = run_loop(ctx, cases, N, False, OdomForm(), getters=True)
    ctx.close()
    ctx = table_ctx(cases, F)
    fp, rp, _, sp = run_loop(ctx, cases, N, True, OdomForm())
    ctx.close()
    ctx = table_ctx(cases, F)
    f0, _, _, s0 = run_loop(ctx, cases, N, True, None)
    ctx.close()
    worst = 0.0
    for f in range(N):
        for b in range(B):
            same_bits(rp[f][b], rs[f][b], (f, b))
            worst = max(worst, against_model(rp[f][b], ref[f][b], (f, b)))
            assert rp[f][b]["status"] == 0
        if f:
            assert any(not np.array_equal(rp[f][b]["p"], rp[f - 1][b]["p"]) for b in range(B))
    print("congruences within %.2f eps |J||S||J|^T" % worst)
    same_frames(cases, fp, f0); same_frames(cases, fp, fs)
    same_state(sp, s0); same_state(sp, ss)


# ---- 4. late forms -----------------------------------------------------------------------------------------------------------------
def late_loop(cases, make_form, make_ctx, N):
    res = []
    for pipelined in (False, True):
        ctx = make_ctx()
        res.append(run_loop(ctx, cases, N, pipelined, OdomForm(make_form()), getters=not pipelined))
        ctx.close()
    (fs, rs, ref, ss), (fp, rp, _, sp) = res
    for f in range(N):
        for b in range(len(cases)):
            same_bits(rp[f][b], rs[f][b], (f, b))
            against_model(rp[f][b], ref[f][b], (f, b))
    same_frames(cases, fp, fs)
    same_state(sp, ss)
    return rp, ref


def test_record_behind_the_gnss_update():
    from ingvio_amd import synth
    B, N = 4, 4
    cases = cg.make_gnss_loop(load_golden("gnss_front"), B, N, every=0)
    chi2 = synth.chi2_table()
    rp, _ = late_loop(cases, lambda: cg.GnssForm(chi2), lambda: table_ctx(cases, F, gnss=True), N)
    assert all(r["gnss_mask"] for r in rp[0])
    # the record carries the GNSS update's boxPlus: it differs from the one a plain loop takes behind the frame's run
    ctx = table_ctx(cases, F, gnss=True)
    plain = run_loop(ctx, cases, 1, False, OdomForm())[1]
    ctx.close()
    assert any(not np.array_equal(plain[0][b]["p"], rp[0][b]["p"]) for b in range(B))


def test_record_behind_the_tail():
    B, N, L = 4, 4, 2
    cases = clt.make_tail_loop(B, N, L=L, F=F, mode="sw")

    def make_ctx():
        from ingvio_amd import capi
        n_max = max(c["P"].shape[0] for c in cases) + 12
        ctx = capi.Context(batch=B, n_max=((n_max + 15) // 16) * 16, c_max=12, f_max=F, m_max=64)
        for b, c in enumerate(cases):
            ctx.cov_set(b, c["P"])
        ctx.tracks_create(F)
        ctx.nominal_create(48)
        ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
        return ctx
    rp, ref = late_loop(cases, lambda: clt.TailForm(clm.lm_opts(), cases), make_ctx, N)
    n0 = [c["P"].shape[0] for c in cases]
    for f in range(N):                                                   # n in the record follows the tail's drop: the clone that
        for b in range(B):                                               # came with the frame and the one the tail dropped cancel,
            assert rp[f][b]["n"] == ref[f][b]["n"] <= n0[b]               # a landmark that left takes 3 more
    assert any(rp[N - 1][b]["n"] < n0[b] for b in range(B))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def no(ctx, fn, with_table=True):
    from ingvio_amd import capi
    if with_table:
        return refused(ctx, fn, capi.E_ARG, sizes=True)
    before = [(ctx.n(b), ctx.cov_get(b)) for b in range(ctx.batch)]
    with pytest.raises(capi.IngvioError) as e:
        fn()
    assert e.value.code == capi.E_ARG
    for b, (n, P) in enumerate(before):
        assert ctx.n(b) == n and np.array_equal(ctx.cov_get(b), P)


def test_refused_without_a_table():
    cases = cl.make_loop(2, 1)
    ctx = cl.loop_ctx(cases, F)
    no(ctx, ctx.odom_begin, with_table=False)
    no(ctx, ctx.odom_end, with_table=False)
    ctx.close()


def landmark_scenario(ctx, cases, refuse):
    """frames with the in-frame landmark stage; -> the records and frame results it produced"""
    o = clm.lm_opts()
    out = []
    if refuse:
        no(ctx, lambda: ctx.odom_begin(0, None, 8))                      # an unknown bit
        no(ctx, lambda: ctx.odom_begin(1, 2))                            # a bad range
        no(ctx, ctx.odom_end)                                            # nothing pending
    for f in range(2):
        cl.nominal_stage(ctx, cases, f)()
        if refuse:
            no(ctx, ctx.odom_begin)                                      # a frame staged from the table has not run
        clm.lm_stage_call(ctx, cases, f, o, in_frame=True)()
        if refuse:
            no(ctx, ctx.odom_begin)                                      # ... and its in-frame landmark stage
        ctx.frame_run()
        ctx.odom_begin()
        if refuse:
            no(ctx, ctx.odom_begin)                                      # a second _begin
        out.append((ctx.frame_fetch(), ctx.landmark_fetch(), ctx.odom_end()))
        if refuse:
            no(ctx, ctx.odom_end)
    return out


def gnss_scenario(ctx, cases, refuse):
    from ingvio_amd import synth
    cl.nominal_stage(ctx, cases, 0)()
    ctx.frame_run()
    fr = ctx.frame_fetch()
    cg.gnss_stage_call(ctx, cases, 0, synth.chi2_table())()
    if refuse:
        no(ctx, ctx.odom_begin)                                          # a GNSS epoch staged from the table has not run
    ctx.gnss_run()
    ctx.odom_begin()
    return [(fr, ctx.gnss_fetch(), ctx.odom_end())]


def update_scenario(ctx, cases, refuse):
    out = []
    for stage in (cl.nominal_stage(ctx, cases, 0), clu.update_stage(ctx, cases, 0)):
        stage()
        if refuse:
            no(ctx, ctx.odom_begin)                                      # a frame / an update-only frame staged from the table
        ctx.frame_run()
        ctx.odom_begin()
        out.append((ctx.frame_fetch(), None, ctx.odom_end()))
    return out


def flat(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [v for y in x for v in flat(y)]
    return [] if x is None else [np.asarray(x)]


@pytest.mark.parametrize("which", ["landmarks", "gnss", "update"])
def test_refusals_change_nothing_and_the_loop_continues(which):
    """every refusal is INGVIO_E_ARG with P, table and n unchanged bit for bit, and the context then produces what a context that was
    never refused produces: frame results, records and the final state"""
    if which == "landmarks":
        cases, scenario, make_ctx = clm.make_lm_loop(2, 2), landmark_scenario, lambda: table_ctx(cases, F)
    elif which == "gnss":
        cases = cg.make_gnss_loop(load_golden("gnss_front"), 2, 1, every=0)
        scenario, make_ctx = gnss_scenario, lambda: table_ctx(cases, F, gnss=True)
    else:
        cases, scenario, make_ctx = clu.make_update_loop(2, 1, F), update_scenario, lambda: table_ctx(cases, F)
    res = []
    for refuse in (False, True):
        ctx = make_ctx()
        out = scenario(ctx, cases, refuse)
        res.append((out, device_state(ctx, 2), [ctx.n(b) for b in range(2)]))
        ctx.close()
    (o0, s0, n0), (o1, s1, n1) = res
    def compared(out):                                                   # dx and rows of the frame, dx of the form's update, the records
        return flat([(o[0][0], o[0][2], None if o[1] is None else o[1][0], o[2]) for o in out])
    a, b = compared(o0), compared(o1)
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and (np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y))
    same_state(s0, s1)
    assert n0 == n1


def test_refused_between_the_halves_of_a_split_step():
    from ingvio_amd import capi, host, synth
    ctx = capi.Context(batch=2, n_max=112, c_max=11, f_max=32, m_max=32)
    cases = [synth.build_case(lambda P, b=b: capi.DeviceCov(ctx, b, P), host.imu_transition, seed=b, F=32, n_gnss=0, n_landmarks=0) for b in range(2)]
    ctx.tracks_create(32); ctx.nominal_create(16)
    ctx.snapshot()
    ctx.frame_stage(0, [c[1] for c in cases], [c[2] for c in cases], cases[0][1]["sigma"])
    ctx.frame_run_phase(1, restore_prior=True)
    with pytest.raises(capi.IngvioError) as e:
        ctx.odom_begin()
    assert e.value.code == capi.E_ARG and "split" in str(e.value)
    ctx.frame_run_phase(2)
    ctx.frame_fetch()
    assert len(records(ctx)) == 2
    ctx.close()


# ---- 6. snapshot / restore ---------------------------------------------------------------------------------------------------------
def test_record_after_restore_equals_the_record_at_the_snapshot():
    B = 4
    cases = cl.make_loop(B, 3)
    ctx = table_ctx(cases, F)
    r0 = records(ctx)
    ctx.snapshot()
    run_loop(ctx, cases, 3, False, None)
    moved = records(ctx)
    ctx.restore()
    r1 = records(ctx)
    for b in range(B):
        same_bits(r0[b], r1[b], b)
        assert not np.array_equal(moved[b]["p"], r0[b]["p"])
    ctx.close()


# ---- 7. ingvio_cov_get_marginal_batch ----------------------------------------------------------------------------------------------
def test_marginal_batch_equals_the_single_getter(filters):
    from ingvio_amd import capi
    ctx, big, ns = filters
    lists = [([0, 9, 12], [9, 3, 3]), ([0, 21, 27, 33], [9, 6, 6, 6]), ([40], [1]), ([240, 5, 3], [9, 0, 6]), ([25, 6], [3, 9])]
    for ns_max in (None, 33, capi.MARGINAL_NS_MAX):
        blocks = ctx.cov_get_marginal_batch(0, lists, ns_max)
        for b, ((vi, vs), blk) in enumerate(zip(lists, blocks)):
            assert blk.shape[0] == sum(vs) and np.array_equal(bits(blk), bits(ctx.marginal(b, vi, vs))), (ns_max, b)
    blocks = ctx.cov_get_marginal_batch(2, lists[2:4])                   # a sub-range
    assert np.array_equal(blocks[1], ctx.marginal(3, *lists[3]))
    blk = big.cov_get_marginal_batch(1, [([0, 135, 9], [9, 6, 6])])[0]
    assert np.array_equal(bits(blk), bits(big.marginal(1, [0, 135, 9], [9, 6, 6])))
    # no table is needed
    plain = capi.Context(batch=2, n_max=32, c_max=11, f_max=8, m_max=32)
    P = spd(20, np.random.default_rng(3))
    plain.cov_set(0, P); plain.cov_set(1, P[:12, :12])
    got = plain.cov_get_marginal_batch(0, [([3, 15], [2, 5]), ([6], [6])])
    assert np.array_equal(got[0], P[np.ix_([3, 4, 15, 16, 17, 18, 19], [3, 4, 15, 16, 17, 18, 19])]) and np.array_equal(got[1], P[6:12, 6:12])
    plain.close()


def test_marginal_batch_refuses_a_list_beyond_n_and_writes_nothing(filters):
    from ingvio_amd import capi
    ctx = filters[0]
    vidx = capi.i32([[0, 9], [36, 0], [0, 9]])                           # filter 1 has n = 39: 36 + 6 > 39
    vsize = capi.i32([[9, 3], [6, 9], [9, 3]])
    out = np.full((3, 15 * 15), 7.5)
    rc = ctx.L.ingvio_cov_get_marginal_batch(ctx.h, 0, 3, capi._i(vidx), capi._i(vsize), 2, 15, capi._d(out))
    assert rc == capi.E_NOT_IN_STATE and np.all(out == 7.5)
    for bad in (dict(ns_max=0), dict(ns_max=capi.MARGINAL_NS_MAX + 1), dict(ns_max=11)):      # 12 columns do not fit 11
        rc = ctx.L.ingvio_cov_get_marginal_batch(ctx.h, 0, 1, capi._i(vidx), capi._i(vsize), 2, bad["ns_max"], capi._d(out))
        assert rc == capi.E_ARG and np.all(out == 7.5)
