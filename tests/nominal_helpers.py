"""What the tests of the device-resident nominal state share (tests/test_gpu_nominal_*.py): a context with the loop's tables set, the
device state's snapshot and its comparisons."""
import numpy as np
import pytest

from conftest import rel_err
from ingvio_amd.closed_loop import NONE, loop_ctx

TABLE_KEYS = ("kind", "idx", "anchor", "val", "clone_var")


def table_ctx(cases, F=24, gnss=False):
    """a fresh context with the cases' covariances and tables set; gnss: their clock slots registered"""
    ctx = loop_ctx(cases, F)
    ctx.nominal_create(48)
    ctx.nominal_set(0, [c["table"].as_dict() for c in cases])
    if gnss:
        ctx.nominal_set_gnss(0, [c["gnss_slots"] for c in cases])
    return ctx


def assert_table(dev, host, tol, what):
    """the device table (ingvio_nominal_get) against a HostTable; -> the worst relative error of a value"""
    h = host.as_dict()
    n = len(h["kind"])
    assert list(dev["kind"][:n]) == list(h["kind"]) and all(k == NONE for k in dev["kind"][n:]), what
    worst = 0.0
    for i in range(n):
        if h["kind"][i] == NONE:
            continue
        assert dev["idx"][i] == h["idx"][i] and dev["anchor"][i] == h["anchor"][i], (what, i)
        worst = max(worst, rel_err(dev["val"][i], h["val"][i]))
        assert rel_err(dev["val"][i], h["val"][i]) <= tol, (what, i, rel_err(dev["val"][i], h["val"][i]))
    assert list(dev["clone_var"]) == list(h["clone_var"]), what
    return worst


def device_state(ctx, B):
    return ctx.nominal_get(), [ctx.cov_get(b) for b in range(B)]


def same_state(s0, s1, keys=TABLE_KEYS, what=""):
    for b in range(len(s0[1])):
        for key in keys:
            assert np.array_equal(s0[0][b][key], s1[0][b][key]), (what, b, key)
        assert np.array_equal(s0[1][b], s1[1][b]), (what, b)


def refused(ctx, fn, code, sizes=False):
    """fn raises IngvioError(code) and leaves tables and covariances (sizes: and every filter's n) as they were"""
    from ingvio_amd import capi
    B = ctx.batch

    def state():
        return device_state(ctx, B), [ctx.n(b) for b in range(B)] if sizes else None
    s0 = state()
    with pytest.raises(capi.IngvioError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code, str(e.value))
    s1 = state()
    same_state(s0[0], s1[0])
    assert s0[1] == s1[1]
