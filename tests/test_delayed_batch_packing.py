"""capi.make_delayed_blocks: the Python blocks of Context.add_variable_delayed_batch as the ingvio_delayed_block / ingvio_delayed_cand
structs of include/ingvio_hip.h (no GPU: the structs are read back field by field)."""
import ctypes as C
import os
import re

import numpy as np

from ingvio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blocks_to_structs():
    rng = np.random.default_rng(0)
    H_old = rng.standard_normal((8, 15)); H_new = rng.standard_normal((8, 3)); res = rng.standard_normal(8)
    H1 = rng.standard_normal((5, 9)); Hn1 = rng.standard_normal((5, 1)); r1 = rng.standard_normal(5)
    blocks = [[(np.array([0, 21]), [9, 6], H_old, H_new, res, 15.5), ([0], [9], H1, Hn1, r1)], [], [([21], [6], H_old[:, :6], H_new, res, None)]]
    arr, cap, keep = capi.make_delayed_blocks(blocks)
    assert cap == 2 and [arr[g].n_cand for g in range(3)] == [2, 0, 1] and not arr[1].cand
    q = arr[0].cand[0]
    assert (q.k, q.m, q.s, q.ldh, q.ldn, q.chi2_check) == (2, 8, 3, 8, 8, 15.5)
    assert [q.vidx[i] for i in range(2)] == [0, 21] and [q.vsize[i] for i in range(2)] == [9, 6]
    # column-major, leading dimension m: element (i, j) at i + j * ldh
    assert all(q.H_old[i + j * q.ldh] == H_old[i, j] for i in range(8) for j in range(15))
    assert all(q.H_new[i + j * q.ldn] == H_new[i, j] for i in range(8) for j in range(3))
    assert [q.res[i] for i in range(8)] == list(res)
    q = arr[0].cand[1]
    from scipy.stats import chi2
    assert (q.k, q.m, q.s, q.ldh, q.ldn) == (1, 5, 1, 5, 5) and q.chi2_check == float(chi2.ppf(0.95, 5))
    assert all(q.H_old[i + j * 5] == H1[i, j] for i in range(5) for j in range(9)) and [q.H_new[i] for i in range(5)] == list(Hn1[:, 0])
    q = arr[2].cand[0]
    assert (q.k, q.m, q.s) == (1, 8, 3) and q.vidx[0] == 21 and q.vsize[0] == 6 and q.chi2_check == float(chi2.ppf(0.95, 8))


def test_struct_layout_follows_the_header():
    """field order and types of the two ctypes structs == the typedefs of include/ingvio_hip.h"""
    text = open(os.path.join(ROOT, "include", "ingvio_hip.h")).read()
    ctype = {"const int*": C.POINTER(C.c_int), "const double*": C.POINTER(C.c_double), "int": C.c_int, "double": C.c_double,
             "const ingvio_delayed_cand*": C.POINTER(capi.DelayedCand)}
    for name, cls in (("ingvio_delayed_cand", capi.DelayedCand), ("ingvio_delayed_block", capi.DelayedBlock)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            m = re.match(r"(const \w+\*|\w+)\s+(.*)", decl)
            fields += [(nm.strip(), ctype[m.group(1)]) for nm in m.group(2).split(",")]
        assert [(n, t) for n, t in cls._fields_] == fields, name
    assert "ingvio_add_variable_delayed_batch" in capi.EXPORTS
