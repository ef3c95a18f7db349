"""Host side of shared-catalog queries (dp_lower_solve_shared): the expanded
64-bit wire dp_expand_shared makes -- problem p is catalog query_catalog[p]'s
variables followed by query p's -- lowers to byte-identical records, offsets,
identities and errors as the concatenated problems encoded one by one, and the
entry points refuse mismatched wires, out-of-range catalogs and NULL."""
import ctypes

import numpy as np
import pytest

from deppy_amd import _lib, sat
from tests.test_device_lowering import assert_same
from tests.test_lowering import EDGE, V, all_golden_variable_sets, variables_of

FLAGS = dict(narrow=True, packed=True)


def concatenated(catalogs, queries):
    return [(list(catalogs[b]) if b is not None else []) + list(q) for b, q in queries]


def golden_splits():
    """Every golden variable set split at every position into a catalog and a
    query, each pair a catalog of its own; then every set as a query without
    a catalog, a catalog no query uses, and one catalog under many queries."""
    catalogs, queries = [], []
    sets = [variables_of(vs) for vs in all_golden_variable_sets()] + [list(vs) for vs in EDGE]
    for vs in sets:
        for s in range(len(vs) + 1):
            catalogs.append(vs[:s])
            queries.append((len(catalogs) - 1, vs[s:]))
    queries += [(None, vs) for vs in sets]
    catalogs.append([V("unused", sat.Mandatory(), sat.Dependency("nowhere"))])
    many = len(catalogs)
    catalogs.append([V("a", sat.Conflict("b")), V("b"), V("c", sat.Dependency("q"))])
    tails = [[], [V("q")], [V("q", sat.Mandatory(), sat.AtMost(1, "a", "b"))], [V("a")],
             [V("q", sat.Dependency("a")), V("r", sat.Mandatory(), sat.Dependency("b", "zz"))]]
    queries += [(many, t) for t in tails * 3]
    return catalogs, queries


@pytest.mark.parametrize("ids16", [True, False])
def test_expanded_wire_lowers_like_the_concatenated_problems(ids16):
    catalogs, queries = golden_splits()
    k32, q32, qc = sat.encode_shared(catalogs, queries, pinned=False, ids16=ids16)
    assert k32.ids16 == q32.ids16 == ids16
    assert k32.n_problems == len(catalogs) and q32.n_problems == len(queries) == len(qc)
    assert qc.dtype == np.int32 and list(qc) == [-1 if b is None else b for b, _ in queries]
    used = np.bincount(qc[qc >= 0], minlength=len(catalogs))
    assert (used == 0).any() and (used == 1).any() and (used > 10).any()
    expanded = _lib.expand_shared(k32, q32, qc)
    direct = sat.encode_inputs(concatenated(catalogs, queries))
    # the same problems, variable for variable
    for k in ("prob_var_off", "var_con_off", "con_kind", "con_n", "con_arg_off"):
        np.testing.assert_array_equal(expanded.a[k], direct.a[k], err_msg=k)
    got, ref = _lib.Lowered(expanded, **FLAGS), _lib.Lowered(direct, **FLAGS)
    assert_same(got, ref)
    assert set(np.unique(ref.err)) == {0, 1, 2}  # duplicates across the seam and lookups among them


def test_expanded_wire_of_a_range():
    """Offsets are absolute: a catalogs' wire that is a range of a larger one."""
    catalogs, queries = golden_splits()
    k32, q32, qc = sat.encode_shared(catalogs, queries, pinned=False)
    whole = _lib.expand_shared(k32, q32, qc)
    skip = 7
    sub = _lib.Wire32Arrays.__new__(_lib.Wire32Arrays)
    sub.__dict__.update({k: v for k, v in k32.__dict__.items() if k != "_struct"})
    sub.a = dict(k32.a)
    for k in ("prob_var_off", "prob_con_off", "prob_arg_off"):
        sub.a[k] = np.ascontiguousarray(k32.a[k][skip:])
    # (queries of the catalogs left out stand alone)
    moved = np.where(qc >= skip, qc - skip, -1).astype(np.int32)
    part = _lib.expand_shared(sub, q32, moved)
    direct = sat.encode_inputs(concatenated(catalogs, [(b if b is not None and b >= skip else None, q)
                                                       for b, q in queries]))
    assert_same(_lib.Lowered(part, **FLAGS), _lib.Lowered(direct, **FLAGS))
    assert whole.n_problems == part.n_problems == len(queries)
    assert sub.n_problems == len(catalogs) - skip and (moved >= 0).any()


def small_shared(ids16=True):
    catalogs = [[V("a", sat.Conflict("b")), V("b")], [V("c", sat.Mandatory())]]
    queries = [(0, [V("q", sat.Dependency("a"))]), (1, [V("q")]), (None, [V("z")])]
    return sat.encode_shared(catalogs, queries, pinned=False, ids16=ids16)


def call_both(k32, q32, qc):
    """(dp_lower_solve_shared's return with a NULL lowerer never reaches the
    checks, so the wires are checked through the expand hook and, for the
    texts, through both.)"""
    with pytest.raises(ValueError) as e:
        _lib.expand_shared(k32, q32, qc)
    return str(e.value)


def test_out_of_range_query_catalog_is_rejected():
    k32, q32, qc = small_shared()
    for bad in (2, -2, 1 << 30):
        x = qc.copy()
        x[1] = bad
        assert "query_catalog" in call_both(k32, q32, x)
    _lib.expand_shared(k32, q32, qc)  # (the wires themselves are fine)
    with pytest.raises(ValueError, match="one entry per query"):
        _lib.expand_shared(k32, q32, qc[:-1])


def test_mismatched_string_tables_are_rejected():
    k32, q32, qc = small_shared()
    other = _lib.Wire32Arrays(sat.encode_inputs([[V("a"), V("b"), V("more")]]), pinned=False)
    assert other.struct().n_strs != q32.struct().n_strs
    assert "string tables differ" in call_both(other, q32, np.array([0, 0, -1], np.int32))
    assert "string tables differ" in call_both(k32, other, np.array([0], np.int32))


def test_mixed_index_widths_are_rejected():
    k16, q16, qc = small_shared(True)
    k32, q32, _ = small_shared(False)
    assert k16.ids16 and not k32.ids16
    assert "index widths differ" in call_both(k16, q32, qc)
    assert "index widths differ" in call_both(k32, q16, qc)
    _lib.expand_shared(k32, q32, qc)


def test_offsets_that_are_not_monotone_are_rejected():
    k32, q32, qc = small_shared()
    for which, key in ((k32, "prob_var_off"), (q32, "prob_con_off"), (q32, "prob_arg_off")):
        saved = which.a[key].copy()
        which.a[key][1] = saved[-1] + 5
        assert "malformed wire batch" in call_both(k32, q32, qc)
        which.a[key][:] = saved
    _lib.expand_shared(k32, q32, qc)


def test_shared_entry_points_refuse_null():
    L = _lib.lib()
    k32, q32, qc = small_shared()
    ks, qs, so = k32.struct(), q32.struct(), _lib.Solved()
    pq = qc.ctypes.data_as(_lib.c_i32p)
    assert L.dp_lower_solve_shared(None, ctypes.byref(ks), ctypes.byref(qs), pq, ctypes.byref(so)) == -1
    msg = L.dp_last_global_error()
    assert b"dp_lower_solve_shared" in msg and b"null" in msg
    assert L.dp_lower_solve_shared(None, None, None, None, None) == -1
    for args in ((None, ctypes.byref(qs), pq), (ctypes.byref(ks), None, pq), (ctypes.byref(ks), ctypes.byref(qs), None)):
        assert not L.dp_expand_shared(*args)
        assert b"null" in L.dp_last_global_error()
    assert not L.dp_expanded_wire(None)
    L.dp_expanded_free(None)
