"""Search traces on the fused and shared-catalog paths (dp_lower_solve_traced,
dp_lower_solve_shared_traced).  The yardstick is test_lower_solve.py's,
traced: sat.solve_wire(wire64, ctx, trace_cap), the host lowering plus the
resident traced solve, with its trace, trace_len and the lowering's
ident_var / ident_con.  Every trace word and length equals it, every identity
word's owner is ident_var / ident_con of that identity, every other word has
the owner -1, and the results are the untraced call's."""
import io

import numpy as np
import pytest

from deppy_amd import _lib, sat
from tests import fixtures
from tests.test_device_lowering import assert_same, wire_of
from tests.test_lower_solve import RESULT_KEYS, assert_equal, colliding_problems, outcome, unsat_goldens
from tests.test_lower_solve_shared import (chain_catalog, concatenated, config2_shared, copied, empty_catalogs,
                                           seam_queries)
from tests.test_lowering import variables_of

pytestmark = pytest.mark.gpu

CAP = 4096
TRACE_KEYS = ("trace_off", "trace", "trace_var", "trace_con")
FMT = 13  # DP_H_FMT


@pytest.fixture(scope="module")
def dl():
    ctx = _lib.Context(0, 1)
    d = _lib.DeviceLowerer(ctx)
    yield d
    d.close()
    ctx.close()


def yardstick(wire, ctx, cap):
    """Host lowering + the resident traced solve, copied (test_lower_solve's
    yardstick with trace [P, cap] and trace_len [P])."""
    lw, res = sat.solve_wire(wire, ctx, cap)
    ref = {k: np.array(res[k]) for k in RESULT_KEYS + ("installed", "core", "trace", "trace_len")}
    ref.update(ident_off=np.array(lw.ident_off), ident_var=np.array(lw.ident_var), ident_con=np.array(lw.ident_con),
               err=np.array(lw.err), msg=list(lw.msg), fmt=np.array(lw.rec[lw.rec_off[:-1] + FMT]))
    return ref


_yardsticks = {}


def shared_yardstick(key, make_wire, ctx, cap):
    """One yardstick per (input, cap), computed once and left unchanged."""
    k = (key, cap)
    if k not in _yardsticks:
        _yardsticks[k] = yardstick(make_wire(), ctx, cap)
    return _yardsticks[k]


def expected_owners(ref, p):
    """The yardstick's trace of problem p and the owner of every word: the
    identity words of each event mapped through ident_var / ident_con, -1 at
    header and variable words and at an identity outside [0, nid)."""
    n = int(ref["trace_len"][p])
    t = ref["trace"][p][:n]
    var = np.full(n, -1, np.int32)
    con = np.full(n, -1, np.int32)
    i0, nid = int(ref["ident_off"][p]), int(ref["ident_off"][p + 1] - ref["ident_off"][p])
    i, words = 0, 0
    while i < n:
        nv = int(t[i])
        m = int(t[i + 1 + nv])
        a = i + 2 + nv
        ids = t[a:a + m]
        ok = (ids >= 0) & (ids < nid)
        var[a:a + m][ok] = ref["ident_var"][i0 + ids[ok]]
        con[a:a + m][ok] = ref["ident_con"][i0 + ids[ok]]
        words += m
        i = a + m
    assert i == n, "the yardstick's trace ends inside an event"
    return t, var, con, words


def assert_traced_equal(got, ref):
    """got (a traced fused call) against the traced yardstick: the results,
    then lengths, words and owners of every problem."""
    assert_equal(got, ref)
    n = len(ref["status"])
    assert len(got["trace_off"]) == n + 1 and got["trace_off"][0] == 0
    np.testing.assert_array_equal(np.diff(got["trace_off"]), ref["trace_len"])
    assert len(got["trace"]) == len(got["trace_var"]) == len(got["trace_con"]) == int(got["trace_off"][-1])
    ident_words = 0
    for p in np.flatnonzero(ref["trace_len"]):
        t, var, con, w = expected_owners(ref, p)
        a, b = int(got["trace_off"][p]), int(got["trace_off"][p + 1])
        np.testing.assert_array_equal(got["trace"][a:b], t, err_msg="trace of problem %d" % p)
        np.testing.assert_array_equal(got["trace_var"][a:b], var, err_msg="trace_var of problem %d" % p)
        np.testing.assert_array_equal(got["trace_con"][a:b], con, err_msg="trace_con of problem %d" % p)
        ident_words += w
    assert (ref["trace_len"][ref["err"] != 0] == 0).all()  # a lowering error: an empty trace
    return ident_words


def assert_results_untraced(got, plain):
    """Everything but the flags' truncation bit is the untraced call's."""
    for k in RESULT_KEYS + ("installed", "core", "core_var", "core_con", "err"):
        if k == "flags":
            np.testing.assert_array_equal(got[k] & ~_lib.F_TRACE_TRUNCATED, plain[k], err_msg=k)
        else:
            np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    assert got["msg"] == plain["msg"] and got["host_lowered"] == plain["host_lowered"]


# ---------------------------------------------------------------------------
# 1. device-lowered problems
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ids16", [True, False], ids=["ids16", "ids32"])
def test_traced_device_lowered(dl, ids16):
    wire = wire_of(2, 1000, 77)
    ref = shared_yardstick("c2-1000-77", lambda: wire, dl.ctx, CAP)
    w32 = _lib.Wire32Arrays(wire, ids16=ids16)
    plain = copied(dl.lower_solve(w32))
    got = dl.lower_solve(w32, CAP)
    assert got["host_lowered"] == 0
    ident_words = assert_traced_equal(got, ref)
    assert_results_untraced(got, plain)
    traced = int((ref["trace_len"] > 0).sum())
    print("traced problems", traced, "identity words", ident_words, "trace words", int(ref["trace_len"].sum()))
    assert traced >= 250 and ident_words >= 2000


def test_traced_register_capped_build(dl):
    wire = wire_of(3, 5000, 77)
    ref = yardstick(wire, dl.ctx, CAP)
    w32 = _lib.Wire32Arrays(wire)
    plain = copied(dl.lower_solve(w32))
    got = dl.lower_solve(w32, CAP)
    assert got["host_lowered"] == 0
    assert_traced_equal(got, ref)
    assert_results_untraced(got, plain)
    assert int((ref["trace_len"] > 0).sum()) >= 1000


# ---------------------------------------------------------------------------
# 2. truncation
# ---------------------------------------------------------------------------
def test_traced_truncation(dl):
    wire = wire_of(2, 1000, 77)
    full = shared_yardstick("c2-1000-77", lambda: wire, dl.ctx, CAP)
    ref = shared_yardstick("c2-1000-77", lambda: wire, dl.ctx, 24)
    got = dl.lower_solve(_lib.Wire32Arrays(wire), 24)
    assert got["host_lowered"] == 0
    assert_traced_equal(got, ref)
    np.testing.assert_array_equal(got["flags"], ref["flags"])
    cut = np.flatnonzero(got["flags"] & _lib.F_TRACE_TRUNCATED)
    print("truncated problems", len(cut))
    assert len(cut) >= 50
    assert np.diff(got["trace_off"]).max() <= 24
    full_res = dict(trace=full["trace"], trace_len=full["trace_len"])
    for p in cut:
        ev = _lib.fused_trace_events(got, p)
        ev_full = _lib.trace_events(full_res, p)
        assert len(ev) < len(ev_full)
        assert [vs for vs, _ in ev] == [vs for vs, _ in ev_full[:len(ev)]]
        a, b = int(got["trace_off"][p]), int(got["trace_off"][p + 1])
        assert sum(2 + len(vs) + len(ids) for vs, ids in ev) == b - a  # whole events only
        np.testing.assert_array_equal(got["trace"][a:b], full["trace"][p][:b - a])


# ---------------------------------------------------------------------------
# 3. host-lowered side
# ---------------------------------------------------------------------------
def test_traced_all_host_lowered(dl):
    wire = wire_of(5, 300, 77)
    ref = yardstick(wire, dl.ctx, CAP)
    got = dl.lower_solve(_lib.Wire32Arrays(wire), CAP)
    assert got["host_lowered"] == 300
    assert_traced_equal(got, ref)
    np.testing.assert_array_equal(got["flags"], ref["flags"])
    assert int((ref["trace_len"] > 0).sum()) >= 90
    assert int(((ref["flags"] & _lib.F_TRACE_TRUNCATED) != 0).sum()) == 2


def test_traced_mixed_with_errors(dl):
    probs = colliding_problems()
    wire = sat.encode_inputs(probs)
    ref = yardstick(wire, dl.ctx, CAP)
    w32 = _lib.Wire32Arrays(wire)
    plain = copied(dl.lower_solve(w32))
    got = dl.lower_solve(w32, CAP)
    assert ref["err"].any()
    assert 0 < got["host_lowered"] < len(probs), got["host_lowered"]
    assert_traced_equal(got, ref)
    assert_results_untraced(got, plain)
    assert (np.diff(got["trace_off"])[got["err"] != 0] == 0).all()


# ---------------------------------------------------------------------------
# 4. windows
# ---------------------------------------------------------------------------
def test_traced_windows(dl, monkeypatch):
    wire = wire_of(2, 700, 21)
    w32 = _lib.Wire32Arrays(wire)
    ref = yardstick(wire, dl.ctx, CAP)
    whole = copied(dl.lower_solve(w32, CAP))
    assert_traced_equal(whole, ref)
    monkeypatch.setenv("DEPPY_FUSED_WINDOW", "128")
    by_window = copied(dl.lower_solve(w32, CAP))
    monkeypatch.delenv("DEPPY_FUSED_WINDOW")
    monkeypatch.setenv("DEPPY_FUSED_TRACE_BYTES", "1048576")  # 64-problem windows: both buffers reused five times
    by_bytes = copied(dl.lower_solve(w32, CAP))
    for got in (by_window, by_bytes):
        assert_traced_equal(got, ref)
        for k in RESULT_KEYS + ("installed", "core", "core_var", "core_con") + TRACE_KEYS:
            np.testing.assert_array_equal(got[k], whole[k], err_msg=k)
        assert got["host_lowered"] == 0


# ---------------------------------------------------------------------------
# 5. reuse of one lowerer
# ---------------------------------------------------------------------------
def test_traced_reuse_of_one_lowerer(dl):
    wire = wire_of(2, 300, 9)
    w32 = _lib.Wire32Arrays(wire)
    ref, ref24 = yardstick(wire, dl.ctx, CAP), yardstick(wire, dl.ctx, 24)
    assert_traced_equal(dl.lower_solve(w32, CAP), ref)
    plain = dl.lower_solve(w32)
    assert not set(TRACE_KEYS) & set(plain)
    assert_equal(plain, ref)
    assert_traced_equal(dl.lower_solve(w32, 24), ref24)
    assert_same(dl.lower(w32, _lib.Lowered.empty(pinned=True)), _lib.Lowered(wire, narrow=True, pinned=True, packed=True))
    catalogs, queries = config2_shared(3, 200, 8)
    k32, q32, qc = sat.encode_shared(catalogs, queries)
    assert_traced_equal(dl.lower_solve_shared(k32, q32, qc, CAP), yardstick(_lib.expand_shared(k32, q32, qc), dl.ctx, CAP))
    none = dl.lower_solve(_lib.Wire32Arrays(sat.encode_inputs([])), CAP)
    assert len(none["status"]) == 0 and list(none["trace_off"]) == [0] and len(none["trace"]) == 0
    assert len(none["trace_var"]) == len(none["trace_con"]) == 0
    bad = _lib.WireArrays(**{k: v.copy() for k, v in wire.a.items() if k != "str_bytes"},
                          str_bytes=wire.a["str_bytes"][:-1].tobytes())
    bad.a["con_arg"][5] = len(bad.a["str_off"]) + 3  # a string index past the table
    with pytest.raises(ValueError, match="malformed wire batch"):
        dl.lower_solve(_lib.Wire32Arrays(bad), CAP)
    assert_traced_equal(dl.lower_solve(w32, CAP), ref)


# ---------------------------------------------------------------------------
# 6. shared
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_catalogs,n_queries,seed", [(16, 800, 5), (3, 700, 21)])
def test_traced_shared(dl, n_catalogs, n_queries, seed):
    catalogs, queries = config2_shared(n_catalogs, n_queries, seed)
    k32, q32, qc = sat.encode_shared(catalogs, queries)
    expanded = _lib.expand_shared(k32, q32, qc)
    plain = copied(dl.lower_solve_shared(k32, q32, qc))
    for cap in (CAP, 24):
        ref = yardstick(expanded, dl.ctx, cap)
        got = dl.lower_solve_shared(k32, q32, qc, cap)
        assert_traced_equal(got, ref)
        np.testing.assert_array_equal(got["flags"], ref["flags"])
        assert_results_untraced(got, plain)
        assert got["host_lowered"] == 0
        if cap == CAP and n_catalogs == 16:
            traced = int((ref["trace_len"] > 0).sum())
            print("traced queries", traced)
            assert traced >= 350
            # owners on both sides of the seam: the catalog's variables and the query's (nv_catalog + i)
            nvk = np.array([len(catalogs[b]) for b, _ in queries])
            prob = np.repeat(np.arange(len(queries)), np.diff(got["trace_off"]))
            own = got["trace_var"]
            assert ((own >= 0) & (own < nvk[prob])).any() and (own >= nvk[prob]).any()


def test_traced_shared_seams(dl):
    """Owners of identities a query's constraint wrote last and of ones the
    catalog's did, both as expanded-problem indices (nv_catalog + i), with
    the seam short of, on and past a 64-lane pass; the UNSAT goldens split
    at the middle."""
    sizes = (63, 64, 65)
    catalogs = [chain_catalog(n) for n in sizes]
    queries = [(b, q) for b, n in enumerate(sizes) for q in seam_queries(n)]
    for vs in unsat_goldens():
        vs = variables_of(vs)
        catalogs.append(vs[:len(vs) // 2])
        queries.append((len(catalogs) - 1, vs[len(vs) // 2:]))
    for ids16 in (True, False):
        k32, q32, qc = sat.encode_shared(catalogs, queries, ids16=ids16)
        ref = yardstick(sat.encode_inputs(concatenated(catalogs, queries)), dl.ctx, CAP)
        got = dl.lower_solve_shared(k32, q32, qc, CAP)
        ident_words = assert_traced_equal(got, ref)
        assert ident_words > 0
        # an owner past the seam: a query's variable, numbered nv_catalog + i
        nvk = np.array([len(catalogs[b]) for b, _ in queries])
        prob = np.repeat(np.arange(len(queries)), np.diff(got["trace_off"]))
        assert (got["trace_var"] >= nvk[prob]).any()


def test_traced_stand_alone_queries(dl):
    wire = wire_of(2, 300, 13)
    q32 = _lib.Wire32Arrays(wire)
    plain = copied(dl.lower_solve(q32, CAP))
    got = dl.lower_solve_shared(empty_catalogs(wire), q32, np.full(300, -1, np.int32), CAP)
    for k in RESULT_KEYS + ("installed", "core", "core_var", "core_con", "err") + TRACE_KEYS:
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    assert int(got["trace_off"][-1]) > 0


# ---------------------------------------------------------------------------
# 7. bytes
# ---------------------------------------------------------------------------
def test_traced_byte_accounting(dl):
    """Only the words that were written cross PCIe (12 bytes each: the word
    and its owner pair) with a length and two offsets' worth per problem, not
    P * trace_cap."""
    n = 1000
    w32 = _lib.Wire32Arrays(wire_of(2, n, 77))
    plain = dl.lower_solve(w32)
    d2h_plain = plain["d2h_bytes"]
    assert plain["host_lowered"] == 0
    got = dl.lower_solve(w32, CAP)
    assert got["host_lowered"] == 0
    words = int(got["trace_off"][-1])
    extra = got["d2h_bytes"] - d2h_plain
    print("trace words", words, "extra d2h", extra, "reservation", 4 * n * CAP)
    assert 12 * words <= extra <= 12 * words + 16 * n + 65536


# ---------------------------------------------------------------------------
# 8. the Python API
# ---------------------------------------------------------------------------
class Rec(sat.Tracer):
    def __init__(self):
        self.events = []

    def Trace(self, pos):
        self.events.append(([str(v.Identifier()) for v in pos.Variables()], [str(a) for a in pos.Conflicts()]))


def outcomes(inputs, results):
    return [outcome(v, r) for v, r in zip(inputs, results)]


def config2_inputs(n, seed):
    w = _lib.generate(2, n, seed)
    return [fixtures.wire_problem_variables(w, p) for p in range(n)]


def test_solve_batch_fused_traced_equals_unfused():
    inputs = config2_inputs(120, 77)
    a, b = Rec(), Rec()
    ra = sat.SolveBatch(inputs, tracer=a)
    rb = sat.SolveBatch(inputs, tracer=b, fused=True)
    assert a.events and a.events == b.events
    assert outcomes(inputs, ra) == outcomes(inputs, rb)


def one_catalog_queries(n_queries=60, seed=5):
    catalogs, queries = config2_shared(1, n_queries, seed)
    return catalogs[0], [q for _, q in queries]


def test_solve_queries_traced_equals_solve_batch():
    catalog, queries = one_catalog_queries()
    inputs = [catalog + q for q in queries]
    a, b = Rec(), Rec()
    ra = sat.SolveBatch(inputs, tracer=a)
    rb = sat.SolveQueries(catalog, queries, tracer=b)
    assert a.events and a.events == b.events
    assert outcomes(inputs, ra) == outcomes(inputs, rb)


def test_truncated_traces_are_escalated(monkeypatch):
    inputs = config2_inputs(120, 77)
    catalog, queries = one_catalog_queries()
    a, c = Rec(), Rec()
    sat.SolveBatch(inputs, tracer=a)
    sat.SolveBatch([catalog + q for q in queries], tracer=c)
    monkeypatch.setattr(sat, "TRACE_CAP", 16)
    b, d = Rec(), Rec()
    sat.SolveBatch(inputs, tracer=b, fused=True)
    sat.SolveQueries(catalog, queries, tracer=d)
    assert a.events == b.events and c.events == d.events
    assert any(2 + len(vs) + len(cs) > 16 for vs, cs in a.events)  # an event that cannot fit 16 words


def test_logging_tracer_text_through_the_fused_path():
    w5 = _lib.generate(5, 20, 61)  # (the goldens fail in the base test; these have search steps to trace)
    cases = [variables_of(vs) for vs in unsat_goldens()] + [fixtures.wire_problem_variables(w5, p) for p in range(20)]
    t0, t1, t2 = io.StringIO(), io.StringIO(), io.StringIO()
    r0 = sat.SolveBatch(cases, tracer=sat.LoggingTracer(t0))
    r1 = sat.SolveBatch(cases, tracer=sat.LoggingTracer(t1), fused=True)
    assert t0.getvalue() and t0.getvalue() == t1.getvalue()
    assert outcomes(cases, r0) == outcomes(cases, r1)
    for vs in cases:  # and split at the middle, through SolveQueries
        sat.SolveQueries(vs[:len(vs) // 2], [vs[len(vs) // 2:]], tracer=sat.LoggingTracer(t2))
    assert t2.getvalue() == t0.getvalue()


def test_tracer_that_calls_solve_queries_inside_trace():
    catalog, queries = one_catalog_queries()
    plain = Rec()
    want = sat.SolveQueries(catalog, queries, tracer=plain)

    class Nested(Rec):
        def Trace(self, pos):
            super().Trace(pos)
            sat.SolveQueries(catalog, queries[:3], tracer=Rec())  # the lowerer's storage, while the outer is mapped

    t = Nested()
    got = sat.SolveQueries(catalog, queries, tracer=t)
    assert plain.events and t.events == plain.events
    inputs = [catalog + q for q in queries]
    assert outcomes(inputs, got) == outcomes(inputs, want)
