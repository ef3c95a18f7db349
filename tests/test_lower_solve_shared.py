"""Shared-catalog queries on the device (dp_lower_solve_shared): problem p is
catalog query_catalog[p]'s variables followed by query p's own, the catalogs
crossing PCIe once per call.  The yardstick is test_lower_solve's, on the
expanded problems: sat.solve_wire on their 64-bit wire; every dp_solved array,
the error codes and texts, and the owner pairs mapped through ident_var /
ident_con are equal."""
import random

import numpy as np
import pytest

from deppy_amd import _lib, sat
from tests import fixtures
from tests.test_device_lowering import assert_same, wire_of
from tests.test_lower_solve import RESULT_KEYS, assert_equal, outcome, unsat_goldens, yardstick
from tests.test_lowering import EDGE, V, _random_problems, all_golden_variable_sets, variables_of

pytestmark = pytest.mark.gpu

P8D, P16 = 6, 3  # DP_FMT_*


@pytest.fixture(scope="module")
def dl():
    ctx = _lib.Context(0, 1)
    d = _lib.DeviceLowerer(ctx)
    yield d
    d.close()
    ctx.close()


def concatenated(catalogs, queries):
    return [(list(catalogs[b]) if b is not None else []) + list(q) for b, q in queries]


def shared_both(dl, catalogs, queries, ids16=True):
    """-> (the shared call's results, the yardstick's on the concatenated problems)"""
    k32, q32, qc = sat.encode_shared(catalogs, queries, ids16=ids16)
    ref = yardstick(sat.encode_inputs(concatenated(catalogs, queries)), dl.ctx)
    return dl.lower_solve_shared(k32, q32, qc), ref


def copied(res):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in res.items()}


def chain_catalog(n):
    """n variables c0..c(n-1): c0 depends on the queries' q0, the rest hold
    Dependencies and Conflicts among themselves."""
    vs = [V("c0", sat.Dependency("q0"))]
    for i in range(1, n):
        if i % 3 == 1:
            vs.append(V("c%d" % i, sat.Dependency("c%d" % ((i + 1) % n), "c%d" % ((i + 2) % n))))
        elif i % 3 == 2:
            vs.append(V("c%d" % i, sat.Conflict("c%d" % ((i + 5) % n))))
        else:
            vs.append(V("c%d" % i))
    return vs


def seam_queries(n):
    q0 = V("q0", sat.Mandatory(), sat.Dependency("c%d" % (n - 1)))
    q1 = V("q1", sat.Conflict("c0"))
    q2 = V("q2", sat.Mandatory(), sat.AtMost(1, "c0", "q0"))
    q1m = V("q1", sat.Mandatory(), sat.Conflict("c%d" % (n // 2)))
    return [[q0], [q0, q1], [q0, q1, q2], [q0, q1m], [V("q0")], [V("q0", sat.Prohibited()), q2]]


def test_segment_boundary_inside_a_pass(dl):
    """Catalogs that end one short of, on and one past a 64-lane pass, and in
    the middle of the third: every scan and table fill crosses the seam."""
    sizes = (1, 63, 64, 65, 130)
    catalogs = [chain_catalog(n) for n in sizes]
    queries = [(b, q) for b, n in enumerate(sizes) for q in seam_queries(n)]
    for ids16 in (True, False):
        got, ref = shared_both(dl, catalogs, queries, ids16)
        assert_equal(got, ref)
        assert got["host_lowered"] == 0
        assert not ref["err"].any() and {1, -1} <= set(ref["status"].tolist())


def test_bit8_plane_across_the_seam(dl):
    """255 catalog variables and 2 of the query: the query's are variables 255
    and 256, so the record carries the high-bit planes (P8D with nv > 256)."""
    catalog = chain_catalog(255)
    queries = []
    for k in range(24):
        q0 = V("q0", sat.Mandatory(), sat.Dependency("q1", "c%d" % (3 + k)))
        cons = [sat.Conflict("c254"), sat.AtMost(1, "q0", "q1", "c%d" % (200 + k))]
        if k % 3 == 0:
            cons.append(sat.Mandatory())
        if k % 4 == 1:
            cons.append(sat.Conflict("q0"))
        queries.append((0, [q0, V("q1", *cons)]))
    got, ref = shared_both(dl, [catalog], queries)
    assert (ref["fmt"] == P8D).all(), np.unique(ref["fmt"])
    assert_equal(got, ref)
    assert got["host_lowered"] == 0
    assert (np.diff(ref["inst_off"]) == 9).all()  # 257 variables: 9 words of installed bits


def test_sums_past_the_kernel_sizes(dl):
    """The kernel's sizes bound the two segments' sums: 511 + 2 variables and
    510 + 3 constraints go to the host, and nothing else of the batch does."""
    wide = [V("w%d" % i) for i in range(511)]
    dense = [V("d%d" % i, sat.Dependency(), sat.Prohibited()) for i in range(255)]  # 510 constraints, no argument
    small = chain_catalog(65)
    two = [V("q0", sat.Mandatory(), sat.Dependency("w7")), V("q1", sat.Conflict("w8"))]
    three = [V("q0", sat.Mandatory(), sat.Conflict("d0"), sat.Conflict("d1"))]
    rest = [(2, q) for q in seam_queries(65)] * 8
    queries = rest[:30] + [(0, two), (1, three)] + rest[30:]
    catalogs = [wide, dense, small]
    got, ref = shared_both(dl, catalogs, queries)
    assert_equal(got, ref)
    assert got["host_lowered"] == 2
    # (whether the kernel takes a problem depends on that problem alone: without the two, none)
    got, ref = shared_both(dl, catalogs, rest)
    assert_equal(got, ref)
    assert got["host_lowered"] == 0
    # exactly at the sizes (512 variables; 512 constraints): what the kernel
    # does with the expanded problems, it does with the shared ones
    edge = [(0, [V("q0", sat.Mandatory(), sat.Dependency("w7"))]), (1, [V("q0", sat.Mandatory(), sat.Conflict("d0"))])]
    edge += rest
    k32, q32, qc = sat.encode_shared(catalogs, edge)
    wire = sat.encode_inputs(concatenated(catalogs, edge))
    ref = yardstick(wire, dl.ctx)
    plain = dl.lower_solve(_lib.Wire32Arrays(wire))["host_lowered"]
    got = dl.lower_solve_shared(k32, q32, qc)
    assert_equal(got, ref)
    assert got["host_lowered"] == plain


def sharing_batch():
    """A catalog's Conflict(a, b) and a query's AtMost(1; a, b) are one
    identity, the query's the last writer.  Half of the queries force a and b
    (NotSatisfiable, the shared identity in the core), half only a."""
    catalogs = []
    for pad in (0, 61, 62, 126):
        catalogs.append([V("a", sat.Conflict("b")), V("b")] + [V("z%d" % i) for i in range(pad)] + [V("x")])
    queries = []
    for k in range(120):
        q = V("q", sat.Mandatory(), sat.Dependency("a"), sat.AtMost(1, "a", "b"))
        extra = [V("e%d" % k, sat.Dependency("x"))] if k % 5 == 0 else []
        if k % 2:
            queries.append((k % 4, [q, V("r", sat.Mandatory(), sat.Dependency("b"))] + extra))
        else:
            queries.append((k % 4, [q] + extra))
    return catalogs, queries


def test_identity_sharing_and_last_writer_across_segments(dl):
    catalogs, queries = sharing_batch()
    got, ref = shared_both(dl, catalogs, queries)
    assert_equal(got, ref)
    assert got["host_lowered"] == 0
    unsat = np.flatnonzero((ref["status"] == sat.UNSAT) & (ref["core_len"] >= 2))
    assert len(unsat) >= 50 and int((ref["status"] == sat.SAT).sum()) >= 50
    for p in unsat:
        nvk = len(catalogs[queries[p][0]])
        c0, n = int(got["core_off"][p]), int(got["core_len"][p])
        owners = set(zip(got["core_var"][c0:c0 + n].tolist(), got["core_con"][c0:c0 + n].tolist()))
        assert (nvk, 2) in owners, (p, owners)  # the query's AtMost, not the catalog's Conflict (0, 0)
        assert (0, 0) not in owners


def test_errors_across_segments(dl):
    catalogs = [[V("a", sat.Dependency("late")), V("b")], chain_catalog(64)]
    queries = [
        (0, [V("late")]),  # the catalog's argument resolves
        (0, [V("q")]),  # ... and does not: the catalog's lookup error
        (0, [V("late"), V("a")]),  # a duplicate across the segments
        (0, [V("late"), V("q", sat.Conflict("nope"), sat.AtMost(1, "b", 'x"\\y'))]),  # the query's lookup errors
        (1, [V("q0"), V("c63")]),
        (1, [V("q1", sat.Dependency("c0", "gone"))]),  # both segments' lookups, in Apply order
        (None, [V("a", sat.Conflict("b"))]),  # alone, the catalog's b is unknown
        (1, [V("q0", sat.Mandatory())]),
    ] * 3
    got, ref = shared_both(dl, catalogs, queries)
    assert_equal(got, ref)
    assert ref["err"][:8].tolist() == [0, 2, 1, 2, 1, 2, 2, 0]
    assert got["host_lowered"] == int((ref["err"] != 0).sum())


def test_colliding_problems_split_at_a_random_seam(dl):
    probs = []
    for seed in (1, 2, 3):
        probs += _random_problems(seed, 400)
    probs += EDGE + [variables_of(vs) for vs in all_golden_variable_sets()]
    rng = random.Random(5)
    catalogs, queries = [], []
    for vs in probs:
        s = rng.randint(0, len(vs))
        catalogs.append(vs[:s])
        queries.append((len(catalogs) - 1, vs[s:]))
    got, ref = shared_both(dl, catalogs, queries)
    assert_equal(got, ref)
    assert ref["err"].any()
    assert 0 < got["host_lowered"] < len(probs), got["host_lowered"]
    # the kernel takes a problem whatever its seam
    plain = dl.lower_solve(_lib.Wire32Arrays(sat.encode_inputs(probs)))["host_lowered"]
    assert dl.lower_solve_shared(*sat.encode_shared(catalogs, queries))["host_lowered"] == plain


def test_p16_records_from_a_query(dl):
    """A query's Dependency whose first candidate is its subject: a choice
    list no row implies, so the record is DP_FMT_P16."""
    catalogs = [chain_catalog(n) for n in (5, 64, 130)]
    queries = []
    for k in range(30):
        cons = [sat.Dependency("q0", "c%d" % (k % 5))]
        if k % 2:
            cons.append(sat.Mandatory())
        queries.append((k % 3, [V("q0", *cons), V("q1", sat.Dependency("q0"))]))
    got, ref = shared_both(dl, catalogs, queries)
    assert (ref["fmt"] == P16).all(), np.unique(ref["fmt"])
    assert_equal(got, ref)
    assert got["host_lowered"] == 0


def empty_catalogs(wire, ids16=True):
    """No catalog at all, over the wire's string table."""
    a = wire.a
    none = _lib.WireArrays([0], [], [0], [], [], [0], [], a["str_off"], a["str_bytes"][:-1].tobytes())
    return _lib.Wire32Arrays(none, ids16=ids16)


def test_stand_alone_queries_equal_lower_solve(dl):
    for config, n, ids16 in ((2, 300, True), (3, 900, False)):
        wire = wire_of(config, n, 13)
        q32 = _lib.Wire32Arrays(wire, ids16=ids16)
        plain = copied(dl.lower_solve(q32))
        got = dl.lower_solve_shared(empty_catalogs(wire, ids16), q32, np.full(n, -1, np.int32))
        for k in RESULT_KEYS + ("installed", "core", "core_var", "core_con", "err"):
            np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
        assert got["msg"] == plain["msg"] and got["host_lowered"] == plain["host_lowered"] == 0
        assert_equal(got, yardstick(wire, dl.ctx))


def config2_shared(n_catalogs, n_queries, seed):
    """Config-2 catalogs under interleaved two-variable queries that name
    their catalog's identifiers."""
    w = _lib.generate(2, n_catalogs, seed)
    catalogs = [fixtures.wire_problem_variables(w, b) for b in range(n_catalogs)]
    ids = [[str(v.Identifier()) for v in c] for c in catalogs]
    rng = random.Random(seed)
    queries = []
    for p in range(n_queries):
        b = p % n_catalogs
        x, y, z = rng.sample(ids[b], 3)
        qa = V("q%da" % p, sat.Mandatory(), sat.Dependency(x, y))
        qb = V("q%db" % p, *([sat.Mandatory()] if p % 3 == 0 else []), sat.Conflict(z))
        queries.append((b, [qa, qb]))
    return catalogs, queries


def test_shared_windows(dl, monkeypatch):
    catalogs, queries = config2_shared(3, 700, 21)
    k32, q32, qc = sat.encode_shared(catalogs, queries)
    ref = yardstick(_lib.expand_shared(k32, q32, qc), dl.ctx)
    whole = copied(dl.lower_solve_shared(k32, q32, qc))
    assert_equal(whole, ref)
    monkeypatch.setenv("DEPPY_FUSED_WINDOW", "128")
    got = dl.lower_solve_shared(k32, q32, qc)
    assert_equal(got, ref)
    for k in RESULT_KEYS + ("installed", "core", "core_var", "core_con"):
        np.testing.assert_array_equal(got[k], whole[k], err_msg=k)
    assert got["host_lowered"] == whole["host_lowered"] == 0
    none = dl.lower_solve_shared(*sat.encode_shared(catalogs, []))
    assert len(none["status"]) == 0 and list(none["inst_off"]) == [0] and none["host_lowered"] == 0


def test_one_lowerer_alternates_the_calls(dl, monkeypatch):
    monkeypatch.setenv("DEPPY_FUSED_WINDOW", "256")
    catalogs, queries = config2_shared(3, 400, 8)
    sizes = (1, 63, 64, 65, 130)
    small = [chain_catalog(n) for n in sizes], [(b, q) for b, n in enumerate(sizes) for q in seam_queries(n)]
    for rnd, (config, n) in enumerate(((2, 600), (6, 200))):
        k32, q32, qc = sat.encode_shared(catalogs, queries, ids16=rnd == 0)
        assert_equal(dl.lower_solve_shared(k32, q32, qc), yardstick(_lib.expand_shared(k32, q32, qc), dl.ctx))
        wire = wire_of(config, n, 31 + rnd)
        w32 = _lib.Wire32Arrays(wire, ids16=rnd == 1)
        assert_equal(dl.lower_solve(w32), yardstick(wire, dl.ctx))
        assert_same(dl.lower(w32, _lib.Lowered.empty(pinned=True)),
                    _lib.Lowered(wire, narrow=True, pinned=True, packed=True))
        k32, q32, qc = sat.encode_shared(catalogs, queries, ids16=rnd == 1)
        assert_equal(dl.lower_solve_shared(k32, q32, qc), yardstick(_lib.expand_shared(k32, q32, qc), dl.ctx))
        got, ref = shared_both(dl, *small, ids16=rnd == 0)
        assert_equal(got, ref)


def test_shared_byte_accounting(dl):
    """The catalogs go to the device once: a call's bytes in are the two
    wires, a catalog number per query and the solve's launch tables, a small
    part of what the expanded compact wire would be."""
    n = 2000
    catalogs, queries = config2_shared(4, n, 77)
    k32, q32, qc = sat.encode_shared(catalogs, queries)
    got = dl.lower_solve_shared(k32, q32, qc)
    expanded = _lib.Wire32Arrays(_lib.expand_shared(k32, q32, qc)).nbytes()
    wires = k32.nbytes() + q32.nbytes()
    print("per query: h2d", got["h2d_bytes"] / n, "wires", wires / n, "expanded wire", expanded / n)
    assert got["host_lowered"] == 0
    assert wires <= got["h2d_bytes"] <= wires + 68 * n + 65536
    assert got["h2d_bytes"] < expanded / 4


def test_solve_queries_equals_solve_batch_fused():
    readme = [variables_of(c["variables"]) for c in fixtures.load("readme")["cases"]]
    unsat = [variables_of(vs) for vs in unsat_goldens()]
    kinds = set()
    for vs in readme + unsat:
        for s in sorted({0, len(vs) // 2, max(0, len(vs) - 1), len(vs)}):
            catalog = vs[:s]
            qs = [vs[s:], vs[s:] + [V("extra-q", sat.Mandatory())], vs[s:][::-1], []]
            want = sat.SolveBatch([list(catalog) + list(q) for q in qs], fused=True)
            got = sat.SolveQueries(catalog, qs)
            assert len(got) == len(want) == len(qs)
            for q, a, b in zip(qs, got, want):
                variables = list(catalog) + list(q)
                assert outcome(variables, a) == outcome(variables, b)
                kinds.add(outcome(variables, a)[1])
    assert {"NotSatisfiable", "NoneType"} <= kinds
    assert sat.SolveQueries(readme[0], []) == []
