"""The Or constraint on the device: dp_lower_device byte for byte against the
host lowering, the fused, shared-catalog and prepared calls (plain and traced)
against sat.solve_wire on the 64-bit wire with Ors on both sides of the seam,
the row of two positive literals (DP_H_NVU, the solve kernels' full scan)
against the oracle on every placement, and the Python API end to end."""
import numpy as np
import pytest

from deppy_amd import _lib, sat
from oracle import oracle
from tests import lower_or_ref
from tests.gpu_common import compare_results
from tests.lower_or_ref import problem_of
from tests.test_device_lowering import assert_same
from tests.test_lower_solve import assert_equal, yardstick
from tests.test_lower_solve_shared import concatenated, copied
from tests.test_lower_solve_traced import CAP, assert_results_untraced, assert_traced_equal
from tests.test_lower_solve_traced import yardstick as traced_yardstick
from tests.test_lowering import V
from tests.test_or_lowering import (FMT_P16, FMT_P8D, H_FMT, H_NVU, NN, ON, SHARING, SN, TABLE, AtMost, Conf, Dep, Mand,
                                    Or, Proh, random_or_problems)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dl():
    ctx = _lib.Context(0, 1)
    d = _lib.DeviceLowerer(ctx)
    yield d
    d.close()
    ctx.close()


_memo = {}


def or_problems():
    """The CPU tests' table and sharing problems and the 2,000 random ones,
    with what the restatement says of each (made once)."""
    if "probs" not in _memo:
        probs = list(TABLE.values()) + [vs for vs, _ in SHARING.values()] + random_or_problems()
        _memo["probs"] = probs, [lower_or_ref.lower_problem(problem_of(vs)) for vs in probs]
    return _memo["probs"]


def host_for_todays_reasons(vs, ref):
    """The problems the kernel leaves to the host for reasons that hold
    without any Or: an error to report, an AtMost naming an identifier twice
    or two AtMosts over one set and bound in different orders (the exact
    path), a Dependency whose later candidate is its subject (the identity
    stays while its row folds away)."""
    if ref.error:
        return True
    orders = {}  # AtMosts over three or more variables: one set and bound in two orders
    for v in vs:
        for c in v.Constraints():
            if c.kind == 5 and 0 <= c.n < len(c.ids) and len(c.ids) >= 3:
                orders.setdefault((c.n, frozenset(c.ids)), set()).add(c.ids)
    if any(len(o) > 1 for o in orders.values()):
        return True
    for v in vs:
        for c in v.Constraints():
            if c.kind == 5 and 0 <= c.n < len(c.ids) and len(set(c.ids)) < len(c.ids):
                return True
            if c.kind == 3 and c.ids and c.ids[0] != v.Identifier() and v.Identifier() in c.ids:
                return True
    return False


# ---------------------------------------------------------------------------
# dp_lower_device
# ---------------------------------------------------------------------------
def test_device_records_equal_host(dl):
    probs, refs = or_problems()
    wire = sat.encode_inputs(probs)
    host = _lib.Lowered(wire, narrow=True, pinned=True, packed=True)
    dev = dl.lower(_lib.Wire32Arrays(wire), _lib.Lowered.empty(pinned=True))
    assert_same(dev, host)
    today = sum(host_for_todays_reasons(vs, ref) for vs, ref in zip(probs, refs))
    print("host-lowered", dl.host_count, "of", len(probs), "for today's reasons", today)
    assert dl.host_count <= today < len(probs) // 2
    fmts = dev.rec[dev.rec_off[:-1] + H_FMT]
    assert (fmts == FMT_P8D).sum() > 100 and (fmts == FMT_P16).sum() > 100
    # problem by problem: one whose only reason would be an Or is the kernel's
    only_or = [p for p, (vs, ref) in enumerate(zip(probs, refs)) if not host_for_todays_reasons(vs, ref)][:300]
    one = [probs[p] for p in only_or]
    w1 = sat.encode_inputs(one)
    dev1 = dl.lower(_lib.Wire32Arrays(w1), _lib.Lowered.empty(pinned=True))
    assert dl.host_count == 0
    assert_same(dev1, _lib.Lowered(w1, narrow=True, pinned=True, packed=True))
    nvu = dev1.rec[dev1.rec_off[:-1] + H_NVU]
    pos = np.array([refs[p].pos_row for p in only_or])
    np.testing.assert_array_equal(nvu > 0, pos)
    assert pos.any() and not pos.all()


# ---------------------------------------------------------------------------
# the fused, shared and prepared calls
# ---------------------------------------------------------------------------
def backtracking_problems():
    """Two anchors a and e each need a candidate, and their first candidates b
    and f exclude each other through Ors -- (~b ~f), or (~b h) with (~f ~h) --
    so the search guesses b, then f, fails and moves on to g: the tracer sees
    a step whose conflict is an Or."""
    out = []
    for k in range(40):
        if k % 2:
            vs = [V("a", Mand(), Dep("b", "c")), V("b", Or("h", **SN)), V("c"), V("e", Mand(), Dep("f", "g")),
                  V("f", Or("h", **NN)), V("g"), V("h")]
        else:
            vs = [V("a", Mand(), Dep("b", "c")), V("b", Or("f", **NN)), V("c"), V("e", Mand(), Dep("f", "g")), V("f"),
                  V("g")]
        out.append(vs + [V("x%d" % i, Or("a")) for i in range(k % 4)])
    return out


def test_fused_equals_host_lowered(dl):
    probs = or_problems()[0] + backtracking_problems()
    wire = sat.encode_inputs(probs)
    ref = traced_yardstick(wire, dl.ctx, CAP)
    w32 = _lib.Wire32Arrays(wire)
    plain = copied(dl.lower_solve(w32))
    assert_equal(plain, ref)
    got = dl.lower_solve(w32, CAP)
    assert_traced_equal(got, ref)
    assert_results_untraced(got, plain)
    # every backtracking problem is traced (its first candidate fails)
    assert {1, -1} <= set(ref["status"].tolist()) and (ref["trace_len"][-40:] > 0).all()


def seam_batch():
    """A closed catalog holding Ors of every polarity, the same catalog
    without them, and queries whose Ors name the catalog's identifiers."""
    cat = [V("a", Dep("b"), Or("c", **SN)),          # (~a c): a first-writer Or of mixed signs
           V("b", Conf("c"), Or("d")),               # (b d): all positive
           V("c", Or("d", **ON)),                    # (~d c)
           V("d", Or("d", **NN), Or("a", **NN)),     # the unit (~d); (~d ~a)
           V("e", Mand(), Dep("a", "b"))]
    plain = [V("a", Dep("b")), V("b", Conf("c")), V("c"), V("d"), V("e", Mand(), Dep("a", "b"))]
    queries = [
        [V("q", Mand(), Or("a", **ON))],                        # (~a q)
        [V("q", Mand(), Or("b", **ON), Dep("a"))],
        [V("q", Mand(), Dep("a")), V("r", Or("q", **SN))],
        [V("q", Or("a", **SN), Mand())],                        # (~q a)
        [V("q", Mand(), Conf("e")), V("r", Or("q"))],
        [V("q", Mand()), V("r", Or("r", **NN), Or("q", **NN), Mand())],
        [V("q", Proh(), Or("e", **NN))],
        [V("q", Mand(), AtMost(1, "a", "d"))],                  # K_CONF{a, d}: catalog 0's Or(~d ~a) wrote it first
        [V("q", Mand(), Dep("d")), V("r", Mand(), Conf("a"), Or("e", **SN), Or("d"))],
        [],
    ]
    return cat, plain, queries


def test_shared_and_prepared_equal_host_lowered(dl):
    cat, plain, queries = seam_batch()
    # catalog 2: its Or of mixed signs is a first writer, so every query's
    # record has explicit lists (the rule crosses the seam)
    c2 = [V("x", Or("y", **SN)), V("y"), V("z", Mand())]
    q2 = [[V("q", Mand(), Dep("x"))], [V("q", Mand(), Dep("x")), V("r", Or("q"))], [V("q", Or("z", **NN))]]
    # catalog 3 names the query's q: the query's Ors are the last writers of
    # its Dependency(a; q) and Conflict(b, q)
    c3 = [V("a", Mand(), Dep("q")), V("b", Mand(), Conf("q"))]
    q3 = [[V("q", Or("a", **ON), Proh())], [V("q", Or("b", **NN), Mand())], [V("q", Or("a", **ON), Or("b", **NN))]]
    # catalog 4: its Or (x ~q) is the first writer of Dependency(q; x)'s
    # identity, which the query joins: a list without a row of its own
    c4 = [V("x", Or("q", **ON), Proh()), V("y", Or("q"))]
    q4 = [[V("q", Mand(), Dep("x"))], [V("q", Dep("x"), Or("y"))]]
    # catalogs 5 and 6: the search backtracks over an Or, so the traces name it
    c5, c6 = backtracking_problems()[:2]
    q5 = [[V("q", Or("a"))], [V("q", Mand(), Or("g", **NN))], []]
    catalogs = [cat, plain, c2, c3, c4, c5, c6]
    qs = [(0, q) for q in queries] + [(1, q) for q in queries] + [(2, q) for q in q2] * 3 + \
        [(None, c2 + q) for q in q2] + [(3, q) for q in q3] * 2 + [(4, q) for q in q4] * 2 + \
        [(b, q) for b in (5, 6) for q in q5]
    k32, q32, qc = sat.encode_shared(catalogs, qs)
    wire = sat.encode_inputs(concatenated(catalogs, qs))
    ref = traced_yardstick(wire, dl.ctx, CAP)
    assert not ref["err"].any() and {1, -1} <= set(ref["status"].tolist())
    of = lambda b: [p for p, (x, _) in enumerate(qs) if x == b]
    fmt = ref["fmt"]
    assert (fmt[of(0)] == FMT_P16).all() and (fmt[of(2)] == FMT_P16).all() and (fmt[of(4)] == FMT_P16).all()
    assert (fmt[of(1)] == FMT_P8D).any() and (fmt[of(3)] == FMT_P8D).all()
    assert (ref["trace_len"][of(5)] > 0).sum() >= 2 and (ref["trace_len"][of(6)] > 0).sum() >= 2

    def core_owners(r, p):
        c0, n = int(r["core_off"][p]), int(r["core_len"][p])
        return set(zip(r["core_var"][c0:c0 + n].tolist(), r["core_con"][c0:c0 + n].tolist()))

    def check(got):
        assert_equal(got, ref)
        assert got["host_lowered"] == 0
        # the shared identities' reported owners are the query's constraints
        p3, p4 = of(3), of(4)
        assert core_owners(got, p3[0]) == {(0, 0), (2, 0), (2, 1)}  # a mandatory, the query's Or, q prohibited
        assert core_owners(got, p3[1]) == {(1, 0), (2, 0), (2, 1)}
        assert core_owners(got, p4[0]) == {(0, 1), (2, 0), (2, 1)}  # x prohibited, q mandatory, the query's Dependency

    shared = copied(dl.lower_solve_shared(k32, q32, qc))
    check(shared)
    traced = dl.lower_solve_shared(k32, q32, qc, CAP)
    assert_traced_equal(traced, ref)
    assert_results_untraced(traced, shared)
    h = dl.prepare(k32)
    try:
        # the closed catalogs, Ors or not, are prepared; the two that name the query's q are not
        assert [h.prepared(b) for b in range(h.count)] == [1, 1, 1, 0, 0, 1, 1]
        got = copied(h.lower_solve(q32, qc))
        check(got)
        traced = h.lower_solve(q32, qc, CAP)
        assert_traced_equal(traced, ref)
        assert_results_untraced(traced, got)
    finally:
        h.close()


# ---------------------------------------------------------------------------
# the row of two positive literals
# ---------------------------------------------------------------------------
def filler_problem(F, b_prohibited=False, a_prohibited=False):
    vs = [V("f%d" % i, Proh()) for i in range(F)]
    vs.append(V("a", Or("b"), *([Proh()] if a_prohibited else [])))
    vs.append(V("b", *([Proh()] if b_prohibited else [])))
    return vs


def filler_records(F, **fl):
    probs = [filler_problem(F), filler_problem(F, b_prohibited=True), filler_problem(F, True, True)]
    lw = _lib.Lowered(sat.encode_inputs(probs), **fl)
    assert all(int(lw.record(p)[H_NVU]) == F + 2 for p in range(3))
    key = (F, tuple(sorted(fl.items())))
    if key not in _memo:
        _memo[key] = oracle.solve_batch(lw.rec_off, lw.rec, 0, 1)
    o = _memo[key]
    a = F
    assert o["status"].tolist() == [1, 1, -1]
    for p in (0, 1):
        assert _lib.installed_list(o, p, F + 2) == [a], p
    i0 = int(lw.ident_off[2])
    owners = sorted((int(lw.ident_var[i0 + i]), int(lw.ident_con[i0 + i])) for i in _lib.core_list(o, 2))
    assert owners == [(F, 0), (F, 1), (F + 1, 0)]  # the Or and the two Prohibiteds
    return probs, lw, o


def test_all_positive_row_one_wavefront(dl):
    """260 Prohibited fillers (more than 256 clause rows, so first_violated
    scans watch lists only), then a: Or(b), then b.  On a build whose
    lowering left DP_H_NVU at 0 the first problem came back with nothing
    installed (flags 0, steps 0) where the oracle installs a (flags 8, 1 step):
    profiles/or_guard.txt."""
    probs, lw, o = filler_records(260, narrow=True, packed=True, pinned=True)
    ctx = dl.ctx
    assert compare_results(ctx.solve(lw.rec_off, lw.rec), o, 3) == []  # the latency path
    many = _lib.Lowered(sat.encode_inputs(probs * 20), narrow=True, packed=True, pinned=True)
    g = ctx.solve(many.rec_off, many.rec)  # the pipeline
    for p in range(60):
        q = p % 3
        assert (g["status"][p], g["flags"][p], g["steps"][p]) == (o["status"][q], o["flags"][q], o["steps"][q]), p
        assert _lib.installed_list(g, p, 262) == _lib.installed_list(o, q, 262), p
        assert _lib.core_list(g, p) == _lib.core_list(o, q), p
    r = ctx.upload(lw.rec_off, lw.rec)  # the resident path
    try:
        r.run()
        assert compare_results(r.download(), o, 3) == []
    finally:
        r.free()
    wire = sat.encode_inputs(probs)
    fused = dl.lower_solve(_lib.Wire32Arrays(wire))  # the fused path
    assert fused["host_lowered"] == 0
    assert_equal(fused, yardstick(wire, ctx))
    for k in ("status", "flags", "steps", "core_len"):
        np.testing.assert_array_equal(fused[k], o[k], err_msg=k)
    np.testing.assert_array_equal(fused["installed"], o["installed"][:len(fused["installed"])])


@pytest.mark.parametrize("F,flags", [(1100, _lib.OPT_FORCE_LDSG), (1100, _lib.OPT_FORCE_MID),
                                     (2100, _lib.OPT_FORCE_GROUP), (2100, _lib.OPT_FORCE_HBM)],
                         ids=["ldsg", "split4", "split", "hbm"])
def test_all_positive_row_multiwave(F, flags):
    _, lw, o = filler_records(F)
    c = _lib.Context(0, 1, flags=flags)
    try:
        g = c.solve(lw.rec_off, lw.rec)
    finally:
        c.close()
    assert compare_results(g, o, 3) == []


# ---------------------------------------------------------------------------
# the Python API
# ---------------------------------------------------------------------------
def eight(unsat):
    """Eight variables, every polarity of Or; SAT, or NotSatisfiable with an Or among the applied constraints."""
    return [V("a", Mand(), Or("b", **SN)),            # a -> b
            V("b", Or("c", **NN)),                    # not both b and c
            V("c", Or("d")),                          # c or d
            V("d", Or("c", **ON), *([Proh()] if unsat else [])),
            V("e", Mand(), Dep("f", "g")),
            V("f", Or("a", **NN)),                    # not both f and a
            V("g", Or("h", **ON)),                    # g or not h
            V("h", *([Mand(), Or("b", **SN, **ON)] if unsat else []))]


def outcome_of(res):
    installed, err = res
    if err is not None:
        return type(err).__name__, sorted(a.String() for a in err)
    return "ok", [str(v.Identifier()) for v in installed]


def test_python_api_end_to_end():
    sat_in, unsat_in = eight(False), eight(True)
    want = []
    for vs in (sat_in, unsat_in):
        s, err = sat.NewSolver(sat.WithInput(vs))
        assert err is None
        want.append(outcome_of(s.Solve(None)))
    assert want[0] == ("ok", ["a", "b", "d", "e", "g"]), want[0]
    assert want[1][0] == "NotSatisfiable" and any(" or " in t for t in want[1][1]), want[1]
    # the model and the core against the definitions
    assert want[1][1] == sorted(["a is mandatory", "not a or b", "h is mandatory", "not h or not b"]), want[1]
    for fused in (False, True):
        assert [outcome_of(r) for r in sat.SolveBatch([sat_in, unsat_in], fused=fused)] == want
    for k, vs in enumerate((sat_in, unsat_in)):
        # (a to d name only each other: a closed catalog, which is prepared)
        assert [outcome_of(r) for r in sat.SolveQueries(vs[:4], [vs[4:], vs[4:]])] == [want[k]] * 2
        cat = sat.Catalog(vs[:4])
        try:
            assert cat.prepared
            assert [outcome_of(r) for r in cat.Solve([vs[4:], vs[4:]])] == [want[k]] * 2
        finally:
            cat.close()
