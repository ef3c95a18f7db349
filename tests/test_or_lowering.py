"""The Or constraint on the host: API, wire checks, the exact and the fast
lowering against the restatement with Or (tests/lower_or_ref.py), the rule
that chooses a record form (explicit choice lists next to a first-writer Or of
mixed signs), DP_H_NVU on records with a row of two positive literals, and
the oracle on Or problems against brute force."""
import itertools

import numpy as np
import pytest

from deppy_amd import _lib, sat
from oracle import lower_ref, oracle
from tests import lower_or_ref
from tests.lower_or_ref import problem_of
from tests.test_lowering import EDGE, V, all_golden_variable_sets, variables_of

Or, Dep, Conf, AtMost, Mand, Proh = sat.Or, sat.Dependency, sat.Conflict, sat.AtMost, sat.Mandatory, sat.Prohibited
NN = dict(isSubjectNegated=True, isOperandNegated=True)
SN = dict(isSubjectNegated=True)
ON = dict(isOperandNegated=True)
H_NV, H_NC, H_NID, H_NVU, H_FMT = 1, 2, 6, 11, 13
FMT_I32, FMT_U16, FMT_P16, FMT_P16D, FMT_P8D = 0, 1, 3, 5, 6
# the flag combinations of the existing lowering tests
FLAGSETS = {"int32": {}, "narrow": dict(narrow=True), "packed": dict(narrow=True, packed=True),
            "no_p8": dict(narrow=True, packed=True, p8=False)}

# every row of the issue's table of cases, two to four variables
TABLE = {
    "same-pos": [V("a", Or("a")), V("b")],
    "same-neg": [V("a", Or("a", **NN)), V("b")],
    "same-differ": [V("a", Or("a", **SN)), V("b", Or("b", **ON))],
    "both-neg": [V("a", Or("b", **NN)), V("b")],
    "both-pos": [V("a", Or("b")), V("b")],
    "mixed-subject": [V("a", Or("b", **SN)), V("b")],
    "mixed-operand": [V("a", Or("b", **ON)), V("b")],
    "all-three": [V("a", Mand(), Or("c"), Or("b", **SN)), V("b", Or("d", **NN)), V("c", Or("a", **ON)), V("d")],
    "with-lists": [V("a", Dep("b", "c"), Or("c", **SN)), V("b", Or("c")), V("c", Dep("a"))],
}

# identity sharing: (problem, the one shared identity's last writer (variable, constraint))
SHARING = {
    "nn-conflict": ([V("a", Or("b", **NN), Conf("b")), V("b")], (0, 1)),
    "conflict-nn": ([V("a", Conf("b")), V("b", Or("a", **NN))], (1, 0)),
    "nn-atmost": ([V("a", Or("b", **NN)), V("b", AtMost(1, "b", "a"))], (1, 0)),
    "atmost-nn": ([V("a", AtMost(1, "a", "b"), Or("b", **NN)), V("b")], (0, 1)),
    "mixed-dep-same-subject": ([V("a", Or("b", **SN), Dep("b")), V("b")], (0, 1)),
    "dep-mixed-same-subject": ([V("a", Dep("b"), Or("b", **SN)), V("b")], (0, 1)),
    "mixed-dep-other-subject": ([V("b", Or("a", **ON)), V("a", Dep("b"))], (1, 0)),
    "dep-mixed-other-subject": ([V("a", Dep("b")), V("b", Or("a", **ON))], (1, 0)),
    "pos-pos": ([V("a", Or("b")), V("b", Or("a"))], (1, 0)),
    "pos-pos-same-subject": ([V("a", Or("b"), Or("b")), V("b")], (0, 1)),
    "same-mandatory": ([V("a", Or("a"), Mand())], (0, 1)),
    "mandatory-same": ([V("a", Mand(), Or("a"))], (0, 1)),
    "same-prohibited": ([V("a", Or("a", **NN), Proh())], (0, 1)),
    "prohibited-same": ([V("a", Proh(), Or("a", **NN))], (0, 1)),
}


def widen(r):
    r = np.ascontiguousarray(r)
    out = np.zeros(int(r[10]), np.int32)
    assert _lib.lib().dp_rec_widen(r.ctypes.data_as(_lib.c_i32p), len(r), out.ctypes.data_as(_lib.c_i32p)) == 0
    return out


def has_pos_row(rec):
    """rec (int32 form) holds a clause row of two or more literals, none negative."""
    nc = int(rec[H_NC])
    off = rec[16:16 + nc + 1]
    lits = rec[16 + nc + 1:]
    return any(off[i + 1] - off[i] >= 2 and not (lits[off[i]:off[i + 1]] & 1).any() for i in range(nc))


def lowered_all(probs, monkeypatch):
    """{(flagset, path): Lowered} for both host paths."""
    wire = sat.encode_inputs(probs)
    out = {}
    for name, fl in FLAGSETS.items():
        monkeypatch.delenv("DEPPY_LOWER_EXACT", raising=False)
        out[name, "fast"] = _lib.Lowered(wire, **fl)
        monkeypatch.setenv("DEPPY_LOWER_EXACT", "1")
        out[name, "exact"] = _lib.Lowered(wire, **fl)
        assert out[name, "exact"].n_exact == len(probs)
    monkeypatch.delenv("DEPPY_LOWER_EXACT", raising=False)
    return out


def check_against_restatement(probs, monkeypatch, refs=None):
    """Both host paths in every flag combination: the int32 record, the
    identities and the owners are the restatement's, a packed record widens
    to it, the two paths give the same bytes, a record next to a first-writer
    Or of mixed signs has explicit lists, and DP_H_NVU is set exactly on the
    records with a row of two positive literals."""
    refs = refs or [lower_or_ref.lower_problem(problem_of(vs)) for vs in probs]
    lws = lowered_all(probs, monkeypatch)
    for name in FLAGSETS:
        fast, exact = lws[name, "fast"], lws[name, "exact"]
        np.testing.assert_array_equal(fast.rec_off, exact.rec_off)
        np.testing.assert_array_equal(fast.rec, exact.rec)
        np.testing.assert_array_equal(fast.ident_var, exact.ident_var)
        np.testing.assert_array_equal(fast.ident_con, exact.ident_con)
        assert fast.msg == exact.msg
        for p, ref in enumerate(refs):
            assert fast.err[p] == ref.error and fast.msg[p] == ref.msg, (p, fast.msg[p], ref.msg)
            if ref.error:
                continue
            r = fast.record(p)
            np.testing.assert_array_equal(widen(r), ref.rec, err_msg="%s problem %d" % (name, p))
            i0, i1 = fast.ident_off[p], fast.ident_off[p + 1]
            assert list(fast.ident_var[i0:i1]) == list(ref.ident_var)
            assert list(fast.ident_con[i0:i1]) == list(ref.ident_con)
            if ref.mixed_or_row:
                assert int(r[H_FMT]) not in (FMT_P16D, FMT_P8D), (name, p)
            if int(ref.rec[H_NV]) == len(probs[p]):  # (no AtMost network's auxiliaries)
                assert int(r[H_NVU]) == (len(probs[p]) if has_pos_row(ref.rec) else 0), (name, p)
            assert _lib.lib().dp_rec_validate(np.ascontiguousarray(r).ctypes.data_as(_lib.c_i32p), len(r)) == 0
    return lws, refs


# ---------------------------------------------------------------------------
# the yardstick itself
# ---------------------------------------------------------------------------
def test_restatement_is_lower_ref_without_or():
    sets = [variables_of(vs) for vs in all_golden_variable_sets()] + [list(vs) for vs in EDGE]
    for vs in sets:
        a, b = lower_or_ref.lower_problem(problem_of(vs)), lower_ref.lower_problem(problem_of(vs))
        assert (a.error, a.msg, list(a.ident_var), list(a.ident_con)) == (b.error, b.msg, list(b.ident_var),
                                                                          list(b.ident_con))
        np.testing.assert_array_equal(a.rec, b.rec)
        assert not a.mixed_or_row and not a.pos_row
    with pytest.raises(ValueError):
        lower_ref.lower_problem(problem_of(TABLE["both-pos"]))


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def test_or_api():
    c = Or("b")
    assert (c.kind, c.ids, c.n) == (sat.OR, (sat.Identifier("b"),), 0) and sat.OR == 6
    assert [Or("b", s, o).n for s in (False, True) for o in (False, True)] == [0, 2, 1, 3]
    assert not c.Anchor() and c.Order() is None
    assert c.String("a") == "a or b"
    assert Or("b", True).String("a") == "not a or b"
    assert Or("b", isOperandNegated=True).String("a") == "a or not b"
    assert Or("b", True, True).String("a") == "not a or not b"
    assert repr(Or("b", True)) == "Or('b', isSubjectNegated=True, isOperandNegated=False)"
    assert Or("b", True) == Or("b", isSubjectNegated=True) != Or("b")


def test_or_reaches_both_wires():
    probs = [TABLE["all-three"], TABLE["with-lists"]]
    wire = sat.encode_inputs(probs)
    kinds = [c.kind for vs in probs for v in vs for c in v.Constraints()]
    ns = [c.n for vs in probs for v in vs for c in v.Constraints()]
    assert list(wire.a["con_kind"]) == kinds and list(wire.a["con_n"]) == ns
    assert {(k, n) for k, n in zip(kinds, ns) if k == 6} == {(6, 0), (6, 1), (6, 2), (6, 3)}
    w32 = _lib.Wire32Arrays(wire, pinned=False)
    assert list(w32.a["con_kn"] & 7) == kinds and list(w32.a["con_kn"] >> 3) == ns
    # ... and through both segments of a shared-catalog call
    k32, q32, qc = sat.encode_shared([probs[0][:2]], [(0, probs[0][2:])], pinned=False)
    ex = _lib.expand_shared(k32, q32, qc)
    one = sat.encode_inputs(probs[:1])
    for k in ("con_kind", "con_n"):
        np.testing.assert_array_equal(ex.a[k], one.a[k])


# ---------------------------------------------------------------------------
# lowering
# ---------------------------------------------------------------------------
def test_table_cases(monkeypatch):
    lws, refs = check_against_restatement(list(TABLE.values()), monkeypatch)
    nid = {name: int(refs[i].rec[H_NID]) for i, name in enumerate(TABLE)}
    assert nid["same-differ"] == 0 and int(refs[list(TABLE).index("same-differ")].rec[H_NC]) == 0
    assert all(nid[k] == 1 for k in ("same-pos", "same-neg", "both-neg", "both-pos", "mixed-subject",
                                     "mixed-operand"))

    def row(name):
        r = refs[list(TABLE).index(name)].rec
        return list(r[16 + 2:16 + 2 + int(r[7])])
    assert row("same-pos") == [0] and row("same-neg") == [1]
    assert row("both-neg") == [1, 3] and row("both-pos") == [0, 2]
    assert row("mixed-subject") == [1, 2] and row("mixed-operand") == [3, 0]
    # the both-negated row is Conflict's, the mixed rows are that Dependency's, byte for byte
    same = {"both-neg": [V("a", Conf("b")), V("b")], "mixed-subject": [V("a", Dep("b")), V("b")],
            "mixed-operand": [V("a"), V("b", Dep("a"))]}
    for name, vs in same.items():
        other = lower_ref.lower_problem(problem_of(vs)).rec
        mine = refs[list(TABLE).index(name)].rec
        o0, m0 = 16, 16
        np.testing.assert_array_equal(mine[m0:m0 + 5], other[o0:o0 + 5])  # clause_off, the row, its identity


@pytest.mark.parametrize("name", list(SHARING))
def test_identity_sharing_and_last_writer(name, monkeypatch):
    vs, owner = SHARING[name]
    lws, refs = check_against_restatement([vs], monkeypatch)
    ref = refs[0]
    assert int(ref.rec[H_NID]) == 1 and int(ref.rec[H_NC]) + int(ref.rec[3]) == 1
    assert (ref.ident_var[0], ref.ident_con[0]) == owner
    for lw in lws.values():
        assert (lw.ident_var[0], lw.ident_con[0]) == owner


def test_longer_dependency_shares_nothing(monkeypatch):
    lws, refs = check_against_restatement([[V("a", Or("b", **SN), Dep("b", "b")), V("b")],
                                           [V("a", Dep("b", "c"), Or("b", **SN)), V("b"), V("c")]], monkeypatch)
    assert [int(r.rec[H_NID]) for r in refs] == [2, 2]


def test_forms_with_implied_lists(monkeypatch):
    """Section 3.1's three cases and the form each gives."""
    cases = {
        "or-first-writer": [V("a", Or("b", **SN)), V("b"), V("c", Dep("a"))],
        "dependency-joins-or": [V("a", Or("b", **SN), Dep("b")), V("b")],
        "or-joins-dependency": [V("a", Dep("b"), Or("b", **SN)), V("b", Or("a", **ON))],
        "both-neg": [V("a", Or("b", **NN), Dep("b")), V("b")],
        "both-pos": [V("a", Or("b"), Dep("b")), V("b")],
    }
    lws, refs = check_against_restatement(list(cases.values()), monkeypatch)
    for path in ("fast", "exact"):
        fm = {name: int(lws["packed", path].record(p)[H_FMT]) for p, name in enumerate(cases)}
        assert fm == {"or-first-writer": FMT_P16, "dependency-joins-or": FMT_P16, "or-joins-dependency": FMT_P8D,
                      "both-neg": FMT_P8D, "both-pos": FMT_P8D}, (path, fm)
        fm = {name: int(lws["no_p8", path].record(p)[H_FMT]) for p, name in enumerate(cases)}
        assert fm == {"or-first-writer": FMT_P16, "dependency-joins-or": FMT_P16, "or-joins-dependency": FMT_P16D,
                      "both-neg": FMT_P16D, "both-pos": FMT_P16D}, (path, fm)
        fm = {name: int(lws["narrow", path].record(p)[H_FMT]) for p, name in enumerate(cases)}
        assert set(fm.values()) == {FMT_U16}
    # the Dependency that joined the Or's identity has a list and no row of its own
    r = refs[1].rec
    assert int(r[H_NC]) == 1 and int(r[4]) == 1


def _random_or_problems(seed, n_problems):
    """Small problems over 4-12 variables with all six kinds; constraints name
    few variables, so identities collide often."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_problems):
        nv = int(rng.integers(4, 13))
        names = ["v%d" % i for i in range(nv)]
        near = int(rng.integers(2, 5))
        vs = []
        for i in range(nv):
            cons = []
            pick = lambda m: [names[(i + int(j)) % nv] for j in rng.integers(0, near, m)]
            for _ in range(int(rng.integers(0, 4))):
                k = int(rng.integers(1, 9))
                if k == 1:
                    cons.append(Mand())
                elif k == 2:
                    cons.append(Proh())
                elif k == 3:
                    cons.append(Dep(*pick(int(rng.integers(0, 3)))))
                elif k == 4:
                    cons.append(Conf(pick(1)[0]))
                elif k == 5:
                    m = int(rng.integers(0, 4))
                    cons.append(AtMost(int(rng.integers(-1, m + 1)), *pick(m)))
                else:
                    fl = int(rng.integers(0, 4))
                    cons.append(Or(pick(1)[0], bool(fl & 1), bool(fl & 2)))
            vs.append(V(names[i], *cons))
        out.append(vs)
    return out


RANDOM_SEED, RANDOM_N = 20, 2000


def random_or_problems():
    return _random_or_problems(RANDOM_SEED, RANDOM_N)


def sharing_counts(refs):
    """How often each pair of the issue's list shares an identity, by (first writer, joiner)."""
    D1, A2 = (3, 1), (5, 2)
    pairs = {"nn>conflict": ((6, 3), (4, 0)), "conflict>nn": ((4, 0), (6, 3)), "nn>atmost": ((6, 3), A2),
             "atmost>nn": (A2, (6, 3)), "pos>pos": ((6, 0), (6, 0)), "same>mandatory": ((6, 0), (1, 0)),
             "mandatory>same": ((1, 0), (6, 0)), "same>prohibited": ((6, 3), (2, 0)),
             "prohibited>same": ((2, 0), (6, 3))}
    n = {k: 0 for k in pairs}
    n["mixed>dep"] = n["dep>mixed"] = 0
    for ref in refs:
        for first, join in ref.shared:
            for k, pr in pairs.items():
                n[k] += (first, join) == pr
            n["mixed>dep"] += first in ((6, 1), (6, 2)) and join == D1
            n["dep>mixed"] += first == D1 and join in ((6, 1), (6, 2))
    return n


def test_random_problems_three_ways(monkeypatch):
    probs = random_or_problems()
    refs = [lower_or_ref.lower_problem(problem_of(vs)) for vs in probs]
    # what the restatement alone says of the sample: explicit and implied
    # forms, every kind of sharing, errors and all-positive rows
    ok = [r for r in refs if not r.error]
    assert sum(r.mixed_or_row for r in ok) > 100 and sum(not r.mixed_or_row for r in ok) > 100
    assert sum(r.pos_row for r in ok) > 100 and sum(bool(r.error) for r in refs) == 0
    counts = sharing_counts(refs)
    assert all(v >= 1 for v in counts.values()), counts
    lws, _ = check_against_restatement(probs, monkeypatch, refs)
    fmts = np.array([int(lws["packed", "fast"].record(p)[H_FMT]) for p in range(len(probs))])
    assert (fmts == FMT_P8D).sum() > 100 and (fmts == FMT_P16).sum() > 100
    # no problem is on the exact path but for an Or of mixed signs over two
    # variables or today's reasons (a repeated AtMost variable among them)
    mixed = sum(any(c.kind == 6 and c.n in (1, 2) and c.ids[0] != v.Identifier() for v in vs for c in v.Constraints())
                for vs in probs)
    assert 0 < lws["int32", "fast"].n_exact < len(probs) and mixed > 0


def test_nvu_unchanged_without_or():
    sets = [variables_of(vs) for vs in all_golden_variable_sets()]
    for fl in FLAGSETS.values():
        lw = _lib.Lowered(sat.encode_inputs(sets), **fl)
        assert all(int(lw.record(p)[H_NVU]) == 0 for p in range(lw.n))
        w = _lib.generate(2, 60, 5)
        lw = _lib.Lowered(_lib.WireArrays(**{k: w[k] for k in (
            "prob_var_off", "var_id", "var_con_off", "con_kind", "con_n", "con_arg_off", "con_arg", "str_off")},
            str_bytes=w["str_bytes"].tobytes()), **fl)
        assert all(int(lw.record(p)[H_NVU]) == 0 for p in range(lw.n))


# ---------------------------------------------------------------------------
# refusals and errors
# ---------------------------------------------------------------------------
def _malformed():
    ident = sat.Identifier
    yield "flags-4", [V("a", sat.Constraint(sat.OR, (ident("b"),), 4)), V("b")]
    yield "flags-negative", [V("a", sat.Constraint(sat.OR, (ident("b"),), -1)), V("b")]
    yield "no-argument", [V("a", sat.Constraint(sat.OR, (), 0)), V("b")]
    yield "two-arguments", [V("a", sat.Constraint(sat.OR, (ident("b"), ident("a")), 0)), V("b")]
    yield "kind-7", [V("a", sat.Constraint(7, (ident("b"),), 0)), V("b")]
    yield None, [V("a", Or("b")), V("b")]


@pytest.mark.parametrize("exact", [False, True])
def test_malformed_or_is_refused_on_both_wires(exact, monkeypatch):
    """The 64-bit wire, and the compact wire as it reaches the host lowering
    (dp_expand_shared: in the query's segment and in the catalog's)."""
    if exact:
        monkeypatch.setenv("DEPPY_LOWER_EXACT", "1")
    for name, vs in _malformed():
        wires = [sat.encode_inputs([vs])]
        for catalogs, queries in (([], [(None, vs)]), ([vs], [(0, [V("q")])])):
            k32, q32, qc = sat.encode_shared(catalogs, queries, pinned=False)
            wires.append(_lib.expand_shared(k32, q32, qc))
        for w in wires:
            if name is None:
                assert _lib.Lowered(w).err[0] == 0
                continue
            with pytest.raises(ValueError, match="malformed"):
                _lib.Lowered(w)
            with pytest.raises(ValueError, match="malformed"):
                _lib.Lowered(w, narrow=True, packed=True)


def test_missing_operand_is_a_lookup_error(monkeypatch):
    probs = [[V("a", Or('no"pe', **SN)), V("b", Conf("gone"), Or("é", **NN))],
             [V("a", Conf('no"pe')), V("b", Conf("gone"), Conf("é"))]]
    lws, refs = check_against_restatement(probs, monkeypatch)
    assert refs[0].error == 2 and refs[0].msg == refs[1].msg
    assert refs[0].msg == ('3 errors encountered: variable "no\\"pe" referenced but not provided, '
                           'variable "gone" referenced but not provided, variable "é" referenced but not provided')


# ---------------------------------------------------------------------------
# the oracle on Or problems, against brute force
# ---------------------------------------------------------------------------
def _holds(c, s, val, index):
    """constraint c on subject s under the assignment val (the definitions)."""
    ids = [index[i] for i in c.ids]
    if c.kind == 1:
        return val[s]
    if c.kind == 2:
        return not val[s]
    if c.kind == 3:
        return not val[s] or any(val[d] for d in ids)
    if c.kind == 4:
        return not (val[s] and val[ids[0]])
    if c.kind == 5:
        return sum(val[d] for d in ids) <= c.n
    return (val[s] != bool(c.n & 1)) or (val[ids[0]] != bool(c.n & 2))


def _satisfiable(cons, index, nv):
    return any(all(_holds(c, s, val, index) for s, c in cons) for val in itertools.product((False, True), repeat=nv))


def test_oracle_on_or_problems_against_brute_force():
    probs = [vs for vs in random_or_problems() if len(vs) <= 10][:400] + list(TABLE.values()) + \
        [vs for vs, _ in SHARING.values()] + [
        [V("a", Mand(), Or("b", **SN)), V("b", Proh())],
        [V("a", Or("b")), V("b", Proh()), V("c", Or("a", **NN), Mand(), Or("b", **ON), Dep("a"))]]
    lw = _lib.Lowered(sat.encode_inputs(probs))
    assert (lw.err == 0).all()
    n_sat = n_unsat = or_in_core = 0
    for p, vs in enumerate(probs):
        nv = len(vs)
        index = {v.Identifier(): i for i, v in enumerate(vs)}
        allc = [(s, c) for s, v in enumerate(vs) for c in v.Constraints()]
        rec = lw.record(p)
        if int(rec[H_NV]) != nv:
            continue  # (an AtMost network: auxiliaries, covered by its own suite)
        st, _, installed, core, _ = oracle.solve(rec)
        truth = _satisfiable(allc, index, nv)
        assert st == (1 if truth else -1), p
        if st == 1:
            n_sat += 1
            val = [i in installed for i in range(nv)]
            assert all(_holds(c, s, val, index) for s, c in allc), p
            assert all(val[s] for s, c in allc if c.kind == 1)
            continue
        n_unsat += 1
        i0 = lw.ident_off[p]
        applied = [(int(lw.ident_var[i0 + i]), vs[lw.ident_var[i0 + i]].Constraints()[lw.ident_con[i0 + i]])
                   for i in core]
        assert not _satisfiable(applied, index, nv), p
        for j in range(len(applied)):  # deletion-minimal
            assert _satisfiable(applied[:j] + applied[j + 1:], index, nv), (p, j)
        err = sat.NotSatisfiable([sat.AppliedConstraint(vs[s], c) for s, c in applied])
        for s, c in applied:
            if c.kind == 6:
                or_in_core += 1
                assert c.String(vs[s].Identifier()) in err.Error() and " or " in c.String(vs[s].Identifier())
    assert n_sat > 50 and n_unsat > 50 and or_in_core > 10, (n_sat, n_unsat, or_in_core)
