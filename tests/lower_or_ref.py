"""The restated lowering (oracle/lower_ref.py lower_problem) with the Or
constraint, kind 6: the yardstick of the records that hold one.

Or is an extension the reference snapshot does not have, so lower_ref raises
on it; this module restates lower_problem's loop with the one more case and
takes everything else -- the And-inverter graph, the row emission of the five
reference kinds, the record builder -- from lower_ref.  On problems without an
Or it gives lower_ref's result (tests/test_or_lowering.py checks that).

Or(operand, flags) on subject s: the gate literal Or(ls, lo) with ls = x_s
(negated by flag bit 0) and lo = x_operand (negated by bit 1).  It is no
anchor and has no choice list.  Its row, when it is its identity's first
writer: the unit (ls) when the gate folds to an input literal; none when it
folds to T; else (ls lo), the negative literal first when exactly one is
negative (so the row equals Dependency(a; b)'s, whoever writes first).  A
record that holds a row of two positive literals carries DP_H_NVU = nv.
"""
from __future__ import annotations

from oracle.lower_ref import (AIG, ATMOST, CONFLICT, DEPENDENCY, MANDATORY, PROHIBITED, T, Lowered, _emit_rows,
                              build_record, empty_record, go_quote)

OR = 6


class LoweredOr(Lowered):
    """Lowered, and what decides the record's form: mixed_or_row (a
    mixed-polarity Or is some identity's first writer, so its row lies in the
    record with a Dependency row's shape and no choice list: the lists must be
    explicit) and pos_row (a row of two positive literals: DP_H_NVU)."""
    __slots__ = ("mixed_or_row", "pos_row", "shared")


def lower_problem(variables) -> LoweredOr:
    """variables: list of (identifier: bytes, constraints: list of (kind, n, [bytes]));
    an Or is (6, flags, [operand])."""
    def done(*a):
        lo = LoweredOr(*a)
        lo.mixed_or_row = lo.pos_row = False
        lo.shared = []
        return lo

    index: dict[bytes, int] = {}
    for i, (vid, _) in enumerate(variables):
        if vid in index:
            return done(empty_record(), [], [], 1, "duplicate identifier %s in input" % go_quote(vid))
        index[vid] = i
    nv = len(variables)
    errs: list[str] = []

    def lit_of(x: bytes):
        v = index.get(x)
        if v is None:
            errs.append("variable %s referenced but not provided" % go_quote(x))
        return v

    aig = AIG(nv)
    key_ident: dict[int, int] = {}
    ident_owner: list[list[int]] = []
    first_kind: list[tuple] = []  # per identity: (kind, flags) of its first writer
    shared: list[tuple] = []      # (first writer's (kind, flags), joining (kind, flags)) per join
    clauses: list[tuple[list[int], int]] = []
    cards: list[tuple[list[int], int, int]] = []
    aux: list[int] = [nv]
    mixed_or_row = pos_row = False

    for vi, (vid, cons) in enumerate(variables):
        s = vi
        for ci, (kind, n, args) in enumerate(cons):
            bad = False
            m = T
            if kind == MANDATORY:
                m = aig.input(s)
            elif kind == PROHIBITED:
                m = aig.input(s) ^ 1
            elif kind == DEPENDENCY:
                m = aig.input(s) ^ 1
                for a in args:
                    d = lit_of(a)
                    if d is None:
                        bad = True
                        continue
                    m = aig.or_(m, aig.input(d))
            elif kind == CONFLICT:
                t = lit_of(args[0])
                if t is None:
                    bad = True
                else:
                    m = aig.or_(aig.input(s) ^ 1, aig.input(t) ^ 1)
            elif kind == ATMOST:
                ms = []
                for a in args:
                    d = lit_of(a)
                    if d is None:
                        bad = True
                        continue
                    ms.append(aig.input(d))
                if not bad:
                    m = AIG.leq(aig.cardsort(ms), len(ms), n)
            elif kind == OR:
                assert len(args) == 1 and 0 <= n <= 3
                t = lit_of(args[0])
                if t is None:
                    bad = True
                else:
                    m = aig.or_(aig.input(s) ^ (n & 1), aig.input(t) ^ (n >> 1))
            else:
                raise ValueError("unknown constraint kind %r" % kind)
            if bad or errs or m == T:
                continue
            tag = (kind, n if kind == OR else len(args) if kind in (DEPENDENCY, ATMOST) else 0)
            ident = key_ident.get(m)
            if ident is not None:
                ident_owner[ident] = [vi, ci]
                shared.append((first_kind[ident], tag))
                continue
            ident = len(ident_owner)
            key_ident[m] = ident
            ident_owner.append([vi, ci])
            first_kind.append(tag)
            if kind != OR or m >> 1 <= nv:  # the reference kinds; an Or folded to an input literal
                _emit_rows(m, nv, kind, s, n, args, index, ident, clauses, cards, aig, aux)
                continue
            ls, lo = 2 * s + (n & 1), 2 * index[args[0]] + (n >> 1)
            clauses.append(([lo, ls] if n == 2 else [ls, lo], ident))
            mixed_or_row |= n in (1, 2)
            pos_row |= n == 0
    if errs:
        return done(empty_record(), [], [], 2, "%d errors encountered: %s" % (len(errs), ", ".join(errs)))

    var_choice_off = [0]
    choice_off = [0]
    choice_lits: list[int] = []
    anchors = []
    for vi, (vid, cons) in enumerate(variables):
        for kind, n, args in cons:
            if kind == DEPENDENCY and len(args) > 0:
                choice_lits.extend(index[a] for a in args)
                choice_off.append(len(choice_lits))
        var_choice_off.append(len(choice_off) - 1)
        if any(kind == MANDATORY for kind, _, _ in cons):
            anchors.append(vi)
    var_choice_off += [var_choice_off[-1]] * (aux[0] - nv)
    rec = build_record(aux[0], clauses, cards, var_choice_off, choice_off, choice_lits, anchors,
                       len(ident_owner), nv if aux[0] > nv or pos_row else 0)
    lo = done(rec, [o[0] for o in ident_owner], [o[1] for o in ident_owner])
    lo.mixed_or_row, lo.pos_row, lo.shared = mixed_or_row, pos_row, shared
    return lo


def problem_of(vs) -> list:
    """sat variables -> lower_problem's input."""
    return [(v.Identifier().encode(), [(c.kind, c.n, [i.encode() for i in c.ids]) for c in v.Constraints()])
            for v in vs]
