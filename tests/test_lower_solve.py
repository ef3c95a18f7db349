"""Fused device lowering and solve (dp_lower_solve): the compact wire in,
results out, with the lowering's records and identity owners left in device
memory.  The yardstick everywhere is the host lowering from the 64-bit wire,
sat.solve_wire(wire64, ctx): every dp_solved array equals its results, and
the owner pairs equal its ident_var / ident_con mapped through the cores."""
import io

import numpy as np
import pytest

from deppy_amd import _lib, sat
from tests import fixtures
from tests.test_device_lowering import assert_same, wire_of
from tests.test_lowering import EDGE, V, _random_problems, all_golden_variable_sets, variables_of

pytestmark = pytest.mark.gpu

FMT = 13  # DP_H_FMT
RESULT_KEYS = ("status", "flags", "steps", "core_len", "inst_off", "core_off")


@pytest.fixture(scope="module")
def dl():
    ctx = _lib.Context(0, 1)
    d = _lib.DeviceLowerer(ctx)
    yield d
    d.close()
    ctx.close()


def yardstick(wire, ctx):
    """Host lowering + dp_solve, copied (the storage is reused per thread)."""
    lw, res = sat.solve_wire(wire, ctx)
    ref = {k: np.array(res[k]) for k in RESULT_KEYS + ("installed", "core")}
    ref.update(ident_off=np.array(lw.ident_off), ident_var=np.array(lw.ident_var), ident_con=np.array(lw.ident_con),
               err=np.array(lw.err), msg=list(lw.msg), fmt=np.array(lw.rec[lw.rec_off[:-1] + FMT]))
    return ref


def core_index(r):
    """(problem, position in the core arrays) of every reported core entry."""
    ps = np.flatnonzero(r["core_len"] > 0)
    if not len(ps):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    lens = r["core_len"][ps].astype(np.int64)
    prob = np.repeat(ps, lens)
    k = np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    return prob, r["core_off"][prob] + k


def assert_equal(got, ref):
    n = len(ref["status"])
    assert len(got["status"]) == n
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(got["installed"], ref["installed"][:int(ref["inst_off"][-1])])
    np.testing.assert_array_equal(got["core"], ref["core"][:int(ref["core_off"][-1])])
    np.testing.assert_array_equal(got["err"], ref["err"])
    assert got["msg"] == ref["msg"]
    prob, at = core_index(ref)
    ident = ref["ident_off"][prob] + ref["core"][at]
    np.testing.assert_array_equal(got["core_var"][at], ref["ident_var"][ident])
    np.testing.assert_array_equal(got["core_con"][at], ref["ident_con"][ident])


def solve_both(dl, wire, ids16=True):
    ref = yardstick(wire, dl.ctx)
    got = dl.lower_solve(_lib.Wire32Arrays(wire, ids16=ids16))
    return got, ref


@pytest.mark.parametrize("config,n,ids16", [(2, 3000, True), (2, 700, False), (3, 5000, True), (6, 2000, True),
                                            (5, 300, True)])
def test_fused_results_equal_host_lowered(dl, config, n, ids16):
    got, ref = solve_both(dl, wire_of(config, n, 77), ids16)
    assert_equal(got, ref)
    print("config", config, "host-lowered", got["host_lowered"], "of", n, "h2d", got["h2d_bytes"], "d2h",
          got["d2h_bytes"])
    assert got["host_lowered"] == (n if config == 5 else 0)


def colliding_problems():
    probs = []
    for seed in (1, 2, 3, 5, 11):
        probs += _random_problems(seed, 400)
    return probs + EDGE + [variables_of(vs) for vs in all_golden_variable_sets()]


def test_fused_colliding_and_error_problems(dl):
    """Problems the kernel leaves to the host (colliding keys, lookup errors,
    duplicate identifiers) are lowered there and solved beside the fused
    windows; results, errors and texts merge by problem index."""
    probs = colliding_problems()
    got, ref = solve_both(dl, sat.encode_inputs(probs))
    assert_equal(got, ref)
    assert ref["err"].any()
    assert 0 < got["host_lowered"] < len(probs), got["host_lowered"]


def unsat_goldens():
    return [c["variables"] for c in fixtures.load("testsolve")["cases"] if c["error"] is not None]


def test_fused_cores_on_the_device_path(dl):
    """NotSatisfiable problems lowered by the kernel: their owner pairs come
    from the device's owner arrays through the owners kernel.  Whether the
    kernel takes a problem depends on that problem alone, so each golden case
    is asked once on its own."""
    cases = [variables_of(vs) for vs in unsat_goldens()]
    taken = [dl.lower_solve(_lib.Wire32Arrays(sat.encode_inputs([c])))["host_lowered"] == 0 for c in cases]
    w2 = _lib.generate(2, 40, 5)
    probs, on_device = [], []
    for k in range(50):
        probs += cases
        on_device += taken
        if k < 40:
            probs.append(fixtures.wire_problem_variables(w2, k))
            on_device.append(True)
    wire = sat.encode_inputs(probs)
    got, ref = solve_both(dl, wire)
    assert_equal(got, ref)
    on_device = np.array(on_device)
    assert got["host_lowered"] == int((~on_device).sum())
    fused_unsat = np.flatnonzero((ref["status"] == -1) & (ref["core_len"] >= 2) & on_device)
    assert len(fused_unsat) >= 100, len(fused_unsat)
    prob, at = core_index(ref)
    sel = np.isin(prob, fused_unsat)
    ident = ref["ident_off"][prob[sel]] + ref["core"][at[sel]]
    np.testing.assert_array_equal(got["core_var"][at[sel]], ref["ident_var"][ident])
    np.testing.assert_array_equal(got["core_con"][at[sel]], ref["ident_con"][ident])


def p16_problem(k):
    """6 Dependencies of 240 candidates each, one candidate repeated: the rows
    do not imply the choice lists, so the record is DP_FMT_P16."""
    cands = ["c%d" % i for i in range(239)]
    vs = []
    for s in range(6):
        ids = cands[s:] + cands[:s]
        rep = ids[(k + s) % 239]
        cons = [sat.Dependency(*(ids + [rep]))]
        if s == k % 6:
            cons.append(sat.Mandatory())
        vs.append(V("s%d" % s, *cons))
    return vs + [V(c) for c in cands]


def test_fused_p16_only_batch(dl):
    wire = sat.encode_inputs([p16_problem(k) for k in range(64)])
    got, ref = solve_both(dl, wire)
    assert (ref["fmt"] == 3).all(), np.unique(ref["fmt"])
    print("P16 batch host-lowered", got["host_lowered"])
    assert_equal(got, ref)


def test_fused_windows(dl, monkeypatch):
    wire = wire_of(2, 700, 21)
    w32 = _lib.Wire32Arrays(wire)
    ref = yardstick(wire, dl.ctx)
    whole = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dl.lower_solve(w32).items()}
    assert_equal(whole, ref)
    monkeypatch.setenv("DEPPY_FUSED_WINDOW", "256")
    got = dl.lower_solve(w32)
    assert_equal(got, ref)
    for k in RESULT_KEYS + ("installed", "core", "core_var", "core_con"):
        np.testing.assert_array_equal(got[k], whole[k])
    one = wire_of(2, 1, 22)
    got, ref = solve_both(dl, one)
    assert_equal(got, ref)
    none = dl.lower_solve(_lib.Wire32Arrays(sat.encode_inputs([])))
    assert len(none["status"]) == 0 and list(none["inst_off"]) == [0] and list(none["core_off"]) == [0]
    assert none["host_lowered"] == 0 and len(none["core"]) == 0


def test_fused_reuse_and_malformed_wire(dl):
    for cfg, n, seed in ((2, 3000, 1), (3, 5000, 2), (2, 700, 3), (6, 2000, 4)):
        got, ref = solve_both(dl, wire_of(cfg, n, seed))
        assert_equal(got, ref)
    wire = wire_of(2, 50, 4)
    bad = _lib.WireArrays(**{k: v.copy() for k, v in wire.a.items() if k != "str_bytes"},
                          str_bytes=wire.a["str_bytes"][:-1].tobytes())
    bad.a["con_arg"][5] = len(bad.a["str_off"]) + 3  # a string index past the table
    with pytest.raises(ValueError, match="malformed wire batch"):
        dl.lower_solve(_lib.Wire32Arrays(bad))
    got, ref = solve_both(dl, wire)
    assert_equal(got, ref)


def test_lower_and_lower_solve_share_a_lowerer(dl, monkeypatch):
    """dp_lower_device and dp_lower_solve stage the wire in the same device
    buffers of one lowerer: alternated over batches that change index width
    and go large, small, large again (the fused calls through both windows),
    every lowering equals dp_lower_into's byte for byte and every fused
    result the host-lowered yardstick."""
    monkeypatch.setenv("DEPPY_FUSED_WINDOW", "256")
    for config, n, ids16 in ((2, 600, True), (6, 200, False), (3, 900, True), (2, 150, False)):
        wire = wire_of(config, n, 31)
        w32 = _lib.Wire32Arrays(wire, ids16=ids16)
        host = _lib.Lowered(wire, narrow=True, pinned=True, packed=True)
        ref = yardstick(wire, dl.ctx)
        assert_same(dl.lower(w32, _lib.Lowered.empty(pinned=True)), host)
        assert_equal(dl.lower_solve(w32), ref)
        assert_same(dl.lower(w32, _lib.Lowered.empty(pinned=True)), host)
        assert dl.host_count == 0


def test_fused_byte_accounting(dl):
    """Per config-2 catalog about 170 bytes come back (32 result, at most 64
    installed, 72 header and counts, a few small cores) instead of the
    records and every identity's owners; to the device go the wire and the
    launch tables."""
    n = 3000
    w32 = _lib.Wire32Arrays(wire_of(2, n, 77))
    got = dl.lower_solve(w32)
    print("per catalog: d2h", got["d2h_bytes"] / n, "h2d", got["h2d_bytes"] / n, "wire", w32.nbytes() / n)
    assert got["host_lowered"] == 0
    assert 72 * n < got["d2h_bytes"] <= 256 * n
    assert w32.nbytes() <= got["h2d_bytes"] <= w32.nbytes() + 64 * n + 65536


def outcome(variables, r):
    installed, err = r
    ids = [str(v.Identifier()) for v in installed] if installed else None
    if isinstance(err, sat.NotSatisfiable):
        applied = sorted(((str(a.Variable.Identifier()).encode(), a.Variable.Constraints().index(a.Constraint))
                          for a in err))
        return ids, "NotSatisfiable", applied
    return ids, type(err).__name__, (err.Error() if hasattr(err, "Error") else str(err))


def test_solve_batch_fused_equals_unfused():
    inputs = [variables_of(vs) for vs in all_golden_variable_sets()] + _random_problems(7, 400)
    plain = sat.SolveBatch(inputs)
    fused = sat.SolveBatch(inputs, fused=True)
    assert len(plain) == len(fused) == len(inputs)
    kinds = set()
    for p, variables in enumerate(inputs):
        a, b = outcome(variables, plain[p]), outcome(variables, fused[p])
        assert a == b, p
        kinds.add(a[1])
    assert {"NotSatisfiable", "NoneType"} <= kinds
    # with a tracer, fused=True takes the traced path: the same trace
    w5 = _lib.generate(5, 20, 61)  # (UNSAT-heavy: their searches have unsatisfiable steps to trace)
    traced = [variables_of(vs) for vs in unsat_goldens()] + [fixtures.wire_problem_variables(w5, p) for p in range(20)]
    t0, t1 = io.StringIO(), io.StringIO()
    r0 = sat.SolveBatch(traced, tracer=sat.LoggingTracer(t0))
    r1 = sat.SolveBatch(traced, tracer=sat.LoggingTracer(t1), fused=True)
    assert t0.getvalue() == t1.getvalue() and t0.getvalue()
    assert [outcome(v, r) for v, r in zip(traced, r0)] == [outcome(v, r) for v, r in zip(traced, r1)]
