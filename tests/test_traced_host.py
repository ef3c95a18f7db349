"""The host half of the traced fused path, without a GPU: the owners walk
that the pack kernel runs (dp_trace_owners_host, trace_walk.hpp), the Python
decoder of its output, and the argument checks of the two entry points."""
import ctypes

import numpy as np

from deppy_amd import _lib, sat
from oracle import oracle
from tests.gpu_common import lowered_config
from tests.test_lowering import V

CAP = 4096
CANARY = -77777


def owners_numpy(t, nid, ivs, ics):
    """The walk restated: owners of every whole event's identity words; -1 at
    every other word and from the first malformed event on."""
    n = len(t)
    var = np.full(n, -1, np.int32)
    con = np.full(n, -1, np.int32)
    i = 0
    while i < n:
        k = int(t[i])
        if k < 0 or i + 1 + k >= n:
            break
        m = int(t[i + 1 + k])
        a = i + 2 + k
        if m < 0 or a + m > n:
            break
        ids = t[a:a + m].astype(np.int64)
        ok = (ids >= 0) & (ids < nid)
        var[a:a + m][ok] = ivs[ids[ok]]
        con[a:a + m][ok] = ics[ids[ok]]
        i = a + m
    return var, con


def owners_host(t, nid, ivs, ics):
    """dp_trace_owners_host with canaries either side of both outputs."""
    n, pad = len(t), 8
    t = np.ascontiguousarray(t, np.int32)
    ivs = np.ascontiguousarray(ivs, np.int32)
    ics = np.ascontiguousarray(ics, np.int32)
    outs = [np.full(n + 2 * pad, CANARY, np.int32) for _ in range(2)]
    p = ctypes.POINTER(ctypes.c_int32)
    arg = lambda a, off=0: ctypes.cast(a.ctypes.data + 4 * off, p)
    rc = _lib.lib().dp_trace_owners_host(arg(t), n, nid, arg(ivs), arg(ics), arg(outs[0], pad), arg(outs[1], pad))
    assert rc == 0
    for o in outs:
        assert (o[:pad] == CANARY).all() and (o[pad + n:] == CANARY).all()
    return outs[0][pad:pad + n], outs[1][pad:pad + n]


def random_streams():
    """2,000 streams, seed 1: well-formed events mixed with an identity at
    nid and past it, a negative n, an m past the end, a length of 0 and a
    final partial event."""
    rng = np.random.default_rng(1)
    out = []
    for k in range(2000):
        nid = int(rng.integers(0, 40))
        words = []
        for _ in range(int(rng.integers(0, 6))):
            n, m = int(rng.integers(0, 5)), int(rng.integers(0, 6))
            ids = rng.integers(0, max(nid, 1), m).tolist()
            words += [n] + rng.integers(0, 50, n).tolist() + [m] + ids
        t = np.array(words, np.int64)
        kind = k % 8
        if kind == 1 and len(t):  # an identity at nid, one past it, a negative one
            t[rng.integers(0, len(t))] = nid + int(rng.integers(0, 2))
            t[rng.integers(0, len(t))] = -3
        elif kind == 2 and len(t):  # a negative n up front
            t[0] = -1
        elif kind == 3 and len(t):  # an m past the end
            t[rng.integers(0, len(t))] = 1 << 20
        elif kind == 4:  # a length of 0
            t = t[:0]
        elif kind == 5 and len(t) > 1:  # a final partial event
            t = t[:len(t) - int(rng.integers(1, min(4, len(t))))]
        elif kind == 6:  # a header alone, and a count of INT32_MAX
            t = np.concatenate([t, [0x7fffffff]])
        out.append((t.astype(np.int32), nid, rng.integers(0, 500, nid + 1).astype(np.int32),
                    rng.integers(0, 9, nid + 1).astype(np.int32)))
    return out


def test_owners_walk_on_oracle_traces():
    lw = lowered_config(2, 300, 5)
    o = oracle.solve_batch(lw.rec_off, lw.rec, 0, 8, trace_cap=CAP)
    traced = ident_words = 0
    for p in range(lw.n):
        t = o["trace"][p][:int(o["trace_len"][p])]
        i0, i1 = int(lw.ident_off[p]), int(lw.ident_off[p + 1])
        ivs, ics = lw.ident_var[i0:i1], lw.ident_con[i0:i1]
        var, con = owners_host(t, i1 - i0, ivs, ics)
        evar, econ = owners_numpy(t, i1 - i0, ivs, ics)
        np.testing.assert_array_equal(var, evar)
        np.testing.assert_array_equal(con, econ)
        # and through the decoder: the oracle's identities, mapped
        res = dict(trace_off=np.array([0, len(t)]), trace=t, trace_var=var, trace_con=con)
        want = [(vs, [(int(ivs[i]), int(ics[i])) for i in ids]) for vs, ids in _lib.trace_events(o, p)]
        assert _lib.fused_trace_events(res, 0) == want
        traced += len(t) > 0
        ident_words += int((var >= 0).sum())
    assert traced >= 50 and ident_words >= 300, (traced, ident_words)


def test_owners_walk_on_random_streams():
    stopped = 0
    for t, nid, ivs, ics in random_streams():
        var, con = owners_host(t, nid, ivs, ics)
        evar, econ = owners_numpy(t, nid, ivs, ics)
        np.testing.assert_array_equal(var, evar)
        np.testing.assert_array_equal(con, econ)
        stopped += len(t) > 0 and (len(_events_words(t)) != len(t))
    assert stopped >= 200  # the malformed streams are in the mix


def _events_words(t):
    """The words of t's whole events (numpy restatement of the decoder's stop)."""
    i, n = 0, len(t)
    while i < n:
        k = int(t[i])
        if k < 0 or i + 1 + k >= n:
            break
        m = int(t[i + 1 + k])
        if m < 0 or i + 2 + k + m > n:
            break
        i += 2 + k + m
    return t[:i]


def test_fused_trace_events_returns_whole_events_only():
    for t, nid, ivs, ics in random_streams():
        var, con = owners_numpy(t, nid, ivs, ics)
        res = dict(trace_off=np.array([0, len(t)]), trace=t, trace_var=var, trace_con=con)
        ev = _lib.fused_trace_events(res, 0)  # (never raises)
        whole = _events_words(t)
        assert sum(2 + len(vs) + len(own) for vs, own in ev) == len(whole)
        flat = []
        for vs, own in ev:
            flat += [len(vs)] + vs + [len(own)]
            a = len(flat)
            assert own == [(int(var[a + k]), int(con[a + k])) for k in range(len(own))]
            flat += whole[a:a + len(own)].tolist()
        assert flat == whole.tolist()


def test_argument_checks_without_a_device():
    L = _lib.lib()
    so, tr = _lib.Solved(), _lib.Traced()
    assert L.dp_lower_solve_traced(None, None, CAP, None, None) == -1
    assert L.dp_lower_solve_traced(None, None, CAP, ctypes.byref(so), ctypes.byref(tr)) == -1
    assert L.dp_lower_solve_shared_traced(None, None, None, None, CAP, None, None) == -1
    assert L.dp_lower_solve_shared_traced(None, None, None, None, CAP, ctypes.byref(so), ctypes.byref(tr)) == -1
    assert b"null argument" in L.dp_last_global_error()
    for cap in (0, -1, (1 << 24) + 1):
        assert L.dp_lower_solve_traced(None, None, cap, ctypes.byref(so), ctypes.byref(tr)) == -1
        assert b"dp_lower_solve_traced: trace_cap" in L.dp_last_global_error()
        assert L.dp_lower_solve_shared_traced(None, None, None, None, cap, ctypes.byref(so), ctypes.byref(tr)) == -1
        assert b"dp_lower_solve_shared_traced: trace_cap" in L.dp_last_global_error()
    assert sat.TRACE_CAP_MAX == 1 << 24


def test_default_tracer_takes_the_untraced_route(monkeypatch):
    caps = []

    def fake(self, k32, q32, qc, trace_cap=0):
        caps.append(trace_cap)
        n = q32.n_problems
        return dict(err=np.zeros(n, np.int32), msg=[None] * n, status=np.zeros(n, np.int8),
                    flags=np.zeros(n, np.int32))

    dl = object.__new__(_lib.DeviceLowerer)
    dl.h = None
    monkeypatch.setattr(_lib.DeviceLowerer, "lower_solve_shared", fake)
    monkeypatch.setattr(sat, "_device_lowerer", lambda ctx: dl)
    monkeypatch.setattr(sat, "device_context", lambda: object())
    catalog = [V("a", sat.Mandatory()), V("b")]
    queries = [[V("q", sat.Dependency("a"))], []]
    for tracer in (None, sat.DefaultTracer()):
        out = sat.SolveQueries(catalog, queries, tracer=tracer)
        assert [e for _, e in out] == [sat.ErrIncomplete] * 2
    assert caps == [0, 0]

    class Rec(sat.Tracer):
        def Trace(self, pos):
            pass

    fused = dict(trace_off=np.zeros(3, np.int64), trace=np.zeros(0, np.int32), trace_var=np.zeros(0, np.int32),
                 trace_con=np.zeros(0, np.int32))
    monkeypatch.setattr(_lib.DeviceLowerer, "lower_solve_shared",
                        lambda self, k32, q32, qc, trace_cap=0: dict(fake(self, k32, q32, qc, trace_cap), **fused))
    sat.SolveQueries(catalog, queries, tracer=Rec())
    assert caps == [0, 0, sat.TRACE_CAP]
