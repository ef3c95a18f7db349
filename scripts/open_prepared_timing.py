"""Query batches over open catalogs -- catalogs with constraints on an
identifier that only the query defines -- legs alternated in one process:

  (a) lower_solve_shared: the catalogs' wire per call, each query's workgroup
      lowers its whole expanded problem
  (b) lower_solve on a handle from the plain prepare: no catalog copy, but the
      catalogs are not closed, so none is prepared (status 0) and each query's
      workgroup lowers its whole expanded problem all the same
  (c) lower_solve on a handle prepared with DP_PREPARE_OPEN: each query's
      workgroup resumes from its catalog's state and finishes the deferred
      constraints

usage: open_prepared_timing.py [QUERIES [STEPS [WARMUP [REPEATS]]]]
(defaults, as prepared_timing.py's: 10000 queries and then 64 queries per
call, 20 timed steps after 5 warm-up steps, 5 repeats).  prepared_timing.py's
16 closed config-2 catalogs, in each of which eight variables get a
Conflict("env"); its queries of two variables that name three catalog
identifiers, each with a third variable, env.  (b)'s and (c)'s results are
checked against (a)'s before anything is timed.  Prints ms per call per
repeat, the median and min-max spread per leg, and the deferred constraints
per catalog.  Run on the GPU box."""
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deppy_amd import _lib, sat  # noqa: E402

argv = [int(x) for x in sys.argv[1:]] + [None] * 4
sizes = (argv[0],) if argv[0] is not None else (10000, 64)
steps, warmup, repeats = (a if a is not None else d for a, d in zip(argv[1:], (20, 5, 5)))
N_CAT, N_OPEN = 16, 8
KEYS = ("status", "flags", "steps", "core_len", "inst_off", "core_off", "installed", "core", "core_var", "core_con", "err")


class Var(sat.Variable):
    def __init__(self, ident, cons):
        self.ident, self.cons = sat.Identifier(ident), cons

    def Identifier(self):
        return self.ident

    def Constraints(self):
        return self.cons


def open_catalog(w, p):
    """Problem p of a generated wire as Variables, without the arguments that
    are not identifiers of the problem itself (prepared_timing.py's
    closed_catalog), and with a Conflict("env") on N_OPEN of its variables,
    evenly spread."""
    so, sb = w["str_off"], w["str_bytes"].tobytes()
    name = lambda i: sb[so[i]:so[i + 1]].decode()  # noqa: E731
    vs = range(int(w["prob_var_off"][p]), int(w["prob_var_off"][p + 1]))
    own = {name(int(w["var_id"][v])) for v in vs}
    gated = {vs[len(vs) * k // N_OPEN] for k in range(N_OPEN)}
    out = []
    for v in vs:
        cons = []
        for c in range(int(w["var_con_off"][v]), int(w["var_con_off"][v + 1])):
            kind, n = int(w["con_kind"][c]), int(w["con_n"][c])
            args = [name(int(x)) for x in w["con_arg"][w["con_arg_off"][c]:w["con_arg_off"][c + 1]]]
            args = [a for a in args if a in own]
            if kind == 1:
                cons.append(sat.Mandatory())
            elif kind == 2:
                cons.append(sat.Prohibited())
            elif kind == 3:
                cons.append(sat.Dependency(*args))
            elif kind == 4 and args:
                cons.append(sat.Conflict(args[0]))
            elif kind == 5:
                cons.append(sat.AtMost(n, *args))
        if v in gated:
            cons.append(sat.Conflict("env"))
        out.append(Var(name(int(w["var_id"][v])), cons))
    return out


def summary(name, ms):
    x = np.array(ms)
    print("leg (%s): median %.3f ms/call, min %.3f, max %.3f, spread %.3f; repeats %s"
          % (name, np.median(x), x.min(), x.max(), x.max() - x.min(), " ".join("%.3f" % v for v in x)))
    return np.median(x), x.max() - x.min()


def compare(slow, fast, a, b):
    gain, spread = a[0] - b[0], max(a[1], b[1])
    print("(%s) - (%s): %+.3f ms/call (%.2fx); larger spread %.3f ms: %s"
          % (slow, fast, gain, a[0] / b[0], spread,
             "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"))


def timed(legs, n_steps):
    ms = {k: [] for k, _ in legs}
    for _ in range(repeats):
        for name, f in legs:
            for _ in range(warmup):
                f()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                f()
            ms[name].append((time.perf_counter() - t0) * 1e3 / n_steps)
    return ms


w = _lib.generate(2, N_CAT, 1000)
catalogs = [open_catalog(w, b) for b in range(N_CAT)]
ids = [[str(v.Identifier()) for v in c] for c in catalogs]
ctx = _lib.Context(0, 1)
dl = _lib.DeviceLowerer(ctx)
print("build", _lib.build_info())
for n in sizes:
    rng = random.Random(1000)
    queries = []
    for p in range(n):  # "can x or y be installed, without z, in this environment?"
        b = p % N_CAT
        x, y, z = rng.sample(ids[b], 3)
        queries.append((b, [Var("q%da" % p, [sat.Mandatory(), sat.Dependency(x, y)]), Var("q%db" % p, [sat.Conflict(z)]),
                            Var("env", [sat.Mandatory()] if p % 2 else [])]))
    k32, q32, qc = sat.encode_shared(catalogs, queries)
    ref = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dl.lower_solve_shared(k32, q32, qc).items()}
    plain, opened = dl.prepare(k32), dl.prepare(k32, open=True)
    for h in (plain, opened):
        got = h.lower_solve(q32, qc)
        for key in KEYS:
            assert np.array_equal(got[key], ref[key]), key
        assert got["msg"] == ref["msg"] and got["host_lowered"] == ref["host_lowered"]
        print("%s: prepared %d of %d catalogs, deferred per catalog %s; h2d per call %d B (shared call: %d B, the "
              "catalogs' wire: %d B)"
              % ("DP_PREPARE_OPEN" if h is opened else "plain prepare", sum(h.prepared(b) for b in range(h.count)), h.count,
                 " ".join(str(h.deferred(b)) for b in range(h.count)), got["h2d_bytes"], ref["h2d_bytes"], k32.nbytes()))
    print("%d open config-2 catalogs (%d variables, %d constraints on average, %d of them on env), %d queries of three "
          "variables per call, %d timed steps after %d warm-up, %d repeats; %d SAT, %d NotSatisfiable, %d lowered on the host"
          % (N_CAT, np.mean([len(c) for c in catalogs]), np.mean([sum(len(v.Constraints()) for v in c) for c in catalogs]),
             N_OPEN, n, steps, warmup, repeats, int((ref["status"] == 1).sum()), int((ref["status"] == -1).sum()),
             ref["host_lowered"]))
    legs = [("a", lambda: dl.lower_solve_shared(k32, q32, qc)), ("b", lambda: plain.lower_solve(q32, qc)),
            ("c", lambda: opened.lower_solve(q32, qc))]
    ms = timed(legs, steps)
    res = {name: summary("%s, %d queries" % (name, n), ms[name]) for name, _ in legs}
    compare("a", "c", res["a"], res["c"])
    compare("b", "c", res["b"], res["c"])
    plain.close()
    opened.close()
