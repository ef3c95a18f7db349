"""Many queries over a few catalogs, the catalogs sent per query against sent
once (dp_lower_solve_shared), legs alternated in one process:

  (a) lower_solve on the expanded compact wire: every problem carries its
      catalog's variables, what a caller has to send without sharing
  (b) lower_solve_shared: the catalogs' wire once per call, per query its own
      variables and a catalog number

usage: shared_timing.py [CATALOGS [QUERIES [STEPS [WARMUP [REPEATS]]]]]
(defaults: 16 config-2 catalogs, 10000 two-variable queries, 20 timed steps
after 5 warm-up steps, 5 repeats).  (b)'s results are checked against (a)'s
first run before anything is timed.  Prints resolutions/s per repeat, the
median and min-max spread per leg and the PCIe bytes per query; with
DEPPY_DL_TIMES=1 each call's phases go to stderr.  Run on the GPU box."""
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deppy_amd import _lib, sat  # noqa: E402

argv = [int(x) for x in sys.argv[1:]] + [None] * 5
n_cat, n, steps, warmup, repeats = (a if a is not None else d for a, d in zip(argv, (16, 10000, 20, 5, 5)))
KEYS = ("status", "flags", "steps", "core_len", "inst_off", "core_off", "installed", "core", "core_var", "core_con", "err")


class Var(sat.Variable):
    def __init__(self, ident, cons):
        self.ident, self.cons = sat.Identifier(ident), cons

    def Identifier(self):
        return self.ident

    def Constraints(self):
        return self.cons


def catalog_variables(w, p):
    """Problem p of a generated wire as Variables."""
    so, sb = w["str_off"], w["str_bytes"].tobytes()
    name = lambda i: sb[so[i]:so[i + 1]].decode()  # noqa: E731
    make = {1: lambda n, a: sat.Mandatory(), 2: lambda n, a: sat.Prohibited(), 3: lambda n, a: sat.Dependency(*a),
            4: lambda n, a: sat.Conflict(a[0]), 5: lambda n, a: sat.AtMost(n, *a)}
    out = []
    for v in range(int(w["prob_var_off"][p]), int(w["prob_var_off"][p + 1])):
        cons = []
        for c in range(int(w["var_con_off"][v]), int(w["var_con_off"][v + 1])):
            args = [name(int(x)) for x in w["con_arg"][w["con_arg_off"][c]:w["con_arg_off"][c + 1]]]
            cons.append(make[int(w["con_kind"][c])](int(w["con_n"][c]), args))
        out.append(Var(name(int(w["var_id"][v])), cons))
    return out


w = _lib.generate(2, n_cat, 1000)
catalogs = [catalog_variables(w, b) for b in range(n_cat)]
ids = [[str(v.Identifier()) for v in c] for c in catalogs]
rng = random.Random(1000)
queries = []
for p in range(n):  # "can x or y be installed, without z?"
    b = p % n_cat
    x, y, z = rng.sample(ids[b], 3)
    queries.append((b, [Var("q%da" % p, [sat.Mandatory(), sat.Dependency(x, y)]), Var("q%db" % p, [sat.Conflict(z)])]))
k32, q32, qc = sat.encode_shared(catalogs, queries)
e32 = _lib.Wire32Arrays(_lib.expand_shared(k32, q32, qc))
ctx = _lib.Context(0, 1)
dl = _lib.DeviceLowerer(ctx)


def leg_a(k):
    for _ in range(k):
        dl.lower_solve(e32)


def leg_b(k):
    for _ in range(k):
        dl.lower_solve_shared(k32, q32, qc)


ref = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dl.lower_solve(e32).items()}
got = dl.lower_solve_shared(k32, q32, qc)
for key in KEYS:
    assert np.array_equal(got[key], ref[key]), key
assert got["msg"] == ref["msg"] and got["host_lowered"] == ref["host_lowered"]
print("build", _lib.build_info())
print("%d config-2 catalogs, %d queries of two variables, %d timed steps after %d warm-up, %d repeats; the shared "
      "call's results equal the expanded wire's (%d SAT, %d NotSatisfiable, %d lowered on the host)"
      % (n_cat, n, steps, warmup, repeats, int((ref["status"] == 1).sum()), int((ref["status"] == -1).sum()),
         ref["host_lowered"]))
print("per query: expanded wire %.1f B, queries' wire %.1f B (+ the catalogs' %d B per call); "
      "h2d (a) %.1f B, (b) %.1f B; d2h (a) %.1f B, (b) %.1f B"
      % (e32.nbytes() / n, q32.nbytes() / n, k32.nbytes(), ref["h2d_bytes"] / n, got["h2d_bytes"] / n,
         ref["d2h_bytes"] / n, got["d2h_bytes"] / n))

legs = (("a", leg_a), ("b", leg_b))
rates = {k: [] for k, _ in legs}
for r in range(repeats):
    for name, f in legs:
        f(warmup)
        t0 = time.perf_counter()
        f(steps)
        rates[name].append(n * steps / (time.perf_counter() - t0))
for name, _ in legs:
    x = np.array(rates[name])
    print("leg (%s): median %.3fM res/s, min %.3fM, max %.3fM, spread %.3fM; repeats %s"
          % (name, np.median(x) / 1e6, x.min() / 1e6, x.max() / 1e6, (x.max() - x.min()) / 1e6,
             " ".join("%.3f" % (v / 1e6) for v in x)))
a, b = np.array(rates["a"]), np.array(rates["b"])
gain = np.median(b) - np.median(a)
spread = max(a.max() - a.min(), b.max() - b.min())
print("(b) - (a): %+.3fM res/s (%.2fx); larger spread %.3fM: %s"
      % (gain / 1e6, np.median(b) / np.median(a), spread / 1e6,
         "faster by more than three times the spread" if gain > 3 * spread
         else "NOT faster by more than three times the spread"))
