"""The served path from the compact wire, unfused against fused
(dp_lower_solve), legs alternated in one process:

  (a) dl.lower + ctx.submit, two batches in flight (bench.py end_to_end_device's loop)
  (b) two threads, each calling lower_solve on a DeviceLowerer of its own
  (c) sat.solve_wire(w32), one batch at a time
  (d) sat.solve_wire_fused(w32), one batch at a time

usage: fused_timing.py CONFIG N STEPS [WARMUP [REPEATS]]
The dp_solved arrays of (b) and (d) are checked against (a)'s results at the
timed size before anything is timed.  Prints resolutions/s per repeat, the
median and min-max spread per leg, and the fused call's PCIe bytes per
catalog.  Run on the GPU box."""
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deppy_amd import _lib, sat  # noqa: E402

cfg, n, steps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 5
repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 5
KEYS = ("status", "flags", "steps", "core_len", "inst_off", "core_off")

w = _lib.generate(cfg, n, 1000)
wa = _lib.WireArrays(**{k: w[k] for k in ("prob_var_off", "var_id", "var_con_off", "con_kind", "con_n", "con_arg_off",
                                          "con_arg", "str_off")}, str_bytes=w["str_bytes"].tobytes())
w32 = _lib.Wire32Arrays(wa)
ctx = _lib.Context(0, 1)
dl = _lib.DeviceLowerer(ctx)
dls = [_lib.DeviceLowerer(ctx) for _ in range(2)]
depth = 2
lws = [dl.lower(w32, _lib.Lowered.empty()) for _ in range(depth)]
outs = [_lib.result_arrays(x.rec_off, x.rec) for x in lws]


def leg_a(k):
    jobs = []
    for i in range(k):
        j = i % depth
        if len(jobs) == depth:
            jobs.pop(0).wait()
        dl.lower(w32, lws[j])
        jobs.append(ctx.submit(lws[j].rec_off, lws[j].rec, outs[j]))
    for job in jobs:
        job.wait()


def leg_b(k):
    def work(d, m):
        for _ in range(m):
            d.lower_solve(w32)
    ts = [threading.Thread(target=work, args=(dls[i], k // 2 + (i < k % 2))) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()


def leg_c(k):
    for _ in range(k):
        sat.solve_wire(w32, ctx)


def leg_d(k):
    for _ in range(k):
        sat.solve_wire_fused(w32, ctx)


def check(name, got, ref, lw):
    for key in KEYS:
        assert np.array_equal(got[key], ref[key]), (name, key)
    assert np.array_equal(got["installed"], ref["installed"][:int(ref["inst_off"][-1])]), (name, "installed")
    assert np.array_equal(got["core"], ref["core"][:int(ref["core_off"][-1])]), (name, "core")
    for p in np.flatnonzero(ref["core_len"] > 0):
        c0, m, i0 = int(ref["core_off"][p]), int(ref["core_len"][p]), int(lw.ident_off[p])
        ids = ref["core"][c0:c0 + m]
        assert np.array_equal(got["core_var"][c0:c0 + m], lw.ident_var[i0 + ids]), (name, "core_var", p)
        assert np.array_equal(got["core_con"][c0:c0 + m], lw.ident_con[i0 + ids]), (name, "core_con", p)


leg_a(depth)
ref = {k: v[:n] if k in ("status", "flags", "core_len", "steps") else v for k, v in outs[0].items()}
for i, d in enumerate(dls):
    check("b%d" % i, d.lower_solve(w32), ref, lws[0])
fused = sat.solve_wire_fused(w32, ctx)[1]
check("d", fused, ref, lws[0])
print("build", _lib.build_info())
print("config %d, %d catalogs, %d timed steps after %d warm-up, %d repeats; fused results equal the unfused leg's"
      % (cfg, n, steps, warmup, repeats))
print("wire bytes per catalog %.1f; fused call: h2d %.1f B, d2h %.1f B per catalog, %d lowered on the host"
      % (w32.nbytes() / n, fused["h2d_bytes"] / n, fused["d2h_bytes"] / n, fused["host_lowered"]))
ctx.stats(reset=True)
leg_a(2)
st = ctx.stats(reset=True)
print("unfused (a): pipeline h2d %.1f B per catalog beside the wire's %.1f and the records' and owners' copy back"
      % (st["h2d_bytes"] / (2 * n), w32.nbytes() / n))

legs = (("a", leg_a), ("b", leg_b), ("c", leg_c), ("d", leg_d))
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
for fu, un in (("b", "a"), ("d", "c")):
    f, u = np.array(rates[fu]), np.array(rates[un])
    gain = np.median(f) - np.median(u)
    print("(%s) - (%s): %+.3fM res/s (%.2fx); unfused spread %.3fM: %s"
          % (fu, un, gain / 1e6, np.median(f) / np.median(u), (u.max() - u.min()) / 1e6,
             "faster beyond the spread" if gain > u.max() - u.min() else "NOT faster beyond the spread"))
print("VERDICT's target for end_to_end_device: 7M res/s (a target, not a gate)")
