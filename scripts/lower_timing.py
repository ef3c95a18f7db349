"""Host lowering time: dp_lower_into(NARROW | PACKED | PINNED) on generated
catalogs, one process per run (so two builds can be alternated run by run).
Prints the best of `reps` calls into the same storage, in milliseconds.

usage: python scripts/lower_timing.py [config] [catalogs] [reps] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deppy_amd import _lib  # noqa: E402


def main():
    config, n, reps, seed = (int(a) for a in (sys.argv[1:] + ["2", "10000", "7", "77"][len(sys.argv) - 1:]))
    w = _lib.generate(config, n, seed)
    wire = _lib.WireArrays(**{k: w[k] for k in (
        "prob_var_off", "var_id", "var_con_off", "con_kind", "con_n", "con_arg_off", "con_arg", "str_off")},
        str_bytes=w["str_bytes"].tobytes())
    lw = _lib.Lowered(wire, narrow=True, pinned=True, packed=True)
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        lw.relower(wire)
        best = min(best, time.perf_counter() - t)
    print("%.3f" % (best * 1e3))


if __name__ == "__main__":
    main()
