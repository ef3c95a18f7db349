"""Host side of the fused lowering and solve (dp_lower_solve): the entry
point refuses NULL without touching a device, and the launch plan made from
the records' headers alone (dp_plan_order_heads, what the fused path plans
from: the records stay in device memory) is the plan made from the full
records (dp_plan_order)."""
import ctypes

import numpy as np
import pytest

from deppy_amd import _lib
from tests.gpu_common import lowered_config


def test_lower_solve_refuses_null():
    L = _lib.lib()
    so = _lib.Solved()
    w32 = _lib.Wire32Arrays(_lib.WireArrays(**_wire(2, 3, 1)), pinned=False)
    ws = w32.struct()
    assert L.dp_lower_solve(None, ctypes.byref(ws), ctypes.byref(so)) == -1
    assert b"dp_lower_solve" in L.dp_last_global_error() and b"null" in L.dp_last_global_error()
    assert L.dp_lower_solve(None, None, None) == -1
    m = ctypes.c_char_p()
    assert L.dp_dlower_error(None, 0, ctypes.byref(m)) == 0 and m.value == b""


def _wire(config, n, seed):
    w = _lib.generate(config, n, seed)
    d = {k: w[k] for k in ("prob_var_off", "var_id", "var_con_off", "con_kind", "con_n", "con_arg_off", "con_arg",
                           "str_off")}
    d["str_bytes"] = w["str_bytes"].tobytes()
    return d


def _mixed():
    """Configs 2, 3, 5 and 6 interleaved in one batch (one-wavefront and
    multi-wave placements, several LDS buckets), as packed records."""
    parts = [lowered_config(c, n, 40 + c, packed=True) for c, n in ((2, 120), (3, 200), (5, 60), (6, 90))]
    recs = []
    for k in range(max(p.n for p in parts)):
        recs += [p.record(k) for p in parts if k < p.n]
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return rec_off, np.concatenate(recs).astype(np.int32)


BATCHES = [(2, 300), (3, 300), (5, 300), (6, 300), "mixed"]


@pytest.mark.parametrize("flags", [0, _lib.OPT_FORCE_LDSG])
@pytest.mark.parametrize("batch", BATCHES, ids=str)
def test_plan_from_headers_equals_plan_from_records(batch, flags):
    if batch == "mixed":
        rec_off, rec = _mixed()
    else:
        lw = lowered_config(batch[0], batch[1], 7, packed=True)
        rec_off, rec = lw.rec_off, lw.rec
    heads = np.stack([rec[o:o + 16] for o in rec_off[:-1]])
    order, first = _lib.plan_order(rec_off, rec, flags)
    order_h, first_h = _lib.plan_order_heads(heads, rec_off, flags)
    np.testing.assert_array_equal(first_h, first)
    np.testing.assert_array_equal(order_h, order)
    assert len(first) >= 1
