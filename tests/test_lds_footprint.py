"""The one-wavefront image keeps its CDCL-only arrays out of LDS.

layout.hpp mode_evict: d_mark, l_off and l_lits serve only Solve()'s decisions
and learned rows (dpll(), analyze(), search_solve(), refute()); M_LDS places
them in a per-problem HBM scratch, so the LDS request of a config-2 launch
falls from 16,064 to at most 14,848 bytes (160 KiB / 11 in 512-byte
allocation units): 11 catalogs share a CU instead of 10.  (The four CDCL-only
bitsets, 128-192 bytes, stay in LDS: DESIGN.md 5.6.)

CPU: what the planner requests (dp_plan_footprints).  GPU: batches whose
catalogs do reach Solve() conflicts, refutations and cores -- the paths that
now work in HBM -- bit-exact against the oracle on every field, through every
entry point that has to provide the scratch.
"""
import functools

import numpy as np
import pytest

from deppy_amd import _lib
from oracle import oracle
from tests.gpu_common import compare_results, lowered_config

LDS = _lib.PLACES.index("lds")
LDSG = _lib.PLACES.index("ldsg")
F_CLASS_B, F_SOLVE_UNSAT = 1 << 1, 1 << 2
# 160 KiB / 11, in 512-byte LDS allocation units (what the runtime itself
# reports at these requests: test_occupancy_rises_at_the_new_request)
LDS_11_PER_CU = (160 * 1024 // 11) // 512 * 512


# ---------------------------------------------------------------------------
# CPU: the planner's requests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(10000, 1000), (3000, 7)], ids=["bench", "one-launch"])
def test_config2_fits_eleven_per_cu(n, seed):
    """Config 2 (the bench's batch, and the batch test_plan_order_one_wavefront
    pins to one launch): every catalog on M_LDS, no LDS footprint above
    14,848 bytes (the parent's maximum on the bench's batch: 16,064), and a
    scratch for each."""
    assert LDS_11_PER_CU == 14848
    lw = lowered_config(2, n, seed, narrow=True, packed=True)
    place = _lib.plan_placements(lw.rec_off, lw.rec)
    lds, scratch = _lib.plan_footprints(lw.rec_off, lw.rec)
    print("config 2, %d catalogs, seed %d: lds max %d mean %.0f, scratch max %d mean %.0f"
          % (n, seed, lds.max(), lds.mean(), scratch.max(), scratch.mean()))
    assert (place == LDS).all(), np.bincount(place + 2)
    assert lds.min() > 0 and lds.max() <= LDS_11_PER_CU, lds.max()
    assert (scratch > 0).all()
    order, first = _lib.plan_order(lw.rec_off, lw.rec)
    assert list(first) == [0]  # (one launch, at the largest footprint's request)


def test_ldsg_footprint_unchanged():
    """M_LDSG keeps its whole working set in LDS: the footprints of the first
    three catalogs of config 2, seed 1000, as the parent commit planned them,
    and no scratch."""
    lw = lowered_config(2, 3, 1000, narrow=True, packed=True)
    assert (_lib.plan_placements(lw.rec_off, lw.rec, _lib.OPT_FORCE_LDSG) == LDSG).all()
    lds, scratch = _lib.plan_footprints(lw.rec_off, lw.rec, _lib.OPT_FORCE_LDSG)
    assert lds.tolist() == [14208, 14528, 16448]
    assert scratch.tolist() == [0, 0, 0]
    # the same catalogs on one wavefront: 11,808 / 12,128 / 14,048 bytes of LDS before
    lds1, scratch1 = _lib.plan_footprints(lw.rec_off, lw.rec)
    assert lds1.tolist() == [10544, 10864, 12720]
    assert scratch1.tolist() == [1264, 1264, 1328]
    assert (lds1 + scratch1).tolist() == [11808, 12128, 14048]


def test_capped_build_launches_evict_nothing():
    """Config 3's small catalogs: even with everything in LDS more than 16
    share a CU, so registers bound the launch, it takes the register-capped
    build, and that build keeps the whole working set in LDS (no scratch, the
    parent's footprint and the parent's code)."""
    lw = lowered_config(3, 2000, 12, narrow=True, packed=True)
    assert (_lib.plan_placements(lw.rec_off, lw.rec) == LDS).all()
    lds, scratch = _lib.plan_footprints(lw.rec_off, lw.rec)
    assert (scratch == 0).all(), scratch.max()
    assert lds.min() > 0 and 160 * 1024 // int(lds.max()) > 16, lds.max()


# ---------------------------------------------------------------------------
# GPU: the evicted arrays at work
# ---------------------------------------------------------------------------
def _subset_arrays(rec_off, rec, idx):
    recs = [rec[rec_off[p]:rec_off[p + 1]] for p in idx]
    return (np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64),
            np.concatenate(recs).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _batches():
    """name -> (packed rec_off, rec as the device gets them; int32 rec_off,
    rec; the oracle's results), computed once.  Seeds chosen with the oracle:
    config 2 (first 600 of seed 1000): 19 class-B, 19 SOLVE_UNSAT, 8 UNSAT with
    a core; config 5 (seed 7, the 190 of 400 planned M_LDS): 39, 39, 95;
    config 6 (seed 3): 0, 0, 59 (its UNSAT catalogs fail at the base: analyze()
    and the core's refutations)."""
    out = {}
    for name, config, n, seed in (("c2", 2, 600, 1000), ("c5", 5, 400, 7), ("c6", 6, 300, 3)):
        wide = lowered_config(config, n, seed)
        pk = lowered_config(config, n, seed, narrow=True, packed=True)
        idx = np.nonzero(_lib.plan_placements(pk.rec_off, pk.rec) == LDS)[0]
        a_off, a_rec = _subset_arrays(pk.rec_off, pk.rec, idx)
        w_off, w_rec = _subset_arrays(wide.rec_off, wide.rec, idx)
        assert (_lib.plan_placements(a_off, a_rec) == LDS).all()
        out[name] = (a_off, a_rec, w_off, w_rec, oracle.solve_batch(w_off, w_rec, 0, 16))
    return out


def _counts(o):
    return (int(((o["flags"] & F_CLASS_B) != 0).sum()), int(((o["flags"] & F_SOLVE_UNSAT) != 0).sum()),
            int(((o["status"] == -1) & (o["core_len"] > 0)).sum()))


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0, 1)
    yield c
    c.close()


@pytest.mark.gpu
def test_occupancy_rises_at_the_new_request():
    """What the HIP runtime itself says (hipOccupancyMaxActiveBlocksPerMultiprocessor,
    dp_lds_occupancy) for the unbounded one-wavefront kernel at the parent's
    LDS request for the bench's batch, 16,064 bytes, and at this layout's:
    at least one more catalog per CU."""
    lw = lowered_config(2, 10000, 1000, narrow=True, packed=True)
    lds, _ = _lib.plan_footprints(lw.rec_off, lw.rec)
    new = int(lds.max())
    occ_parent, occ_new = _lib.lds_occupancy(16064), _lib.lds_occupancy(new)
    print("one-wavefront kernel, workgroups per CU: %d at 16064 B, %d at %d B; capped build %d at 8192 B"
          % (occ_parent, occ_new, new, _lib.lds_occupancy(8192, True)))
    assert occ_parent >= 1 and occ_new >= occ_parent + 1, (occ_parent, occ_new)


@pytest.mark.gpu
def test_reference_reaches_the_evicted_paths():
    """The oracle alone says the batches below run Solve() conflicts (class B,
    SOLVE_UNSAT) and refutations (UNSAT with a core): the parity tests cannot
    pass without touching the scratch."""
    B = _batches()
    per = {k: _counts(v[4]) for k, v in B.items()}
    print("class-B, SOLVE_UNSAT, UNSAT with core per batch:", per)
    assert len(B["c2"][0]) - 1 == 600 and len(B["c6"][0]) - 1 == 300 and len(B["c5"][0]) - 1 >= 100
    tot = [sum(p[i] for p in per.values()) for i in range(3)]
    assert tot[0] >= 5 and tot[1] >= 5 and tot[2] >= 20, per
    for k in ("c2", "c5"):  # (config 6 has no Solve() conflict; its cores come from base conflicts)
        assert per[k][0] >= 5 and per[k][1] >= 5, per
    assert all(p[2] >= 5 for p in per.values()), per


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "c5", "c6"])
def test_pipeline_bit_exact(ctx, name):
    a_off, a_rec, _, _, o = _batches()[name]
    g = ctx.submit(a_off, a_rec).wait()
    assert compare_results(g, o, len(a_off) - 1) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "c5", "c6"])
def test_resident_bit_exact_and_repeatable(ctx, name):
    """dp_upload / dp_run: the slice's own scratch; a second run of the same
    resident batch starts from the first run's scratch contents."""
    a_off, a_rec, _, _, o = _batches()[name]
    r = ctx.upload(a_off, a_rec)
    try:
        r.run()
        g1 = r.download()
        r.run()
        g2 = r.download()
    finally:
        r.free()
    n = len(a_off) - 1
    assert compare_results(g1, o, n) == []
    assert compare_results(g2, o, n) == []


@pytest.mark.gpu
def test_latency_path_one_catalog(ctx):
    """dp_solve of one catalog (the latency path has a scratch of its own):
    a class-B one, a SOLVE_UNSAT one and an UNSAT one with a core."""
    a_off, a_rec, _, _, o = _batches()["c5"]
    fl, st = o["flags"], o["status"]
    picks = [int(np.nonzero((fl & F_CLASS_B) != 0)[0][0]), int(np.nonzero((fl & F_SOLVE_UNSAT) != 0)[0][-1]),
             int(np.nonzero((st == -1) & (o["core_len"] > 0))[0][0])]
    for p in picks:
        off, rec = np.array([0, a_off[p + 1] - a_off[p]], np.int64), a_rec[a_off[p]:a_off[p + 1]]
        g = ctx.solve(off, rec)
        assert g["status"][0] == st[p] and g["flags"][0] == fl[p] and g["steps"][0] == o["steps"][p], p
        assert _lib.core_list(g, 0) == _lib.core_list(o, p), p
        nv = int(rec[1])
        assert _lib.installed_list(g, 0, nv) == _lib.installed_list(o, p, nv), p


@pytest.mark.gpu
def test_traced_class_b_catalog(ctx):
    """One small class-B catalog through dp_upload_traced: the results and the
    event stream equal the oracle's."""
    a_off, a_rec, w_off, w_rec, o = _batches()["c2"]
    cb = np.nonzero((o["flags"] & F_CLASS_B) != 0)[0]
    p = int(cb[np.argmin(o["steps"][cb])])
    off, rec = np.array([0, a_off[p + 1] - a_off[p]], np.int64), a_rec[a_off[p]:a_off[p + 1]]
    woff, wrec = np.array([0, w_off[p + 1] - w_off[p]], np.int64), w_rec[w_off[p]:w_off[p + 1]]
    cap = 4096
    ot = oracle.solve_batch(woff, wrec, 0, 1, trace_cap=cap)
    g = ctx.solve(off, rec, cap)
    assert compare_results(g, ot, 1) == []
    assert ot["flags"][0] & F_CLASS_B and g["flags"][0] == ot["flags"][0]
    assert g["trace_len"][0] == ot["trace_len"][0]
    assert np.array_equal(g["trace"][0][:g["trace_len"][0]], ot["trace"][0][:ot["trace_len"][0]])


@pytest.mark.gpu
def test_sixteen_jobs_in_flight_then_a_larger_batch():
    """16 jobs of 64 catalogs in flight at once (every lane's scratch in use),
    then a different, larger batch on the same context: the lanes' scratch
    grows, and a region now holds another catalog's old state."""
    B = _batches()
    a_off, a_rec, _, _, o = B["c5"]
    n = len(a_off) - 1
    jobs_idx = [np.arange(64) + (7 * j) % (n - 64) for j in range(16)]
    c = _lib.Context(0, 1)
    try:
        jobs = [c.submit(*_subset_arrays(a_off, a_rec, idx)) for idx in jobs_idx]
        outs = [j.wait() for j in jobs]
        b_off, b_rec, _, _, ob = B["c2"]
        big = c.submit(b_off, b_rec).wait()
        again = c.submit(a_off, a_rec).wait()
    finally:
        c.close()
    for idx, g in zip(jobs_idx, outs):
        sub = {k: o[k][idx] for k in ("status", "flags", "steps", "core_len")}
        assert np.array_equal(g["status"], sub["status"]) and np.array_equal(g["flags"], sub["flags"])
        assert np.array_equal(g["steps"], sub["steps"]) and np.array_equal(g["core_len"], sub["core_len"])
        for k, p in enumerate(idx):
            assert _lib.core_list(g, k) == _lib.core_list(o, int(p))
            nv = int(a_rec[a_off[p] + 1])
            assert _lib.installed_list(g, k, nv) == _lib.installed_list(o, int(p), nv)
    assert compare_results(big, ob, len(b_off) - 1) == []
    assert compare_results(again, o, n) == []

