// The owners of a search trace's identity words (trace_owners.hip on the
// device, dp_trace_owners_host on the host: the same walk).
//
// A trace is a run of event records [n, n variable indices, m, m identities]
// (include/deppy_hip.h dp_upload_traced; Tracer.Trace, search.go:173).  What a
// caller is shown of an identity is its AppliedConstraint, the pair (variable,
// index in its Constraints()) the lowering kept per identity
// (lit_mapping.go:69-72).  The walk writes that pair beside every identity
// word and -1 beside every other word.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DP_TW_HD __host__ __device__
#else
#define DP_TW_HD
#endif

namespace dp {

// Words [0, len) of t, lane `lane` of `nlanes` (1 lane: the whole of it).  The
// event headers are read by every lane alike, so the walk is uniform; each
// lane writes the words lane, lane + nlanes, ... of every range, and every
// word of out_var / out_con [0, len) is written exactly once.  An identity
// outside [0, nid) has the owner -1.  A negative count or an event that runs
// past len ends the walk: the words from that event on have no owner.
// Nothing outside t[0, len), ivs / ics[0, nid) and out[0, len) is touched.
DP_TW_HD inline void trace_owners_walk(const int32_t* t, int32_t len, int32_t nid, const int32_t* ivs,
                                       const int32_t* ics, int32_t* out_var, int32_t* out_con, int lane,
                                       int nlanes) {
  int64_t pos = 0;
  while (pos < len) {
    const int64_t n = t[pos];
    if (n < 0 || pos + 1 + n >= len) break;
    const int64_t m = t[pos + 1 + n];
    const int64_t ids = pos + 2 + n;
    if (m < 0 || ids + m > len) break;
    for (int64_t i = pos + lane; i < ids; i += nlanes) out_var[i] = out_con[i] = -1;
    for (int64_t i = ids + lane; i < ids + m; i += nlanes) {
      const int32_t id = t[i];
      const bool ok = id >= 0 && id < nid;
      out_var[i] = ok ? ivs[id] : -1;
      out_con[i] = ok ? ics[id] : -1;
    }
    pos = ids + m;
  }
  for (int64_t i = pos + lane; i < len; i += nlanes) out_var[i] = out_con[i] = -1;
}

}  // namespace dp
