// Hand-over between the device lowering (lower_device.hip) and the host
// lowering's result type (lower.cpp dp_lowered) and context (runtime.cpp).
#pragma once
#include <cstdint>

#include "../../include/deppy_hip.h"

namespace dp {

struct LoweredOut {
  int64_t *rec_off, *ident_off;
  int32_t *rec, *ivar, *icon;
};
// lw sized for P problems, rec_words record words and n_ident identities
// (page-locked when asked), every problem without an error.
LoweredOut lowered_prepare(dp_lowered* lw, int32_t P, int64_t rec_words, int64_t n_ident, bool pinned);
// Problems `which` lowered on the host from `sub` and spliced into lw.
int lowered_splice(dp_lowered* lw, const dp_wire* sub, int32_t flags, const int32_t* which, int32_t nw);
// The HIP ordinal of the context's first device (runtime.cpp).
int ctx_first_ordinal(const dp_ctx* ctx);
// The context's dp_opt_flag bits.
int32_t ctx_flags(const dp_ctx* ctx);

// A fused job's records (dp_lower_solve): left in device memory by the
// lowering, with only their headers on the host.  Problem i's record is at
// dev_rec + rec_off[i], its header at heads + i * DP_H_SIZE (all zero: no
// record, the problem is not launched), its identity owners at dev_ivs /
// dev_ics + i * owner_stride (dev_nid[i] of them).
struct FusedSrc {
  const int32_t* heads;    // host
  const int64_t* rec_off;  // host [n+1]
  const int32_t* dev_rec;  // device (of the context's first device)
  const int32_t *dev_nid, *dev_ivs, *dev_ics;
  int32_t owner_stride;
  int32_t *core_var, *core_con;  // host: owners of res->core, indexed as it is
  // A traced job (dp_lower_solve_traced): problem i's search trace goes to
  // dev_trace + i * trace_cap and its length to dev_trace_len[i], both device
  // memory.  Untraced: null, null and 0.
  int32_t* dev_trace;
  int32_t* dev_trace_len;
  int32_t trace_cap;
};
// dp_submit with byte accounting: *h2d / *d2h (may be null) grow by every
// byte the job's chunks move over PCIe (kernel writes to and reads from
// mapped host memory included) before dp_job_wait returns.  With `fused`,
// the job is one chunk on the context's first device whose solve reads the
// records where they lie; only its tables go to the device, and the owners
// of the reported cores come back beside them.
int submit_job(dp_ctx* ctx, const dp_batch* b, dp_result* res, const FusedSrc* fused, int64_t* h2d, int64_t* d2h,
               dp_job** out);


}  // namespace dp
