// Search traces of the fused path (dp_lower_solve_traced), packed and given
// their owners on the device.
//
// The solve kernels write each problem's trace (WithTracer, solve.go:141-146;
// Tracer.Trace, search.go:173) into its trace_cap-word region of the window's
// device buffer.  After the window's job, the host knows every trace_len,
// prefix-sums them, and this kernel writes the words that were written --
// not P * trace_cap -- densely into page-locked host memory through its
// device mapping, with each identity word's AppliedConstraint beside it
// (trace_walk.hpp), read from the owner arrays the lowering left in device
// memory (lower_device.hip ivs / ics).
//
// One wavefront per problem.  The region is device memory kernels of an
// earlier launch wrote, and is trusted no more than core_owners.hip trusts
// the cores: the length is clamped to the region and to the output range the
// host laid out, and the walk checks every count against it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/deppy_hip.h"
#include "kernel_api.hpp"
#include "trace_walk.hpp"

namespace {

constexpr int TP_T = 64;

__global__ void __launch_bounds__(TP_T) trace_pack_kernel(int32_t n, const int32_t* __restrict__ region,
                                                          const int32_t* __restrict__ trace_len, int32_t trace_cap,
                                                          const int64_t* __restrict__ trace_off,
                                                          const int32_t* __restrict__ nid,
                                                          const int32_t* __restrict__ ivs,
                                                          const int32_t* __restrict__ ics, int32_t stride,
                                                          int64_t out_words, int32_t* __restrict__ out,
                                                          int32_t* __restrict__ out_var,
                                                          int32_t* __restrict__ out_con) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (p >= n) return;
  const int64_t o0 = trace_off[p], o1 = trace_off[p + 1];
  if (o0 < 0 || o1 < o0 || o1 > out_words) return;
  const int32_t len = (int32_t)min((int64_t)max(min(trace_len[p], trace_cap), 0), o1 - o0);
  const int32_t* t = region + (int64_t)p * trace_cap;
  for (int i = lane; i < len; i += TP_T) out[o0 + i] = t[i];
  dp::trace_owners_walk(t, len, max(min(nid[p], stride), 0), ivs + (int64_t)p * stride, ics + (int64_t)p * stride,
                        out_var + o0, out_con + o0, lane, TP_T);
}

}  // namespace

namespace dp {

hipError_t launch_trace_pack(int32_t n, const int32_t* region, const int32_t* trace_len, int32_t trace_cap,
                             const int64_t* trace_off, const int32_t* nid, const int32_t* ivs, const int32_t* ics,
                             int32_t stride, int64_t out_words, int32_t* out, int32_t* out_var, int32_t* out_con,
                             hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(trace_pack_kernel, dim3((unsigned)n), dim3(TP_T), 0, stream, n, region, trace_len, trace_cap,
                     trace_off, nid, ivs, ics, stride, out_words, out, out_var, out_con);
  return hipGetLastError();
}

}  // namespace dp

extern "C" int dp_trace_owners_host(const int32_t* trace, int32_t len, int32_t nid, const int32_t* ivs,
                                    const int32_t* ics, int32_t* out_var, int32_t* out_con) {
  if (len < 0 || nid < 0 || (len > 0 && (!trace || !out_var || !out_con)) || (nid > 0 && (!ivs || !ics))) return -1;
  dp::trace_owners_walk(trace, len, nid, ivs, ics, out_var, out_con, 0, 1);
  return 0;
}
