// Owners of the reported cores, on the device (dp_lower_solve).
//
// A NotSatisfiable explanation is a list of identities; what the caller is
// told is each identity's AppliedConstraint (pkg/sat/lit_mapping.go:69-72),
// the pair (variable, index in its Constraints()) the lowering kept per
// identity.  The fused path leaves those pairs in device memory
// (lower_device.hip ivs / ics, DL_C per problem), so the mapping runs here,
// after the chunk's solve launches on their stream, and only the pairs of
// the cores that were reported cross PCIe -- not every identity's.
//
// Sixteen lanes per work item (most problems report no core, and a core is a
// handful of identities): a 256-thread workgroup covers 16 items.  Every
// index is checked: the results and the core pool are read back from where
// the solve wrote them (mapped host memory), and an identity outside
// [0, nid) yields -1, never a read out of bounds.
#include <hip/hip_runtime.h>

#include "kernel_api.hpp"

namespace {

constexpr int CO_T = 256;   // threads per workgroup
constexpr int CO_SUB = 16;  // lanes per work item

__global__ void __launch_bounds__(CO_T) core_owners_kernel(const dp::WorkItem* __restrict__ items, int n_items,
                                                          const dp::ProblemOut* __restrict__ out,
                                                          const int32_t* __restrict__ core, int64_t core_cap,
                                                          int32_t* __restrict__ own_var, int32_t* __restrict__ own_con,
                                                          const int32_t* __restrict__ nid,
                                                          const int32_t* __restrict__ ivs,
                                                          const int32_t* __restrict__ ics, int32_t stride) {
  const int t = (int)blockIdx.x * CO_T + (int)threadIdx.x;
  const int w = t / CO_SUB, sub = t % CO_SUB;
  if (w >= n_items) return;
  const int pid = items[w].pid;
  const int len = out[pid].core_len, at = out[pid].core_at;
  if (len <= 0 || at < 0 || (int64_t)at + len > core_cap) return;
  const int n = min(nid[pid], stride);
  const int64_t base = (int64_t)pid * stride;
  for (int k = sub; k < len; k += CO_SUB) {
    const int id = core[at + k];
    const bool ok = id >= 0 && id < n;
    own_var[at + k] = ok ? ivs[base + id] : -1;
    own_con[at + k] = ok ? ics[base + id] : -1;
  }
}

}  // namespace

namespace dp {

hipError_t launch_core_owners(const WorkItem* items, int n_items, const ProblemOut* out, const int32_t* core,
                              int64_t core_cap, int32_t* own_var, int32_t* own_con, const int32_t* nid,
                              const int32_t* ivs, const int32_t* ics, int32_t stride, hipStream_t stream) {
  if (n_items <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)(((int64_t)n_items * CO_SUB + CO_T - 1) / CO_T);
  hipLaunchKernelGGL(core_owners_kernel, dim3(blocks), dim3(CO_T), 0, stream, items, n_items, out, core, core_cap,
                     own_var, own_con, nid, ivs, ics, stride);
  return hipGetLastError();
}

}  // namespace dp
