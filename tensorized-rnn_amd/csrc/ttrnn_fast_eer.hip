// ttrnn_fast_eer.hip — equal error rate of the GE2E similarity matrix on the device (gfx950).
//
// The selection and the phase bodies live in ttrnn_eer.h (shared with the serial host executor of tests/hostemu/hostemu_eer.cpp);
// this file is their device executor, the launches and the C entry points (include/ttrnn.h, TTRNN_HAS_GE2E_EER).
//   k_eer_one    1 workgroup of 1024 threads        route 1: four digit passes and the formula in one launch
//   k_eer_pass   G workgroups of 256 threads        route 2, once per digit: totals of the pass before, selection, this chunk's partial
//   k_eer_last   1 workgroup of 256 threads         route 2: the last digit's totals, selection, the formula
// The counters are LDS integer atomics (ds_add_u32, no return value); across workgroups only plain stores read behind a kernel
// boundary.  Integer counts: the outputs are the same bits whatever the order of threads and workgroups.
#include <hip/hip_runtime.h>
#include "ttrnn.h"
#include "ttrnn_eer.h"

namespace ttrnn {
namespace {

struct EerDevExec {
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
  }
  __device__ __forceinline__ void add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
};

__global__ void __launch_bounds__(TTRNN_EER_THREADS1) k_eer_one(EerPlan p, const float* __restrict__ sim, double* __restrict__ eer,
                                                                float* __restrict__ threshold, int64_t* __restrict__ counts) {
  __shared__ uint32_t lds[TTRNN_EER_LDS_WORDS];
  EerDevExec ex;
  eer_route1_body(ex, p, sim, eer, threshold, counts, lds);
}

__global__ void __launch_bounds__(TTRNN_EER_THREADS2) k_eer_pass(EerPlan p, int pass, const float* __restrict__ sim, uint32_t* ws) {
  __shared__ uint32_t lds[TTRNN_EER_LDS_WORDS];
  EerDevExec ex;
  eer_pass_body(ex, p, pass, (int)blockIdx.x, sim, ws, lds);
}

__global__ void __launch_bounds__(TTRNN_EER_THREADS2) k_eer_last(EerPlan p, uint32_t* ws, double* __restrict__ eer,
                                                                 float* __restrict__ threshold, int64_t* __restrict__ counts) {
  __shared__ uint32_t lds[TTRNN_EER_LDS_WORDS];
  EerDevExec ex;
  eer_last_body(ex, p, ws, eer, threshold, counts, lds);
}

int eer_launched() { return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH; }

// route 1 touches no workspace; the query still answers a non-zero size, as 0 means "refused"
size_t eer_ws_bytes(const EerPlan& p) { return p.route == 2 ? p.total * sizeof(uint32_t) : 64; }

}  // namespace
}  // namespace ttrnn

using namespace ttrnn;

extern "C" size_t ttrnn_ge2e_eer_workspace(const ttrnn_eer_desc* desc) {
  EerPlan p;
  if (eer_plan_init(&p, desc) != TTRNN_OK) return 0;
  return eer_ws_bytes(p);
}

extern "C" int ttrnn_ge2e_eer(const ttrnn_eer_desc* desc, const float* sim, double* eer, float* threshold, int64_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream) {
  EerPlan p;
  if (!desc) return TTRNN_ERR_NULL;
  const int st = eer_plan_init(&p, desc);
  if (st != TTRNN_OK) return st;
  if (!sim || !eer || !workspace) return TTRNN_ERR_NULL;
  if (workspace_bytes < eer_ws_bytes(p)) return TTRNN_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (p.route == 1) {
    hipLaunchKernelGGL(k_eer_one, dim3(1), dim3(TTRNN_EER_THREADS1), 0, s, p, sim, eer, threshold, counts);
    return eer_launched();
  }
  uint32_t* ws = (uint32_t*)workspace;
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(k_eer_pass, dim3(p.G), dim3(TTRNN_EER_THREADS2), 0, s, p, pass, sim, ws);
    if (eer_launched() != TTRNN_OK) return TTRNN_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(k_eer_last, dim3(1), dim3(TTRNN_EER_THREADS2), 0, s, p, ws, eer, threshold, counts);
  return eer_launched();
}
