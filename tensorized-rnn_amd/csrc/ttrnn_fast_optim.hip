// ttrnn_fast_optim.hip — gradient scaling, global-norm clipping and the Adam step as one library call (gfx950).
//
// The chunking, the fixed-order sums and the phase bodies live in ttrnn_optim.h (shared with the serial host executor of
// tests/hostemu/hostemu_optim.cpp); this file is their device executor, the launches and the C entry points (include/ttrnn.h,
// TTRNN_HAS_OPTIM).
//   k_optim_one   1 workgroup of 1024 threads   route 1, a table of one argument group: counter, partials, total, update
//   k_optim_a     W workgroups                  per argument group: the chunks' partial sums of squares (+ the counter and the
//                                               step's scalars in workgroup 0 of the first group)
//   k_optim_b     W workgroups                  per argument group: the total of all partials (every workgroup, the same sum),
//                                               the clip coefficient, the update of the workgroup's chunks
// k_optim_a / k_optim_b run with 256 threads on route 2 and as one workgroup of 1024 on route 1 with a longer table.
// Across workgroups only plain stores read behind a kernel boundary; no atomics.
#include <hip/hip_runtime.h>
#include "ttrnn.h"
#include "ttrnn_optim.h"

namespace ttrnn {
namespace {

struct OptimDevExec {
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
  }
};

__global__ void __launch_bounds__(TTRNN_OPTIM_THREADS1) k_optim_one(OptimPlan p, OptimGroup gr, float* m, float* v, int64_t* step,
                                                                    const float* lr, float* total_norm, float* ws) {
  __shared__ OptimLds lds;
  OptimDevExec ex;
  optim_route1_body(ex, p, gr, m, v, step, lr, total_norm, ws, &lds);
}

__global__ void __launch_bounds__(TTRNN_OPTIM_THREADS1) k_optim_a(OptimPlan p, OptimGroup gr, int64_t* step, const float* lr, float* ws) {
  __shared__ OptimLds lds;
  OptimDevExec ex;
  optim_a_body(ex, p, gr, (int)blockIdx.x, (int)gridDim.x, step, lr, ws, &lds);
}

__global__ void __launch_bounds__(TTRNN_OPTIM_THREADS1) k_optim_b(OptimPlan p, OptimGroup gr, float* m, float* v, float* total_norm,
                                                                  const float* ws) {
  __shared__ OptimLds lds;
  OptimDevExec ex;
  optim_b_body(ex, p, gr, (int)blockIdx.x, (int)gridDim.x, m, v, total_norm, ws, &lds);
}

int optim_launched() { return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH; }

}  // namespace
}  // namespace ttrnn

using namespace ttrnn;

extern "C" int64_t ttrnn_optim_state_elems(const ttrnn_optim_desc* desc, const int64_t* numel) {
  OptimPlan p;
  if (optim_plan_init(&p, desc, numel, 0) != TTRNN_OK) return 0;
  return optim_state_elems(p);
}

extern "C" size_t ttrnn_optim_workspace(const ttrnn_optim_desc* desc, const int64_t* numel) {
  OptimPlan p;
  if (optim_plan_init(&p, desc, numel, 0) != TTRNN_OK) return 0;
  return optim_ws_bytes(p);
}

extern "C" int ttrnn_optim_step(const ttrnn_optim_desc* desc, const int64_t* numel, void* const* params, void* const* grads,
                                const float* grad_scale, float* m, float* v, int64_t* step, const float* lr, float* total_norm,
                                void* workspace, size_t workspace_bytes, void* stream) {
  OptimPlan p;
  if (!desc || !numel) return TTRNN_ERR_NULL;
  const int st = optim_plan_init(&p, desc, numel, total_norm != nullptr);
  if (st != TTRNN_OK) return st;
  const bool adam = p.mode == TTRNN_OPTIM_ADAM;
  if (!grads || !workspace) return TTRNN_ERR_NULL;
  if (adam && (!params || !m || !v || !step || !lr)) return TTRNN_ERR_NULL;
  for (int i = 0; i < p.n; ++i)
    if (!grads[i] || (adam && !params[i])) return TTRNN_ERR_NULL;
  if (workspace_bytes < optim_ws_bytes(p)) return TTRNN_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  OptimGroup gr;
  if (p.route == 1 && p.groups == 1) {
    optim_group_init(&gr, p, 0, numel, adam ? params : nullptr, grads, grad_scale);
    hipLaunchKernelGGL(k_optim_one, dim3(1), dim3(TTRNN_OPTIM_THREADS1), 0, s, p, gr, m, v, step, lr, total_norm, ws);
    return optim_launched();
  }
  const int threads = p.route == 1 ? TTRNN_OPTIM_THREADS1 : TTRNN_OPTIM_THREADS2;
  // all first launches before the first second one: the norm spans every group.  Without a norm to form, one workgroup of the
  // first group's launch advances the counter and the others have nothing to do.
  const int a_launches = p.need_norm ? p.groups : (adam ? 1 : 0);
  for (int k = 0; k < a_launches; ++k) {
    optim_group_init(&gr, p, k, numel, adam ? params : nullptr, grads, grad_scale);
    hipLaunchKernelGGL(k_optim_a, dim3(p.need_norm ? optim_group_wg(p, gr) : 1), dim3(threads), 0, s, p, gr, step, lr, ws);
    if (optim_launched() != TTRNN_OK) return TTRNN_ERR_LAUNCH;
  }
  for (int k = 0; k < p.groups; ++k) {
    optim_group_init(&gr, p, k, numel, adam ? params : nullptr, grads, grad_scale);
    hipLaunchKernelGGL(k_optim_b, dim3(optim_group_wg(p, gr)), dim3(threads), 0, s, p, gr, m, v, total_norm, ws);
    if (optim_launched() != TTRNN_OK) return TTRNN_ERR_LAUNCH;
  }
  return TTRNN_OK;
}
