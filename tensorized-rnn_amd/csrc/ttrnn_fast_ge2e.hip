// ttrnn_fast_ge2e.hip — GE2E similarity matrix, softmax loss and every gradient of it as four launches (gfx950).
//
// The phase bodies and the plan live in ttrnn_ge2e.h (shared with the serial host executor of tests/hostemu/hostemu_ge2e.cpp);
// this file is their device executor, the launches and the C entry points (include/ttrnn.h, TTRNN_HAS_GE2E).  The operands are
// ~512 x 256 floats: the kernels are latency-bound, fp32 VALU FMAs with fp32 accumulation, and what the call replaces is the
// 50-60 small launches of the tensor-op formulation (ttrnn_hip/ge2e.py) and of autograd's mirror image of them.
//   k_ge2e_centroids  S workgroups                      phase 1
//   k_ge2e_rows       ceil(S U / R) workgroups          phase 2 (dynamic LDS: Ge2ePlan::lds_rows floats, <= 54 KB)
//   k_ge2e_cgrad      1 + K S + S workgroups            phase 3 (workgroup 0: the loss's fixed-order final sum; K S slabs of the
//                                                       centroid gradients; S sums through the exclusive centroids)
//   k_ge2e_dE         S ceil(U / 2) workgroups          phase 4 (the backward call)
// No kernel waits on another workgroup; every cross-workgroup sum is a slab written with plain stores and read behind a kernel
// boundary in an order the plan fixes.
#include <hip/hip_runtime.h>
#include "ttrnn.h"
#include "ttrnn_ge2e.h"

namespace ttrnn {
namespace {

struct Ge2eDevExec {
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
  }
};

extern __shared__ float ge2e_lds[];

__global__ void __launch_bounds__(TTRNN_GE2E_THREADS) k_ge2e_centroids(Ge2ePlan p, const float* __restrict__ src, int Usrc,
                                                                       float* __restrict__ ws) {
  Ge2eDevExec ex;
  ge2e_centroid_body(ex, p, (int)blockIdx.x, src, Usrc, ws, ge2e_lds, TTRNN_GE2E_THREADS);
}

__global__ void __launch_bounds__(TTRNN_GE2E_THREADS) k_ge2e_rows(Ge2ePlan p, const float* __restrict__ E, const float* __restrict__ w,
                                                                  const float* __restrict__ b, float* __restrict__ sim_out,
                                                                  int need_grad, float* ws) {
  Ge2eDevExec ex;
  ge2e_rows_body(ex, p, (int)blockIdx.x, E, w, b, sim_out, need_grad, ws, ge2e_lds, TTRNN_GE2E_THREADS);
}

__global__ void __launch_bounds__(TTRNN_GE2E_THREADS) k_ge2e_cgrad(Ge2ePlan p, const float* __restrict__ E, float* __restrict__ loss,
                                                                   int need_grad, float* ws) {
  Ge2eDevExec ex;
  if (blockIdx.x == 0)
    ge2e_finalize_body(ex, p, loss, need_grad, ws, ge2e_lds, TTRNN_GE2E_THREADS);
  else if ((int)blockIdx.x <= p.K * p.S)
    ge2e_cgrad_body(ex, p, (int)blockIdx.x - 1, E, ws, ge2e_lds, TTRNN_GE2E_THREADS);
  else
    ge2e_asum_body(ex, p, (int)blockIdx.x - 1 - p.K * p.S, E, ws, ge2e_lds);
}

__global__ void __launch_bounds__(TTRNN_GE2E_THREADS) k_ge2e_dE(Ge2ePlan p, const float* __restrict__ E, const float* __restrict__ w,
                                                                const float* __restrict__ g, float* __restrict__ dE,
                                                                float* __restrict__ dw, float* __restrict__ db,
                                                                const float* __restrict__ ws) {
  Ge2eDevExec ex;
  ge2e_dE_body(ex, p, (int)blockIdx.x, E, w, g, dE, dw, db, ws, ge2e_lds);
}

int launched() { return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH; }

}  // namespace
}  // namespace ttrnn

using namespace ttrnn;

extern "C" size_t ttrnn_ge2e_workspace(const ttrnn_ge2e_desc* desc) {
  Ge2ePlan p;
  if (ge2e_plan_init(&p, desc) != TTRNN_OK) return 0;
  return p.total * sizeof(float);
}

extern "C" int ttrnn_ge2e_forward(const ttrnn_ge2e_desc* desc, const float* E, const float* A, const float* w, const float* b,
                                  float* loss, float* sim_out, int need_grad, void* workspace, size_t workspace_bytes, void* stream) {
  Ge2ePlan p;
  if (!desc) return TTRNN_ERR_NULL;
  const int st = ge2e_plan_init(&p, desc);
  if (st != TTRNN_OK) return st;
  if (!E || !w || !b || !workspace || (p.Ue > 0 && !A)) return TTRNN_ERR_NULL;
  if (workspace_bytes < p.total * sizeof(float)) return TTRNN_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const bool train = p.Ue == 0;
  const unsigned T = TTRNN_GE2E_THREADS;
  hipLaunchKernelGGL(k_ge2e_centroids, dim3(p.S), dim3(T), (p.D + T + 17) * sizeof(float), s, p, train ? E : A, train ? p.U : p.Ue,
                     ws);
  if (launched() != TTRNN_OK) return TTRNN_ERR_LAUNCH;
  hipLaunchKernelGGL(k_ge2e_rows, dim3(p.nrow_wg), dim3(T), p.lds_rows * sizeof(float), s, p, E, w, b, sim_out, need_grad ? 1 : 0, ws);
  if (launched() != TTRNN_OK) return TTRNN_ERR_LAUNCH;
  const unsigned grid3 = 1u + (need_grad && train ? (unsigned)(p.K + 1) * p.S : 0u);
  hipLaunchKernelGGL(k_ge2e_cgrad, dim3(grid3), dim3(T), p.lds_cgrad * sizeof(float), s, p, E, loss, need_grad ? 1 : 0, ws);
  return launched();
}

extern "C" int ttrnn_ge2e_backward(const ttrnn_ge2e_desc* desc, const float* E, const float* w, const float* g, float* d_E,
                                   float* d_w, float* d_b, void* workspace, size_t workspace_bytes, void* stream) {
  Ge2ePlan p;
  if (!desc) return TTRNN_ERR_NULL;
  const int st = ge2e_plan_init(&p, desc);
  if (st != TTRNN_OK) return st;
  if (!E || !w || !workspace) return TTRNN_ERR_NULL;
  if (workspace_bytes < p.total * sizeof(float)) return TTRNN_ERR_WORKSPACE;
  if (!d_E && !d_w && !d_b) return TTRNN_OK;
  const unsigned grid = d_E ? (unsigned)p.S * p.UTn : 1u;
  hipLaunchKernelGGL(k_ge2e_dE, dim3(grid), dim3(TTRNN_GE2E_THREADS), p.lds_dE * sizeof(float), (hipStream_t)stream, p, E, w, g, d_E, d_w, d_b,
                     (const float*)workspace);
  return launched();
}
