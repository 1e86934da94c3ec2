// ttrnn_fast_varlen.hip — the one kernel a variable-length training step adds in front of the reverse-time kernels (gfx950).
//
// A variable-length forward (ttrnn_rnn_forward_varlen) leaves FROZEN records in the reserve for the steps t >= len_b of sample b:
// LSTM (i, g, f, o) = (0, 0, 1, 0) with c_t = c_{len-1}, GRU (r, z, n, hn) = (0, 1, 0, 0).  Every reverse kernel's gate gradients
// are products of those stored values (ttrnn_core.h rnn_bwd_body): they come out as exact zeros there, and dc (LSTM) / dh (GRU) pass
// through unchanged.  What an LSTM's frozen steps DROP is dh (it leaves a step only through W^T times the zero gate gradients), so
// the gradient of hT cannot enter at step T - 1: it enters at the sample's own last row.  This kernel builds that d_out:
//   d_out_seeded[b][t] = (t < len_b ? d_out[b][t] : 0) + (t == len_b - 1 ? d_hT[b] : 0)
// in storage dtype (the sum is formed in fp32 and rounded once); either input may be NULL (zeros).  d_cT needs nothing: it flows
// through f = 1.  The GRU takes the same seed (with d_hT = NULL afterwards) so that there is one rule for both cells.
// The reference has no counterpart: its callers run one utterance per call (experiments/speaker_verification/encoder/inference.py).
#include <hip/hip_runtime.h>
#include "ttrnn.h"
#include "ttrnn_core.h"
#include "ttrnn_launch.h"

namespace ttrnn {
namespace {

// one thread per element of [B][T][H]; the row's length is read once per thread (L1 / L2 hit: B ints)
template <typename TS>
__global__ void __launch_bounds__(256) k_varlen_seed_dout(long n, int T, int H, const int* __restrict__ lens,
                                                          const TS* __restrict__ d_out, const TS* __restrict__ d_hT,
                                                          TS* __restrict__ seeded) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long row = e / H;
  const int j = (int)(e - row * H);
  const long b = row / T;
  const int t = (int)(row - b * T);
  const int len = varlen_clamp(lens[b], T);
  float v = 0.f;
  if (d_out && t < len) v = ld(d_out, (size_t)e);
  if (d_hT && t == len - 1) v += ld(d_hT, (size_t)b * H + j);
  st(seeded, (size_t)e, v);
}

}  // namespace

int launch_varlen_seed_dout(int dtype, int B, int T, int H, const int* lens, const void* d_out, const void* d_hT, void* d_out_seeded,
                            hipStream_t stream) {
  const long n = (long)B * T * H;
  if (n == 0) return TTRNN_OK;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (dtype == TTRNN_F32)
    hipLaunchKernelGGL(k_varlen_seed_dout<float>, dim3(grid), dim3(256), 0, stream, n, T, H, lens, (const float*)d_out,
                       (const float*)d_hT, (float*)d_out_seeded);
  else
    hipLaunchKernelGGL(k_varlen_seed_dout<bf16_t>, dim3(grid), dim3(256), 0, stream, n, T, H, lens, (const bf16_t*)d_out,
                       (const bf16_t*)d_hT, (bf16_t*)d_out_seeded);
  return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH;
}

}  // namespace ttrnn
