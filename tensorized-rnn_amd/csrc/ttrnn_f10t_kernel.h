// ttrnn_f10t_kernel.h — k_lstm_fwd_f10t (the fused-core TT-LSTM forward with cores 0·1 contracted first) and its launcher, for the
// two translation units that instantiate it: ttrnn_fast_f10t.hip (ADJ = true, the default loop; built with -fno-slp-vectorize) and
// ttrnn_fast_f10t_r7.hip (ADJ = false, round 7's loop behind option f10t_r7_loop; built with the plain flags, so that its code is
// the code it was measured with).  Description, layouts, instruction counts and resources: ttrnn_fast_f10t.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "ttrnn_core.h"
#include "ttrnn_launch.h"
#include "ttrnn_opts.h"
#include "ttrnn_mfma.h"
#include "ttrnn_split.h"
#include "ttrnn_f10.h"
#include "ttrnn_f10_dev.h"

namespace ttrnn {

// fp16 pieces of 2^4 h as stage 1's A operand + four floats for f10h_h0_expo.  ADJ: [parity][row = 2 j2 + piece] rows of F10T_ROW = 48 halves
// (32 used), the four 16-byte chunks of a row XORed with row >> 2; round 7's loop: [parity][piece][j2][k = 32]
template <bool ADJ>
static constexpr size_t F10T_LDS_BYTES = 2 * (ADJ ? 16 * F10T_ROW : 2 * 8 * 32) * sizeof(_Float16) + 64;

// H0 / OUT / IN1 / DIAG: as k_lstm_fwd_f10q.  ADJ: a unit's two pieces on adjacent rows of stage 1's A operand, fold in the lane
// (round 8); false = round 7's loop (pieces eight rows apart, fold across the wave's halves), option f10t_r7_loop
template <class S, bool H0, bool OUT, bool IN1, bool ADJ, bool DIAG = false>
__global__ void __launch_bounds__(256, 2) k_lstm_fwd_f10t(int B, int T, GinSrc gs, const float* __restrict__ h0,
                                                          const float* __restrict__ c0, const float* __restrict__ packed_hid,
                                                          const float* __restrict__ hdr,
                                                          const float* __restrict__ bias_hid, float* __restrict__ out,
                                                          float* __restrict__ hT, float* __restrict__ cT,
                                                          float* __restrict__ reserve) {
  static_assert(f10_ok<S>(), "shape not supported by the fused-core kernel");
  using F = F10<S>;
  static_assert(F::MT == 4 && F::ROWS2 == 32 && F::J2 == 8 && F::R2 == 8 && F::I2 == 16 && F::M == 64, "H = 256, r = 8");
  constexpr int H = F::H;
  constexpr int PAR = ADJ ? 16 * F10T_ROW : 2 * 8 * 32;   // fp16 elements per parity of the h image
  constexpr int PIECE1 = ADJ ? F10T_ROW : 8 * 32;         // from a unit's first piece to its second

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_t[];
  _Float16* himg = reinterpret_cast<_Float16*>(smem_t);
  float* scratch = reinterpret_cast<float*>(himg + 2 * PAR);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  xh8 w10[F::R2][2];                                      // stage 1's B operand: built here (ttrnn_f10_dev.h)
  const F10hScales fsc = f10t_scales(hdr, f10t_build_w10<S>(w10, packed_hid, hdr, wave, lane), lane);
  const float hsc = F10T_HSC;
  const f32x4 psc = fsc.pre, usc = fsc.un;
  const int c = lane & 15, q = lane >> 4;
  const size_t b = blockIdx.x;

  xh8 g2[2][2];                                           // [k-block][piece]
  f10t_load_g2<S, ADJ>(g2, packed_hid, lane, hdr);

  // the hidden unit of this lane: hid = (4*wave + q)*I2 + c, gates in acc[0..3] = i,f,g,o; gin slots i,g,f,o
  const float* __restrict__ gin = gs.gin;
  const float* __restrict__ xs = reinterpret_cast<const float*>(gs.x);
  constexpr bool in1 = IN1;
  const int hd = (4 * wave + q) * F::I2 + c;
  // (j2, k) = (hd & 7, hd >> 3) of this unit in the image (first piece; second piece: + PIECE1), and this lane's A fragment
  const int hoff = ADJ ? f10t_img_off(2 * (hd & 7), hd >> 3) : (hd & 7) * 32 + (hd >> 3);
  const int aoff = ADJ ? f10t_img_off(c, 8 * q) : c * 32 + 8 * q;
  float hst = H0 ? h0[b * H + hd] : 0.f;
  float cst = c0 ? c0[b * H + hd] : 0.f;
  float h0sc = 1.0f, h0un = 1.0f;
  if constexpr (H0) {
    const int e0 = f10h_h0_expo<4>(hst, scratch, wave, lane);
    h0sc = ldexpf(1.f, -e0); h0un = ldexpf(1.f, e0);
  }
  f32x4 bh = f32x4{0.f, 0.f, 0.f, 0.f}, gi = bh, vv = bh, bb = bh;       // slot order i,g,f,o
  const f32x4 gsc = f32x4{-1.4426950408889634f, 2.8853900817779268f, -1.4426950408889634f, -1.4426950408889634f} *
                    f32x4{psc[0], psc[2], psc[1], psc[3]};      // slots i,g,f,o <- accumulator rows i,f,g,o
  XChunk<float> xq;
  xq.cur = 0.f; xq.nxt = 0.f;
  if (in1) xq.init(xs, b * T, T, lane);
  if (bias_hid) bh = f32x4{bias_hid[hd], bias_hid[2 * H + hd], bias_hid[H + hd], bias_hid[3 * H + hd]};
  if (T > 0) {
    if (in1) {
      bb = *reinterpret_cast<const f32x4*>(gin + (H + hd) * 4);
      vv = (*reinterpret_cast<const f32x4*>(gin + hd * 4) - bb) * gsc;
      bb = (bb + bh) * gsc;
    } else {
      gi = *reinterpret_cast<const f32x4*>(gin + ((b * T) * H + hd) * 4);
    }
  }
  {
    _Float16 p0, p1;                                       // parity 0 = h_{-1}
    split2h(hst * (hsc * h0sc), p0, p1);
    himg[hoff] = p0; himg[PIECE1 + hoff] = p1;
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) here, so that no weight-register wait lands inside the loop
  lds_barrier();

  unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long last_ = 0;
  if constexpr (DIAG) last_ = stamp();
  f32x4 us_t = usc * h0un;                  // step 0 runs on 2^-e0 h_0 (f10h_h0_expo); reset to usc / 1 at the end of it
  float ps_t = h0sc;
  xh8 ha;
  if constexpr (ADJ) ha = *reinterpret_cast<const xh8*>(himg + aoff);    // h_{-1}; inside the loop: read right behind the barrier
  for (int t = 0; t < T; ++t) {
    const _Float16* hp = himg + (t & 1) * PAR;            // pieces of h_{t-1}
    _Float16* hn = himg + ((t + 1) & 1) * PAR;            // pieces of h_t
    // ---- stage 1: eight tiles (one per r2), two chained MFMAs each: first-piece rows h0 (w0 + w1), second-piece rows h1 (w0 + w1)
    if constexpr (!ADJ) ha = *reinterpret_cast<const xh8*>(hp + aoff);
    f32x4 d[F::R2];
#pragma unroll
    for (int r = 0; r < F::R2; ++r) d[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, w10[r][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < F::R2; ++r) d[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, w10[r][1], d[r], 0, 0, 0);
    if constexpr (DIAG) {
#pragma unroll
      for (int r = 0; r < F::R2; ++r) asm volatile("" : "+v"(d[r]));
    }
    TT_STAMP(0)
    unsigned a0[2][4], a1[2][4];                           // [k-block][dword]: stage 2's A operand, k = 8 q + j
    if constexpr (ADJ) {
      // ---- fold in the lane: registers 0/1 = the two pieces' sums of j2 = 2 q, 2/3 of j2 = 2 q + 1; tile r2 -> dword r2 & 3 of
      //      k-block r2 >> 2 (f10t_load_g2<S, true>'s order), ready as soon as the tile's own two MFMAs have drained --------------
#pragma unroll
      for (int r = 0; r < F::R2; ++r)
        split_pair_h(d[r][0] + d[r][1], d[r][2] + d[r][3], a0[r >> 2][r & 3], a1[r >> 2][r & 3]);
    } else {
      // ---- fold tile pairs (p, p + 4): lanes 0-31 keep r2 = p, lanes 32-63 r2 = p + 4; then the two pieces of every sum ----------
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        f32x4 s;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(d[p][j]), __float_as_uint(d[p + 4][j]), false, false);
          s[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
        split_pair_h(s[0], s[1], a0[p >> 1][2 * (p & 1)], a1[p >> 1][2 * (p & 1)]);
        split_pair_h(s[2], s[3], a0[p >> 1][2 * (p & 1) + 1], a1[p >> 1][2 * (p & 1) + 1]);
      }
    }
    if constexpr (DIAG) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(a0[kb][j]), "+v"(a1[kb][j]));
    }
    TT_STAMP(1)
    const size_t bt = b * T + t;
    // ---- stage 2: d0 g0 into the accumulator that carries the input term, d0 g1 + d1 g0 into its own; gates + state ------------
    f32x4 acc;
    {
      // (W_in x_t + b_in + b_hid) * scale, slots i,g,f,o -> accumulator rows i,f,g,o
      f32x4 pre = in1 ? bb + xq.at(t) * vv : (gi + bh) * gsc;
      if constexpr (H0) pre = pre * ps_t;
      f32x4 acc_lo = f32x4{0.f, 0.f, 0.f, 0.f}, acc_hi = f32x4{pre[0], pre[2], pre[1], pre[3]};
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const xh8 d0 = __builtin_bit_cast(xh8, u32x4{a0[kb][0], a0[kb][1], a0[kb][2], a0[kb][3]});
        const xh8 d1 = __builtin_bit_cast(xh8, u32x4{a1[kb][0], a1[kb][1], a1[kb][2], a1[kb][3]});
        acc_lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(d0, g2[kb][1], acc_lo, 0, 0, 0);
        acc_lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(d1, g2[kb][0], acc_lo, 0, 0, 0);
        acc_hi = __builtin_amdgcn_mfma_f32_16x16x32_f16(d0, g2[kb][0], acc_hi, 0, 0, 0);
      }
      const f32x4 un = H0 ? us_t : usc;
      acc = acc_hi * un + acc_lo * un;                    // 2^-S per row and column (2^(e0-S) at step 0 of a given h_0), exact
      if constexpr (DIAG) asm volatile("" : "+v"(acc));
    }
    TT_STAMP(2)
    const float ig = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[0]));                // lstm.py:26
    const float fg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[1]));                // lstm.py:27
    const float gg = 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[2]));  // lstm.py:28
    const float og = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc[3]));                // lstm.py:29
    const float cy = fg * cst + ig * gg;                    // lstm.py:31
    const float hy = og * ftanh(cy);                        // lstm.py:32
    cst = cy;
    hst = hy;
    {
      _Float16 p0, p1;
      split2h(hy * hsc, p0, p1);
      hn[hoff] = p0; hn[PIECE1 + hoff] = p1;
    }
    if constexpr (OUT) out[bt * H + hd] = hy;               // outputs[:, t, :] (lstm.py:133): 256 contiguous bytes per wave
    if (reserve) {
      *reinterpret_cast<f32x4*>(reserve + res_gate(bt, H, hd)) = f32x4{ig, gg, fg, og};
      reserve[res_cell((size_t)B * T, bt, H, hd)] = cy;
    }
    if (!in1 && t + 1 < T) gi = *reinterpret_cast<const f32x4*>(gin + ((bt + 1) * H + hd) * 4);
    if (in1) xq.advance(xs, b * T, T, t, lane);
    us_t = usc; ps_t = 1.0f;
    TT_STAMP(3)
    lds_barrier();                                          // h_t published; the parity read in this step is free for h_{t+1}
    if constexpr (ADJ) {      // the next step's fragment at once: the pointer bumps and the loop control issue in the read's shadow
      ha = *reinterpret_cast<const xh8*>(hn + aoff);
      __builtin_amdgcn_sched_barrier(0);
    }
    TT_STAMP(4)
  }
  if (hT) hT[b * H + hd] = hst;
  if (cT) cT[b * H + hd] = cst;
  if constexpr (DIAG) {
    if (lane == 0 && reserve && b < 8) {
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(reserve) + (b * 8 + wave) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) dst[i] = seg[i];
    }
  }
}

template <class S, bool ADJ>
static int launch_f10t(const RnnShape& rs, GinSrc gin, const void* h0, const void* c0, const float* packed_hid, const float* hdr,
                       const float* bias_hid, void* out, void* hT, void* cT, float* reserve, hipStream_t stream) {
  auto kern = gin.in1 ? (out ? (h0 ? k_lstm_fwd_f10t<S, true, true, true, ADJ> : k_lstm_fwd_f10t<S, false, true, true, ADJ>)
                             : (h0 ? k_lstm_fwd_f10t<S, true, false, true, ADJ> : k_lstm_fwd_f10t<S, false, false, true, ADJ>))
                      : (out ? (h0 ? k_lstm_fwd_f10t<S, true, true, false, ADJ> : k_lstm_fwd_f10t<S, false, true, false, ADJ>)
                             : (h0 ? k_lstm_fwd_f10t<S, true, false, false, ADJ> : k_lstm_fwd_f10t<S, false, false, false, ADJ>));
  if (opt(OPT_DIAG) && reserve && out && !h0)      // stamped build (diagnostics)
    kern = gin.in1 ? k_lstm_fwd_f10t<S, false, true, true, ADJ, true> : k_lstm_fwd_f10t<S, false, true, false, ADJ, true>;
  hipLaunchKernelGGL(kern, dim3(rs.B), dim3(256), F10T_LDS_BYTES<ADJ>, stream, rs.B, rs.T, gin, (const float*)h0,
                     (const float*)c0, packed_hid, hdr, bias_hid, (float*)out, (float*)hT, (float*)cT, reserve);
  return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH;
}

}  // namespace ttrnn
