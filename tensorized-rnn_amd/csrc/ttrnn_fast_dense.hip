// ttrnn_fast_dense.hip — MFMA step kernels of the dense (nn.Linear, d = 1) LSTM / GRU layers: route TTRNN_ROUTE_DENSE_STEP (gfx950).
//
// The reference's uncompressed baselines (tensorized_rnn/lstm.py:7-41, gru.py:9-50) have no TT structure to keep on chip: a step is
// the GEMM [x_t | h_{t-1}] . [W_in ; W_hh] over the whole batch.  One launch per time step runs it on v_mfma_f32_16x16x32_bf16
// with the cell arithmetic (lstm.py:24-32 / gru.py:33-44) as the epilogue on the accumulators; workgroups are ordered by kernel
// boundaries only (no flags, no spin-waits, no atomics).  Layouts and the tile plan: ttrnn_dense.h.
//
//   forward   k_dense_prep_fwd (weight planes, planes of h0)  +  T x k_dense_fwd                         T + 1 launches
//   reverse   k_dense_prep_bwd (planes of W_hh for dh)        +  T x k_dense_bwd  +  1 closing k_dense_bwd  T + 2 launches
//
// Arithmetic: every operand is three bf16 pieces (ttrnn_split.h: x = x0 + x1 + x2 exactly), the six terms of weight >= 2^-18 —
// no scales, so x rows and gate-gradient rows of any range are safe.  The activations' pieces are written by the producing
// epilogue (h_t, d_gates_hid of step t) and read as ready fragments by the next launch; only the x columns are split in the loop.
// Each output element is summed by one wave in a fixed k order: results are repeatable bit for bit and a sample's result does not
// depend on the batch it runs in.
#include <hip/hip_runtime.h>
#include "ttrnn.h"
#include "ttrnn_core.h"
#include "ttrnn_dense.h"
#include "ttrnn_launch.h"
#include "ttrnn_split.h"

namespace ttrnn {
namespace {

__device__ __forceinline__ f32x4 mfma_bf16(xbf8 a, xbf8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void split8(const float (&v)[8], xbf8& p0, xbf8& p1, xbf8& p2) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 a, b, c;
    split3(v[e], a, b, c);
    p0[e] = a; p1[e] = b; p2[e] = c;
  }
}

// ---- weight planes ------------------------------------------------------------------------------------------------------
// value of column k of [W_in ; W_hh] (k < Kxp: input column, zero padded; else hidden column k - Kxp) for (slot, unit); packed
// d = 1 cores are W[j][o] (include/ttrnn.h: W_0[(j)*M + i])
__device__ __forceinline__ float dense_wcat(bool gru, int slot, int unit, int k, int in, int H, int Kxp, const float* __restrict__ pin,
                                            const float* __restrict__ phid) {
  const int G = gru ? 3 : 4;
  const bool xseg = k < Kxp;
  int gate;
  if (gru) {
    if (slot == 2 && !xseg) return 0.f;      // n_x: the x columns only
    if (slot == 3 && xseg) return 0.f;       // n_h: the h columns only
    gate = slot == 3 ? 2 : slot;
  } else {
    gate = dense_lstm_gate_of_slot(slot);
  }
  const size_t col = (size_t)gate * H + unit;
  if (xseg) return k < in ? pin[(size_t)k * G * H + col] : 0.f;
  return phid[(size_t)(k - Kxp) * G * H + col];
}

// one thread per (unit tile, k-block, slot, lane) of the WF planes, then one per 8 consecutive elements of h0
__global__ void __launch_bounds__(256) k_dense_prep_fwd(int gru, int B, int in, int H, int Kxp, long n_w, long n_h,
                                                        const float* __restrict__ pin, const float* __restrict__ phid,
                                                        const float* __restrict__ h0, __bf16* __restrict__ wf,
                                                        __bf16* __restrict__ hpl, long plane) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  float v[8];
  xbf8 p0, p1, p2;
  if (idx < n_w) {
    const int lane = (int)(idx & 63);
    const long frag = idx >> 6;                       // (ut * nkb + kb) * 4 + slot
    const int slot = (int)(frag & 3);
    const int nkb = (Kxp + H) / 32;
    const int kb = (int)((frag >> 2) % nkb);
    const int ut = (int)((frag >> 2) / nkb);
    const int n = lane & 15, q = lane >> 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = dense_wcat(gru != 0, slot, 16 * ut + n, 32 * kb + 8 * q + e, in, H, Kxp, pin, phid);
    split8(v, p0, p1, p2);
    xbf8* dst = reinterpret_cast<xbf8*>(wf) + frag * 3 * 64 + lane;
    dst[0] = p0; dst[64] = p1; dst[128] = p2;
    return;
  }
  const long e8 = idx - n_w;
  if (e8 >= n_h) return;
  const long el = e8 * 8;                             // element of [B][H], H % 8 == 0
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = h0 ? h0[el + e] : 0.f;
  split8(v, p0, p1, p2);
  *reinterpret_cast<xbf8*>(hpl + el) = p0;
  *reinterpret_cast<xbf8*>(hpl + plane + el) = p1;
  *reinterpret_cast<xbf8*>(hpl + 2 * plane + el) = p2;
}

// WR planes: k = column c of d_gates_hid, value W_hh[c][unit] from the transposed half Wt[c][j] of the packed core
__global__ void __launch_bounds__(256) k_dense_prep_bwd(int H, int GH, long n_w, const float* __restrict__ wt, __bf16* __restrict__ wr) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_w) return;
  const int lane = (int)(idx & 63);
  const long frag = idx >> 6;                         // ut * nkr + kb
  const int nkr = GH / 32;
  const int kb = (int)(frag % nkr), ut = (int)(frag / nkr);
  const int n = lane & 15, q = lane >> 4;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = wt[(size_t)(32 * kb + 8 * q + e) * H + 16 * ut + n];
  xbf8 p0, p1, p2;
  split8(v, p0, p1, p2);
  xbf8* dst = reinterpret_cast<xbf8*>(wr) + frag * 3 * 64 + lane;
  dst[0] = p0; dst[64] = p1; dst[128] = p2;
}

// ---- forward step ---------------------------------------------------------------------------------------------------------
struct DenseFwdArgs {
  int B, T, in, H, Kxp, t;
  const float* x;            // [B][T][in]
  const __bf16* wf;
  const __bf16* hpl_r;       // planes of h_{t-1}
  __bf16* hpl_w;             // planes of h_t (NULL at the last step)
  long plane;                // Bp * H
  const float* hprev; long hprev_stride;      // fp32 h_{t-1} rows (GRU epilogue): h0 / out[b][t-1] / ping-pong; NULL = zeros
  const float* cprev;        // c_{t-1} [.][H]: c0 / the workspace; NULL = zeros
  float* cnext;              // workspace
  const float* bin; const float* bhid;
  float* out;                // [B][T][H] or NULL
  float* h32_w;              // fp32 h_t for an out == NULL call, or NULL
  float* hT; float* cT;      // non-NULL at the last step only
  float* reserve;
};

template <bool GRU>
__global__ void __launch_bounds__(256) k_dense_fwd(const DenseFwdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int ut = blockIdx.x * 2 + (wave >> 1);
  const int row0 = blockIdx.y * DENSE_BATCH_TILE + 16 * (wave & 1);
  const int arow = row0 + n;                                   // this lane's row of the A operand (< Bp)
  const int H = a.H, nkx = a.Kxp / 32, nkb = nkx + H / 32;
  // per slot three accumulators, one per order of magnitude of the six terms (x0 w0 | x0 w1, x1 w0 | x0 w2, x1 w1, x2 w0): the
  // large sum is rounded once per k-block, not six times, and consecutive MFMAs do not wait for each other; added smallest first
  f32x4 c0[4], c1[4], c2[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) c0[s] = c1[s] = c2[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  const xbf8* wf = reinterpret_cast<const xbf8*>(a.wf) + (size_t)ut * nkb * 12 * 64 + lane;
  // x columns: split in the loop (zero beyond `in` and beyond the batch)
  const float* xr = a.x + ((size_t)(arow < a.B ? arow : 0) * a.T + a.t) * a.in;
  for (int kb = 0; kb < nkx; ++kb) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = 32 * kb + 8 * q + e;
      v[e] = (arow < a.B && j < a.in) ? xr[j] : 0.f;
    }
    xbf8 a0, a1, a2;
    split8(v, a0, a1, a2);
    const xbf8* w = wf + (size_t)kb * 12 * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (GRU && s == 3) continue;                             // n_h: no x columns
      const xbf8 w0 = w[(3 * s) * 64], w1 = w[(3 * s + 1) * 64], w2 = w[(3 * s + 2) * 64];
      c2[s] = mfma_bf16(a2, w0, c2[s]);
      c1[s] = mfma_bf16(a1, w0, c1[s]);
      c0[s] = mfma_bf16(a0, w0, c0[s]);
      c2[s] = mfma_bf16(a1, w1, c2[s]);
      c1[s] = mfma_bf16(a0, w1, c1[s]);
      c2[s] = mfma_bf16(a0, w2, c2[s]);
    }
  }
  // h columns: ready pieces.  Two k-blocks' fragments in registers: the loads of block kb + 1 are in flight under the MFMAs of
  // block kb (at 1.5 waves per SIMD nothing else hides an L2 round trip per k-block)
  const __bf16* hr = a.hpl_r + (size_t)arow * H + 8 * q;
  struct Frag { xbf8 a[3]; xbf8 w[12]; };
  auto load = [&](Frag& f, int kb) {
    const __bf16* hp = hr + 32 * (kb - nkx);
    f.a[0] = *reinterpret_cast<const xbf8*>(hp);
    f.a[1] = *reinterpret_cast<const xbf8*>(hp + a.plane);
    f.a[2] = *reinterpret_cast<const xbf8*>(hp + 2 * a.plane);
    const xbf8* w = wf + (size_t)kb * 12 * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (GRU && s == 2) continue;                             // n_x: no h columns
#pragma unroll
      for (int p = 0; p < 3; ++p) f.w[3 * s + p] = w[(3 * s + p) * 64];
    }
  };
  auto compute = [&](const Frag& f) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (GRU && s == 2) continue;
      c2[s] = mfma_bf16(f.a[2], f.w[3 * s], c2[s]);
      c1[s] = mfma_bf16(f.a[1], f.w[3 * s], c1[s]);
      c0[s] = mfma_bf16(f.a[0], f.w[3 * s], c0[s]);
      c2[s] = mfma_bf16(f.a[1], f.w[3 * s + 1], c2[s]);
      c1[s] = mfma_bf16(f.a[0], f.w[3 * s + 1], c1[s]);
      c2[s] = mfma_bf16(f.a[0], f.w[3 * s + 2], c2[s]);
    }
  };
  {
    Frag f0, f1;
    load(f0, nkx);
    int kb = nkx;
    for (; kb + 1 < nkb; kb += 2) {
      load(f1, kb + 1);
      compute(f0);
      if (kb + 2 < nkb) load(f0, kb + 2);
      compute(f1);
    }
    if (kb < nkb) compute(f0);
  }
  f32x4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = (c2[s] + c1[s]) + c0[s];
  // the cell on the accumulators: lane (n, q) holds the four slots of unit 16 ut + n for rows row0 + 4 q + i
  const int u = 16 * ut + n;
  const size_t RROWS = (size_t)a.B * a.T;
  float b0, b1, b2, b3;      // per-slot biases (GRU: b3 = the hidden n bias, b2 = the input n bias)
  if (GRU) {
    b0 = (a.bin ? a.bin[u] : 0.f) + (a.bhid ? a.bhid[u] : 0.f);
    b1 = (a.bin ? a.bin[H + u] : 0.f) + (a.bhid ? a.bhid[H + u] : 0.f);
    b2 = a.bin ? a.bin[2 * H + u] : 0.f;
    b3 = a.bhid ? a.bhid[2 * H + u] : 0.f;
  } else {
    b0 = (a.bin ? a.bin[u] : 0.f) + (a.bhid ? a.bhid[u] : 0.f);                        // i
    b1 = (a.bin ? a.bin[2 * H + u] : 0.f) + (a.bhid ? a.bhid[2 * H + u] : 0.f);        // g
    b2 = (a.bin ? a.bin[H + u] : 0.f) + (a.bhid ? a.bhid[H + u] : 0.f);                // f
    b3 = (a.bin ? a.bin[3 * H + u] : 0.f) + (a.bhid ? a.bhid[3 * H + u] : 0.f);        // o
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = row0 + 4 * q + i;
    if (r >= a.B) continue;
    const size_t bt = (size_t)r * a.T + a.t;
    const size_t e = (size_t)r * H + u;
    float hy;
    if (GRU) {
      const float rg = sigmoidf_(acc[0][i] + b0), zg = sigmoidf_(acc[1][i] + b1);
      const float hn = acc[3][i] + b3;
      const float ng = tanhf(acc[2][i] + b2 + rg * hn);
      const float hp = a.hprev ? a.hprev[(size_t)r * a.hprev_stride + u] : 0.f;
      hy = (1.0f - zg) * ng + zg * hp;
      if (a.reserve) *reinterpret_cast<f32x4*>(a.reserve + res_gate(bt, H, u)) = f32x4{rg, zg, ng, hn};
    } else {
      const float ig = sigmoidf_(acc[0][i] + b0), gg = tanhf(acc[1][i] + b1);
      const float fg = sigmoidf_(acc[2][i] + b2), og = sigmoidf_(acc[3][i] + b3);
      const float cp = a.cprev ? a.cprev[e] : 0.f;
      const float cy = fg * cp + ig * gg;
      hy = og * tanhf(cy);
      a.cnext[e] = cy;
      if (a.cT) a.cT[e] = cy;
      if (a.reserve) {
        *reinterpret_cast<f32x4*>(a.reserve + res_gate(bt, H, u)) = f32x4{ig, gg, fg, og};
        a.reserve[res_cell(RROWS, bt, H, u)] = cy;
      }
    }
    if (a.out) a.out[bt * H + u] = hy;
    if (a.h32_w) a.h32_w[e] = hy;
    if (a.hT) a.hT[e] = hy;
    if (a.hpl_w) {
      __bf16 p0, p1, p2;
      split3(hy, p0, p1, p2);
      a.hpl_w[e] = p0; a.hpl_w[a.plane + e] = p1; a.hpl_w[2 * a.plane + e] = p2;
    }
  }
}

// ---- reverse step ---------------------------------------------------------------------------------------------------------
struct DenseBwdArgs {
  int B, T, H, t;            // t = -1: the closing launch (d_h0 / d_c0 only)
  int gemm;                  // 0 at step T - 1: no later step, dh = d_out + d_hT
  const __bf16* wr;
  const __bf16* dgpl_r;      // planes of d_gates_hid of step t + 1
  __bf16* dgpl_w;            // planes of this step's d_gates_hid
  long plane;                // Bp * G * H
  float* carry;              // [Bp][H]: dc f (LSTM) / dh z (GRU) of the previous launch, replaced by this step's
  const float* reserve; const float* out; const float* h0; const float* c0;
  const float* d_out; const float* d_hT; const float* d_cT;
  float* dg_in; float* dg_hid;
  float* d_h0; float* d_c0;
};

template <bool GRU>
__global__ void __launch_bounds__(256) k_dense_bwd(const DenseBwdArgs a) {
  constexpr int G = GRU ? 3 : 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int ut = blockIdx.x * 2 + (wave >> 1);
  const int row0 = blockIdx.y * DENSE_BATCH_TILE + 16 * (wave & 1);
  const int arow = row0 + n;
  const int H = a.H, GH = G * H, nkr = GH / 32;
  // three independent accumulators, one per order of magnitude of the terms; added smallest first
  f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0;
  if (a.gemm) {
    const xbf8* w = reinterpret_cast<const xbf8*>(a.wr) + (size_t)ut * nkr * 3 * 64 + lane;
    const __bf16* dr = a.dgpl_r + (size_t)arow * GH + 8 * q;
    // a ring of four k-blocks' fragments: three blocks' loads in flight under the MFMAs of the fourth (K = G H is long and a wave
    // has one output tile: without it every k-block waits out its own L2 round trip)
    struct Frag { xbf8 a[3]; xbf8 w[3]; };
    auto load = [&](Frag& f, int kb) {
      const __bf16* dp = dr + 32 * kb;
      f.a[0] = *reinterpret_cast<const xbf8*>(dp);
      f.a[1] = *reinterpret_cast<const xbf8*>(dp + a.plane);
      f.a[2] = *reinterpret_cast<const xbf8*>(dp + 2 * a.plane);
      f.w[0] = w[(size_t)kb * 3 * 64]; f.w[1] = w[(size_t)kb * 3 * 64 + 64]; f.w[2] = w[(size_t)kb * 3 * 64 + 128];
    };
    Frag f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < nkr) load(f[u], u);
    for (int kb = 0; kb < nkr; kb += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (kb + u < nkr) {
          c2 = mfma_bf16(f[u].a[2], f[u].w[0], c2);
          c1 = mfma_bf16(f[u].a[1], f[u].w[0], c1);
          c0 = mfma_bf16(f[u].a[0], f[u].w[0], c0);
          c2 = mfma_bf16(f[u].a[1], f[u].w[1], c2);
          c1 = mfma_bf16(f[u].a[0], f[u].w[1], c1);
          c2 = mfma_bf16(f[u].a[0], f[u].w[2], c2);
          if (kb + u + 4 < nkr) load(f[u], kb + u + 4);
        }
      }
    }
  }
  const f32x4 acc = (c2 + c1) + c0;
  const int u = 16 * ut + n;
  const size_t RROWS = (size_t)a.B * a.T;
  const bool last = a.t == a.T - 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = row0 + 4 * q + i;
    if (r >= a.B) continue;
    const size_t e = (size_t)r * H + u;
    if (a.t < 0) {                                   // closing launch: the state gradients of step 0's inputs
      float dh = acc[i];
      if (GRU) dh += a.carry[e];
      if (a.d_h0) a.d_h0[e] = dh;
      if (!GRU && a.d_c0) a.d_c0[e] = a.carry[e];
      continue;
    }
    const size_t bt = (size_t)r * a.T + a.t;
    const f32x4 rv = *reinterpret_cast<const f32x4*>(a.reserve + res_gate(bt, H, u));
    float dht = acc[i];
    if (GRU && !last) dht += a.carry[e];
    if (last && a.d_hT) dht += a.d_hT[e];
    if (a.d_out) dht += a.d_out[bt * H + u];
    float* gp = a.dg_in + bt * GH;
    float p0, p1, p2, p3 = 0.f, ph2;                 // gate-order values for d_gates_in; ph2: the hidden n column (GRU)
    if (GRU) {
      const float rg = rv[0], zg = rv[1], ng = rv[2], hn = rv[3];
      const float hprev = a.t > 0 ? a.out[(bt - 1) * H + u] : (a.h0 ? a.h0[e] : 0.f);
      const float dn_pre = dht * (1.0f - zg) * (1.0f - ng * ng);
      p1 = dht * (hprev - ng) * zg * (1.0f - zg);
      p0 = dn_pre * hn * rg * (1.0f - rg);
      p2 = dn_pre;
      ph2 = dn_pre * rg;
      a.carry[e] = dht * zg;
      gp[u] = p0; gp[H + u] = p1; gp[2 * H + u] = p2;
      float* gq = a.dg_hid + bt * GH;
      gq[u] = p0; gq[H + u] = p1; gq[2 * H + u] = ph2;
    } else {
      const float ig = rv[0], gg = rv[1], fg = rv[2], og = rv[3], cy = a.reserve[res_cell(RROWS, bt, H, u)];
      const float cprev = a.t > 0 ? a.reserve[res_cell(RROWS, bt - 1, H, u)] : (a.c0 ? a.c0[e] : 0.f);
      const float dcin = last ? (a.d_cT ? a.d_cT[e] : 0.f) : a.carry[e];
      const float tc = tanhf(cy);
      const float dct = dcin + dht * og * (1.0f - tc * tc);
      p0 = dct * gg * ig * (1.0f - ig);
      p1 = dct * cprev * fg * (1.0f - fg);
      p2 = dct * ig * (1.0f - gg * gg);
      p3 = dht * tc * og * (1.0f - og);
      ph2 = p2;
      a.carry[e] = dct * fg;
      gp[u] = p0; gp[H + u] = p1; gp[2 * H + u] = p2; gp[3 * H + u] = p3;
      if (a.dg_hid && a.dg_hid != a.dg_in) {
        float* gq = a.dg_hid + bt * GH;
        gq[u] = p0; gq[H + u] = p1; gq[2 * H + u] = p2; gq[3 * H + u] = p3;
      }
    }
    // pieces of d_gates_hid for the next launch's GEMM
    const float dv[4] = {p0, p1, ph2, p3};
    __bf16* pw = a.dgpl_w + (size_t)r * GH + u;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      __bf16 s0, s1, s2;
      split3(dv[g], s0, s1, s2);
      pw[(size_t)g * H] = s0; pw[a.plane + (size_t)g * H] = s1; pw[2 * a.plane + (size_t)g * H] = s2;
    }
  }
}

}  // namespace

// fp32 storage, split math, one core per matrix, H >= 128 and a multiple of the unit tile: the uncompressed baselines
bool dense_step_available(const RnnShape& rs, int dtype, int fp32_math) {
  return dtype == TTRNN_F32 && fp32_math == TTRNN_MATH_SPLIT && rs.in_s.d == 1 && rs.hid_s.d == 1 && rs.hid_blocks <= 1 &&
         rs.H >= DENSE_MIN_H && rs.H % DENSE_UNIT_TILE == 0 && rs.B > 0 && rs.T > 0;
}
size_t dense_step_fwd_workspace(const RnnShape& rs) { return dense_plan(rs).fwd_bytes; }
size_t dense_step_bwd_workspace(const RnnShape& rs) { return dense_plan(rs).bwd_bytes; }

int launch_rnn_fwd_dense(const RnnShape& rs, const void* x, const void* h0, const void* c0, const float* packed_in,
                         const void* bias_in, const float* packed_hid, const void* bias_hid, void* out, void* hT, void* cT,
                         float* reserve, void* ws, hipStream_t stream) {
  const DensePlan p = dense_plan(rs);
  const bool gru = rs.cell == TTRNN_GRU;
  const int H = rs.H, T = rs.T;
  char* w = (char*)ws;
  __bf16* wf = (__bf16*)w; w += p.wf_bytes;
  __bf16* hpl = (__bf16*)w; w += p.hpl_bytes;
  float* cbuf = (float*)w; w += p.c_bytes;
  float* h32 = (float*)w;
  const long plane = (long)p.Bp * H;
  const long n_w = (long)(H / 16) * p.nkb * 4 * 64, n_h = (long)rs.B * H / 8;
  // h0's pieces go where step 0 reads them: buffer 1 (step t reads buffer (t & 1) ^ 1 and writes buffer t & 1)
  hipLaunchKernelGGL(k_dense_prep_fwd, dim3((unsigned)((n_w + n_h + 255) / 256)), dim3(256), 0, stream, gru ? 1 : 0, rs.B, rs.in, H,
                     p.Kxp, n_w, n_h, packed_in, packed_hid, (const float*)h0, wf, hpl + 3 * plane, plane);
  DenseFwdArgs a{};
  a.B = rs.B; a.T = T; a.in = rs.in; a.H = H; a.Kxp = p.Kxp;
  a.x = (const float*)x; a.wf = wf; a.plane = plane;
  a.cnext = cbuf;
  a.bin = rs.has_bias_in ? (const float*)bias_in : nullptr;
  a.bhid = rs.has_bias_hid ? (const float*)bias_hid : nullptr;
  a.out = (float*)out; a.reserve = reserve;
  const dim3 grid((unsigned)(H / DENSE_UNIT_TILE), (unsigned)(p.Bp / DENSE_BATCH_TILE));
  for (int t = 0; t < T; ++t) {
    a.t = t;
    a.hpl_r = hpl + (size_t)((t & 1) ^ 1) * 3 * plane;
    a.hpl_w = t + 1 < T ? hpl + (size_t)(t & 1) * 3 * plane : nullptr;
    if (t == 0) { a.hprev = (const float*)h0; a.hprev_stride = H; }
    else if (out) { a.hprev = (const float*)out + (size_t)(t - 1) * H; a.hprev_stride = (long)T * H; }
    else { a.hprev = h32 + (size_t)((t & 1) ^ 1) * plane; a.hprev_stride = H; }
    a.h32_w = (!out && gru && t + 1 < T) ? h32 + (size_t)(t & 1) * plane : nullptr;
    a.cprev = t == 0 ? (const float*)c0 : cbuf;
    a.hT = t + 1 == T ? (float*)hT : nullptr;
    a.cT = t + 1 == T ? (float*)cT : nullptr;
    if (gru) hipLaunchKernelGGL(k_dense_fwd<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_dense_fwd<false>, grid, dim3(256), 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH;      // once, after the loop
}

int launch_rnn_bwd_dense(const RnnShape& rs, const void* out, const void* h0, const void* c0, const float* packed_hid,
                         const float* reserve, const void* d_out, const void* d_hT, const void* d_cT, float* dg_in, float* dg_hid,
                         void* d_h0, void* d_c0, void* ws, hipStream_t stream) {
  const DensePlan p = dense_plan(rs);
  const bool gru = rs.cell == TTRNN_GRU;
  const int H = rs.H, T = rs.T, GH = rs.G * H;
  char* w = (char*)ws;
  __bf16* wr = (__bf16*)w; w += p.wr_bytes;
  __bf16* dgpl = (__bf16*)w; w += p.dgpl_bytes;
  float* carry = (float*)w;
  const long plane = (long)p.Bp * GH;
  const long n_w = (long)(H / 16) * p.nkr * 64;
  hipLaunchKernelGGL(k_dense_prep_bwd, dim3((unsigned)((n_w + 255) / 256)), dim3(256), 0, stream, H, GH, n_w,
                     packed_hid + (size_t)H * GH, wr);
  DenseBwdArgs a{};
  a.B = rs.B; a.T = T; a.H = H;
  a.wr = wr; a.plane = plane; a.carry = carry;
  a.reserve = reserve; a.out = (const float*)out; a.h0 = (const float*)h0; a.c0 = (const float*)c0;
  a.d_out = (const float*)d_out; a.d_hT = (const float*)d_hT; a.d_cT = (const float*)d_cT;
  a.dg_in = dg_in; a.dg_hid = dg_hid; a.d_h0 = (float*)d_h0; a.d_c0 = (float*)d_c0;
  const dim3 grid((unsigned)(H / DENSE_UNIT_TILE), (unsigned)(p.Bp / DENSE_BATCH_TILE));
  for (int t = T - 1; t >= -1; --t) {      // step t reads the planes step t + 1 wrote (buffer (t + 1) & 1), writes buffer t & 1
    a.t = t;
    a.gemm = t < T - 1 ? 1 : 0;
    a.dgpl_r = dgpl + (size_t)((t + 1) & 1) * 3 * plane;
    a.dgpl_w = dgpl + (size_t)(t & 1) * 3 * plane;
    if (gru) hipLaunchKernelGGL(k_dense_bwd<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_dense_bwd<false>, grid, dim3(256), 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH;
}

}  // namespace ttrnn
