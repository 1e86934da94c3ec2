// ttrnn_generic.hip — any-shape kernels of libttrnn (gfx950) and their launchers.
//
// These kernels accept every descriptor include/ttrnn.h allows (any d <= 6, any modes / ranks,
// LSTM / GRU, f32 / bf16 storage): one workgroup per batch tile, sequence loop on device, state and
// chain intermediates in LDS (spilling to a global workspace only when a sample's intermediates do
// not fit 160 KB), fp32 VALU FMAs with 4-row register tiles.  The shape-specialised MFMA kernels in
// ttrnn_fast.hip take over for the configurations they are built for (see ttrnn_api.hip).
#include <hip/hip_runtime.h>
#include "ttrnn_core.h"
#include "ttrnn_launch.h"

namespace ttrnn {

struct DevExec {
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
  }
};

struct AddPlain {
  __device__ __forceinline__ void operator()(float* p, float v) const { *p += v; }
};
struct AddAtomic {
  __device__ __forceinline__ void operator()(float* p, float v) const { atomicAdd(p, v); }
};

static constexpr int NT_RNN = 512;
static constexpr int NT_LIN = 256;

__device__ __forceinline__ void copy_to_lds(float* dst, const float* src, int n) {
  for (int e = threadIdx.x; e < n; e += blockDim.x) dst[e] = src[e];
}

// The two unit input rows x = [1, 0] of the input_size == 1 paths live in device constants (one launch less per
// forward than filling them into the workspace: the cfg2 step has only six launches, ~8 us each)
__device__ __attribute__((used)) float g_unit_rows_f32[4] = {1.0f, 0.0f, 0.0f, 0.0f};
__device__ __attribute__((used)) uint16_t g_unit_rows_bf16[4] = {0x3F80, 0, 0, 0};        // bf16(1.0), bf16(0.0)

const void* unit_rows_ptr(int dtype) {
  static const void* cached[16][2] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) {
    (void)hipGetLastError();
    dev = 0;
  }
  const int di = dtype == TTRNN_F32 ? 0 : 1;
  if (!cached[dev][di]) {
    void* p = nullptr;
    const hipError_t e = di == 0 ? hipGetSymbolAddress(&p, HIP_SYMBOL(g_unit_rows_f32))
                                 : hipGetSymbolAddress(&p, HIP_SYMBOL(g_unit_rows_bf16));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    cached[dev][di] = p;
  }
  return cached[dev][di];
}

// input_size == 1: y_n = b + x_n * v  =>  dL/dv[o] = sum_n x_n dy[n][o],  dL/db[o] = sum_n dy[n][o].
typedef float4 f32x4_t;

// One pass over dy (HBM-bound: reads n_rows * out values once).  A workgroup owns a slab of rows; a thread owns FOUR
// consecutive columns (one 16-byte load per row when dy is fp32) and walks the slab eight rows at a time so that eight
// independent loads are in flight per lane; partial sums leave through one atomic per column and workgroup.
static constexpr int IN1_PARTS = 512;      // workgroups of k_in1_reduce at most (two per CU)

template <typename TX, typename TDY>
__global__ void __launch_bounds__(256) k_in1_reduce(int64_t n_rows, int out, int rows_per_wg, const TX* __restrict__ x,
                                                    const TDY* __restrict__ dy, float* __restrict__ part, int want_db) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < n_rows ? r0 + rows_per_wg : n_rows;
  if (r0 >= r1) return;
  for (int o = 4 * threadIdx.x; o < out; o += 4 * blockDim.x) {
    float av[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
    const int nc = out - o < 4 ? out - o : 4;
    int64_t n = r0;
    if (nc == 4 && out % 4 == 0) {      // 16-byte aligned rows
      for (; n + 8 <= r1; n += 8) {
        float g[8][4], xv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if constexpr (sizeof(TDY) == 4) {
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(dy) + (size_t)(n + k) * out + o);
            g[k][0] = v.x; g[k][1] = v.y; g[k][2] = v.z; g[k][3] = v.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[k][j] = ld(dy, (size_t)(n + k) * out + o + j);
          }
          xv[k] = ld(x, (size_t)(n + k));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            av[j] = fmaf(xv[k], g[k][j], av[j]);
            ab[j] += g[k][j];
          }
      }
    }
    for (; n < r1; ++n) {
      const float xn = ld(x, (size_t)n);
      for (int j = 0; j < nc; ++j) {
        const float g = ld(dy, (size_t)n * out + o + j);
        av[j] = fmaf(xn, g, av[j]);
        ab[j] += g;
      }
    }
    // this workgroup's partial sums [2][out] (every launched workgroup has rows: the grid is cut to the rows); summed in a
    // fixed order by k_in1_finish — round 3 flushed them with atomicAdd: the last bits depended on the order of arrival
    float* pw = part + (size_t)blockIdx.x * 2 * out;
    for (int j = 0; j < nc; ++j) {
      pw[o + j] = av[j];
      if (want_db) pw[out + o + j] = ab[j];
    }
  }
}

// dv[o] = sum over the workgroups' partials (overwritten), db[o] += the same for the plain sums: 8 columns x 32 groups of
// workgroups per block — a thread walks its group's (<= 16) partial rows with four loads in flight, then ONE thread per column adds
// the 32 group sums in order from LDS (a thread walking 56 rows one dependent L2 latency at a time made this a 20 us kernel)
__global__ void __launch_bounds__(256) k_in1_finish(const float* __restrict__ part, int nparts, int out, float* __restrict__ dv,
                                                    float* __restrict__ db) {
  __shared__ float red[2][32][8];
  const int c = threadIdx.x & 7, kg = threadIdx.x >> 3;
  const int o = blockIdx.x * 8 + c;
  const int per = (nparts + 31) / 32, k0 = kg * per, k1 = k0 + per < nparts ? k0 + per : nparts;
  const bool wb = db != nullptr;
  float a = 0.f, b = 0.f;
  if (o < out) {
    int k = k0;
    for (; k + 4 <= k1; k += 4) {
      float va[4], vb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        va[i] = part[(size_t)(k + i) * 2 * out + o];
        vb[i] = wb ? part[(size_t)(k + i) * 2 * out + out + o] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) { a += va[i]; b += vb[i]; }
    }
    for (; k < k1; ++k) {
      a += part[(size_t)k * 2 * out + o];
      if (wb) b += part[(size_t)k * 2 * out + out + o];
    }
  }
  red[0][kg][c] = a;
  red[1][kg][c] = b;
  __syncthreads();
  if (kg == 0 && o < out) {
    float sa = red[0][0][c], sb = red[1][0][c];
#pragma unroll
    for (int g = 1; g < 32; ++g) { sa += red[0][g][c]; sb += red[1][g][c]; }
    dv[o] = sa;
    if (wb) db[o] += sb;
  }
}

size_t in1_reduce_part_bytes(int out) { return (size_t)IN1_PARTS * 2 * out * sizeof(float); }

int launch_in1_reduce(int dtype, int dy_dtype, int64_t n_rows, int out, const void* x, const void* dy, float* dv,
                      float* db, float* part, hipStream_t stream) {
  // at most IN1_PARTS workgroups (two per CU), each leaving one row of partial sums
  if (n_rows <= 0) {      // no rows: the sums are zero (k_in1_finish would add up a partial row nobody wrote — ADVICE r4)
    if (hipMemsetAsync(dv, 0, (size_t)out * sizeof(float), stream) != hipSuccess) return TTRNN_ERR_LAUNCH;
    return TTRNN_OK;
  }
  if (!part) return TTRNN_ERR_WORKSPACE;
  int rows_per_wg = (int)((n_rows + IN1_PARTS - 1) / IN1_PARTS);
  rows_per_wg = (rows_per_wg + 7) & ~7;
  if (rows_per_wg < 8) rows_per_wg = 8;
  const int grid = (int)((n_rows + rows_per_wg - 1) / rows_per_wg) > 0 ? (int)((n_rows + rows_per_wg - 1) / rows_per_wg) : 1;
#define TT_L(TX, TDY) hipLaunchKernelGGL((k_in1_reduce<TX, TDY>), dim3(grid), dim3(256), 0, stream, n_rows, out, rows_per_wg, (const TX*)x, (const TDY*)dy, part, db ? 1 : 0)
  if (dtype == TTRNN_F32 && dy_dtype == TTRNN_F32) TT_L(float, float);
  else if (dtype == TTRNN_F32) TT_L(float, bf16_t);
  else if (dy_dtype == TTRNN_F32) TT_L(bf16_t, float);
  else TT_L(bf16_t, bf16_t);
#undef TT_L
  hipLaunchKernelGGL(k_in1_finish, dim3((out + 7) / 8), dim3(256), 0, stream, (const float*)part, grid, out, dv, db);
  return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------
// pack / unpack
// ---------------------------------------------------------------------------------------------
struct PackArgs {
  const void* core[TTRNN_MAX_D];
  void* grad[TTRNN_MAX_D];
  int64_t st[TTRNN_MAX_D * 4];
};

template <typename T>
__global__ void k_pack_cores(TtShape s, PackArgs a, float* packed) {
  const int k = blockIdx.y;
  pack_core_elems<T>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, s, k,
                     (const T*)a.core[k], &a.st[4 * k], packed);
}

// two TT-matrices (a layer's input and hidden weights) in ONE launch: blockIdx.y < sa.d packs matrix a, the rest matrix b
template <typename T>
__global__ void k_pack_cores2(TtShape sa, PackArgs aa, float* packed_a, TtShape sb, PackArgs ab, float* packed_b) {
  const int k = blockIdx.y;
  if (k < sa.d)
    pack_core_elems<T>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, sa, k,
                       (const T*)aa.core[k], &aa.st[4 * k], packed_a);
  else
    pack_core_elems<T>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, sb, k - sa.d,
                       (const T*)ab.core[k - sa.d], &ab.st[4 * (k - sa.d)], packed_b);
}

template <typename T>
__global__ void k_unpack_core_grads(TtShape s, PackArgs a, const float* packed_grad) {
  const int k = blockIdx.y;
  unpack_core_grad_elems<T>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, s, k,
                            packed_grad, (T*)a.grad[k], &a.st[4 * k]);
}

// ---------------------------------------------------------------------------------------------
// TTLinear forward / backward over n_rows rows (grid-stride over tiles of nb rows)
// ---------------------------------------------------------------------------------------------
template <typename T, bool W_LDS, bool BUF_GLOBAL>
__global__ void __launch_bounds__(NT_LIN) k_ttlinear_fwd(TtShape s, int64_t n_rows, int nb, int bs,
                                                         const float* packed, const T* bias, const T* x, T* y,
                                                         float* ws, int ilv_h, int ilv_mode, int epi, float* aux) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  DevExec ex;
  float* p = smem;
  float *bufA, *bufB;
  if (BUF_GLOBAL) {
    bufA = ws + (size_t)blockIdx.x * 2 * nb * bs; bufB = bufA + (size_t)nb * bs;
  } else {
    bufA = p; p += (size_t)nb * bs; bufB = p; p += (size_t)nb * bs;
  }
  const float* W = packed;
  if (W_LDS) { copy_to_lds(p, packed, s.wtotal); W = p; __syncthreads(); }
  const int64_t ntiles = (n_rows + nb - 1) / nb;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * nb;
    const int n = (int)tmin<int64_t>(nb, n_rows - n0);
    ttlinear_fwd_tile<DevExec, T>(ex, s, W, bias, x, y, n0, n, bufA, bufB, bs, ilv_h, ilv_mode, epi, aux);
  }
}

// ACC: 0 = atomics from every row straight into d_packed / d_bias; 1 = accumulators in LDS, one atomic flush per workgroup;
// 2 = accumulators too large for LDS (a classifier head 1024 -> 256 with rank 32: 200 KB): a private global slab per
// workgroup, plain adds (L2-resident), summed into d_packed / d_bias by k_slab_reduce — 33 k atomics per row from 128
// workgroups into ONE buffer cost 1.85 ms of cfg5's training step
template <typename T, typename TDY, bool BUF_GLOBAL, int ACC>
__global__ void __launch_bounds__(NT_LIN) k_ttlinear_bwd(TtShape s, int64_t n_rows, int nb, int bs, int ss,
                                                         const float* packed, const T* x, const TDY* dy, T* dx,
                                                         float* d_packed, float* d_bias, float* ws, float* slabs, int mixed) {
  constexpr bool ACC_LDS = ACC == 1 || ACC == 3;      // 3: LDS accumulators flushed into this workgroup's slab (fixed-order sums)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  DevExec ex;
  float* p = smem;
  float *bufA, *bufB, *stash;
  if (BUF_GLOBAL) {
    float* base = ws + (size_t)blockIdx.x * ((size_t)2 * nb * bs + (size_t)nb * ss);
    bufA = base; bufB = bufA + (size_t)nb * bs; stash = bufB + (size_t)nb * bs;
    if (mixed) {      // LinPlan::buf_mixed: the two ping-pong buffers fit LDS, only the stash of stage inputs stays in the workspace
      bufA = p; p += (size_t)nb * bs; bufB = p; p += (size_t)nb * bs;
    }
  } else {
    bufA = p; p += (size_t)nb * bs; bufB = p; p += (size_t)nb * bs; stash = p; p += (size_t)nb * ss;
  }
  float* dWacc = d_packed;
  float* dbacc = d_bias;
  if (ACC_LDS) {
    if (d_packed) { dWacc = p; p += s.wtotal; for (int e = threadIdx.x; e < s.wtotal; e += blockDim.x) dWacc[e] = 0.f; }
    if (d_bias) { dbacc = p; p += s.out_size; for (int e = threadIdx.x; e < s.out_size; e += blockDim.x) dbacc[e] = 0.f; }
    __syncthreads();
  }
  if (ACC == 2) {
    float* slab = slabs + (size_t)blockIdx.x * ((size_t)s.wtotal + s.out_size);
    if (d_packed) { dWacc = slab; for (int e = threadIdx.x; e < s.wtotal; e += blockDim.x) dWacc[e] = 0.f; }
    if (d_bias) { dbacc = slab + s.wtotal; for (int e = threadIdx.x; e < s.out_size; e += blockDim.x) dbacc[e] = 0.f; }
    __threadfence_block();
    __syncthreads();
  }
  const float* W = packed;
  const float* Wt = packed + s.wtotal;
  const int64_t ntiles = (n_rows + nb - 1) / nb;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n0 = tile * nb;
    const int n = (int)tmin<int64_t>(nb, n_rows - n0);
    if (ACC_LDS || ACC == 2)
      ttlinear_bwd_tile<DevExec, T, TDY>(ex, s, W, Wt, x, dy, dx, dWacc, dbacc, n0, n, stash, ss, bufA, bufB, bs, AddPlain(),
                                         BUF_GLOBAL && mixed);
    else
      ttlinear_bwd_tile<DevExec, T, TDY>(ex, s, W, Wt, x, dy, dx, dWacc, dbacc, n0, n, stash, ss, bufA, bufB, bs, AddAtomic(),
                                         BUF_GLOBAL && mixed);
  }
  if (ACC == 3) {
    __syncthreads();
    float* slab = slabs + (size_t)blockIdx.x * ((size_t)s.wtotal + s.out_size);
    for (int e = threadIdx.x; e < s.wtotal; e += blockDim.x) slab[e] = d_packed ? dWacc[e] : 0.f;
    for (int e = threadIdx.x; e < s.out_size; e += blockDim.x) slab[s.wtotal + e] = d_bias ? dbacc[e] : 0.f;
  } else if (ACC_LDS) {
    __syncthreads();
    if (d_packed) for (int e = threadIdx.x; e < s.wtotal; e += blockDim.x) { const float v = dWacc[e]; if (v != 0.f) atomicAdd(d_packed + e, v); }
    if (d_bias) for (int e = threadIdx.x; e < s.out_size; e += blockDim.x) { const float v = dbacc[e]; if (v != 0.f) atomicAdd(d_bias + e, v); }
  }
}

// dst[e] += sum over the `grid` slabs (each [wtotal | out] floats) of slab[e]  (k_ttlinear_bwd, ACC = 2)
__global__ void __launch_bounds__(256) k_slab_reduce(const float* __restrict__ slabs, int grid, int wtotal, int out,
                                                     float* __restrict__ d_packed, float* __restrict__ d_bias) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int per = wtotal + out;
  if (e >= per) return;
  float* dst = e < wtotal ? (d_packed ? d_packed + e : nullptr) : (d_bias ? d_bias + (e - wtotal) : nullptr);
  if (!dst) return;
  float v = 0.f;
  for (int g = 0; g < grid; ++g) v += slabs[(size_t)g * per + e];
  *dst += v;
}

// ---------------------------------------------------------------------------------------------
// recurrent layer: persistent over the sequence, one workgroup per tile of nb samples
// ---------------------------------------------------------------------------------------------
template <typename T, bool W_LDS, bool BUF_GLOBAL>
__global__ void __launch_bounds__(NT_RNN) k_rnn_fwd(RnnShape rs, int nb, const T* x, const T* h0, const T* c0,
                                                    const float* packed_in, const T* bias_in,
                                                    const float* packed_hid, const T* bias_hid,
                                                    T* out, T* hT, T* cT, float* reserve, float* ws, const int* lens) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  DevExec ex;
  const int b0 = blockIdx.x * nb;
  const int n = tmin(nb, rs.B - b0);
  const int H = rs.H, GH = rs.G * rs.H, bs = rs.bs;
  float* p = smem;
  float* hbuf = p; p += (size_t)nb * H;
  float* cbuf = p; p += (size_t)nb * H;
  float* gin = p; p += (size_t)nb * GH;
  float *bufA, *bufB;
  if (BUF_GLOBAL) {
    bufA = ws + (size_t)blockIdx.x * 2 * nb * bs; bufB = bufA + (size_t)nb * bs;
  } else {
    bufA = p; p += (size_t)nb * bs; bufB = p; p += (size_t)nb * bs;
  }
  const float* Win = packed_in;
  const float* Whid = packed_hid;
  if (W_LDS) {
    copy_to_lds(p, packed_in, rs.in_s.wtotal); Win = p; p += rs.in_s.wtotal;
    copy_to_lds(p, packed_hid, rs.hid_s.wtotal); Whid = p; p += rs.hid_s.wtotal;
    __syncthreads();
  }
  rnn_fwd_body<DevExec, T>(ex, rs, b0, n, x, h0, c0, Win, rs.has_bias_in ? bias_in : nullptr, Whid,
                           rs.has_bias_hid ? bias_hid : nullptr, out, hT, cT, reserve, bufA, bufB, hbuf, cbuf, gin, lens);
}

template <typename T, bool W_LDS, bool BUF_GLOBAL>
__global__ void __launch_bounds__(NT_RNN) k_rnn_bwd(RnnShape rs, int nb, const T* out, const T* h0, const T* c0,
                                                    const float* packed_hid, const float* reserve,
                                                    const T* d_out, const T* d_hT, const T* d_cT,
                                                    float* dg_in, float* dg_hid, T* d_h0, T* d_c0, float* ws,
                                                    float* dstate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  DevExec ex;
  const int b0 = blockIdx.x * nb;
  const int n = tmin(nb, rs.B - b0);
  const int H = rs.H, bs = rs.bs;
  float* p = smem;
  float* dh = p; p += (size_t)nb * H;
  float* dc = p; p += (size_t)nb * H;
  float* dhd = p; p += (size_t)nb * H;
  float *bufA, *bufB;
  if (BUF_GLOBAL) {
    bufA = ws + (size_t)blockIdx.x * 2 * nb * bs; bufB = bufA + (size_t)nb * bs;
  } else {
    bufA = p; p += (size_t)nb * bs; bufB = p; p += (size_t)nb * bs;
  }
  const float* Wt = packed_hid + rs.hid_s.wtotal;
  if (W_LDS) { copy_to_lds(p, Wt, rs.hid_s.wtotal); Wt = p; __syncthreads(); }
  rnn_bwd_body<DevExec, T>(ex, rs, b0, n, out, h0, c0, Wt, reserve, d_out, d_hT, d_cT, dg_in, dg_hid, d_h0, d_c0,
                           bufA, bufB, dh, dc, dhd, dstate);
}

// ---------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------
static constexpr size_t LDS_LIMIT = 160 * 1024;

template <class K>
static int set_lds(K kernel, size_t bytes) {
  return ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), bytes);
}

static int check_launch() { return hipGetLastError() == hipSuccess ? TTRNN_OK : TTRNN_ERR_LAUNCH; }

int launch_pack(const TtShape& s, const void* const* cores, const int64_t* strides, int dtype, float* packed,
                hipStream_t stream) {
  PackArgs a;
  int maxn = 1;
  for (int k = 0; k < s.d; ++k) {
    a.core[k] = cores[k];
    for (int q = 0; q < 4; ++q) a.st[4 * k + q] = strides[4 * k + q];
    if (s.K[k] * s.M[k] > maxn) maxn = s.K[k] * s.M[k];
  }
  dim3 grid((maxn + 255) / 256, s.d);
  if (dtype == TTRNN_F32) hipLaunchKernelGGL(k_pack_cores<float>, grid, dim3(256), 0, stream, s, a, packed);
  else hipLaunchKernelGGL(k_pack_cores<bf16_t>, grid, dim3(256), 0, stream, s, a, packed);
  return check_launch();
}

int launch_pack2(const TtShape& sa, const void* const* cores_a, const int64_t* strides_a, float* packed_a,
                 const TtShape& sb, const void* const* cores_b, const int64_t* strides_b, float* packed_b, int dtype,
                 hipStream_t stream) {
  PackArgs aa, ab;
  int maxn = 1;
  for (int k = 0; k < sa.d; ++k) {
    aa.core[k] = cores_a[k];
    for (int q = 0; q < 4; ++q) aa.st[4 * k + q] = strides_a[4 * k + q];
    if (sa.K[k] * sa.M[k] > maxn) maxn = sa.K[k] * sa.M[k];
  }
  for (int k = 0; k < sb.d; ++k) {
    ab.core[k] = cores_b[k];
    for (int q = 0; q < 4; ++q) ab.st[4 * k + q] = strides_b[4 * k + q];
    if (sb.K[k] * sb.M[k] > maxn) maxn = sb.K[k] * sb.M[k];
  }
  dim3 grid((maxn + 255) / 256, sa.d + sb.d);
  if (dtype == TTRNN_F32)
    hipLaunchKernelGGL(k_pack_cores2<float>, grid, dim3(256), 0, stream, sa, aa, packed_a, sb, ab, packed_b);
  else
    hipLaunchKernelGGL(k_pack_cores2<bf16_t>, grid, dim3(256), 0, stream, sa, aa, packed_a, sb, ab, packed_b);
  return check_launch();
}

int launch_unpack(const TtShape& s, const float* packed_grad, void* const* grads, const int64_t* strides, int dtype,
                  hipStream_t stream) {
  PackArgs a;
  int maxn = 1;
  for (int k = 0; k < s.d; ++k) {
    a.grad[k] = grads[k];
    for (int q = 0; q < 4; ++q) a.st[4 * k + q] = strides[4 * k + q];
    if (s.K[k] * s.M[k] > maxn) maxn = s.K[k] * s.M[k];
  }
  dim3 grid((maxn + 255) / 256, s.d);
  if (dtype == TTRNN_F32) hipLaunchKernelGGL(k_unpack_core_grads<float>, grid, dim3(256), 0, stream, s, a, packed_grad);
  else hipLaunchKernelGGL(k_unpack_core_grads<bf16_t>, grid, dim3(256), 0, stream, s, a, packed_grad);
  return check_launch();
}

// ---- TTLinear plans ---------------------------------------------------------------------------
LinPlan plan_ttlinear_fwd(const TtShape& s, int64_t n_rows) {
  LinPlan p{};
  p.bs = (s.maxbuf + 3) & ~3;
  int nb = (4096 + p.bs - 1) / p.bs;
  if (nb < 1) nb = 1;
  if (nb > 16) nb = 16;
  if (n_rows < nb) nb = n_rows > 0 ? (int)n_rows : 1;
  const size_t wbytes = (size_t)s.wtotal * 4;
  // shrink the tile until the ping-pong buffers fit LDS; else spill them to global
  while (nb > 1 && (size_t)2 * nb * p.bs * 4 > LDS_LIMIT) nb >>= 1;
  p.nb = nb;
  const size_t bufbytes = (size_t)2 * nb * p.bs * 4;
  p.buf_global = bufbytes > LDS_LIMIT;
  size_t lds = p.buf_global ? 0 : bufbytes;
  p.w_lds = lds + wbytes <= LDS_LIMIT;
  if (p.w_lds) lds += wbytes;
  p.lds_bytes = lds;
  const int64_t ntiles = (n_rows + nb - 1) / nb;
  p.grid = (int)(ntiles < 1 ? 1 : (ntiles > 2048 ? 2048 : ntiles));
  p.ws_bytes = p.buf_global ? (size_t)p.grid * bufbytes : 0;
  return p;
}

LinPlan plan_ttlinear_bwd(const TtShape& s, int64_t n_rows, bool fixed_order) {
  LinPlan p{};
  p.bs = (s.maxbuf + 3) & ~3;
  p.ss = stash_floats(s);
  p.nb = 1;
  const size_t per = ((size_t)2 * p.bs + p.ss) * 4;
  const size_t acc = ((size_t)s.wtotal + s.out_size) * 4;
  p.buf_global = per > LDS_LIMIT;
  // a sample too large for LDS as a whole (a classifier head 1024 -> 256 with rank 32: 266 KB): keep at least the two
  // ping-pong buffers of the gradient chain on chip (128 KB) and only the stash of stage inputs in the workspace
  p.buf_mixed = p.buf_global && (size_t)2 * p.bs * 4 <= LDS_LIMIT - 4096;
  size_t lds = p.buf_global ? (p.buf_mixed ? (size_t)2 * p.bs * 4 : 0) : per;
  if (!p.buf_global) {
    // more rows per tile amortise the per-stage barriers when a sample is small — as long as two tiles per CU remain (a
    // classifier head sees B rows: 128 rows in tiles of 8 ran on 16 of the 256 CUs)
    while (p.nb < 8 && (size_t)(p.nb * 2) * per + acc <= LDS_LIMIT / 2 && (int64_t)(p.nb * 2) <= n_rows &&
           (size_t)(p.nb * 2) * p.bs < 8192 && n_rows / (p.nb * 2) >= 512)
      p.nb *= 2;
    lds = (size_t)p.nb * per;
  }
  p.acc_lds = lds + acc <= LDS_LIMIT;
  if (p.acc_lds) lds += acc;
  p.w_lds = false;
  p.lds_bytes = lds;
  const int64_t ntiles = (n_rows + p.nb - 1) / p.nb;
  p.grid = (int)(ntiles < 1 ? 1 : (ntiles > 1024 ? 1024 : ntiles));
  p.ws_bytes = p.buf_global ? (size_t)p.grid * p.nb * per : 0;
  // accumulators that do not fit LDS: one global slab per workgroup (at most 256 workgroups then, each walking several
  // tiles) as long as the slabs stay within 256 MB; otherwise atomics
  p.acc_slab = false;
  p.acc_fixed = false;
  p.slab_off = 0;
  if (p.acc_lds && fixed_order && p.grid > 1) {
    // the caller wants repeatable sums (the pull-back of a dense weight gradient onto the cores: `in` rows, one workgroup each):
    // LDS accumulators as before, flushed into a slab per workgroup instead of through atomics.  At most 256 workgroups, each
    // walking several tiles (the kernel strides its tiles by gridDim.x), so that the slabs stay small whatever the shape: round 4
    // took this branch only while grid x acc fit 64 MB, and d = 4, r = 16 at H >= 768 (768 workgroups x 100 KB) fell back to
    // atomics — four grid shapes whose hidden-core gradients differed from run to run
    if (p.grid > 256) p.grid = 256;
    p.ws_bytes = p.buf_global ? (size_t)p.grid * p.nb * per : 0;
    p.acc_fixed = true;
    p.slab_off = (p.ws_bytes + 255) & ~(size_t)255;
    p.ws_bytes = p.slab_off + (size_t)p.grid * acc;
  }
  if (!p.acc_lds) {
    const int g = p.grid > 256 ? 256 : p.grid;
    if ((size_t)g * acc <= ((size_t)256 << 20)) {
      p.acc_slab = true;
      p.grid = g;
      p.ws_bytes = p.buf_global ? (size_t)p.grid * p.nb * per : 0;
      p.slab_off = (p.ws_bytes + 255) & ~(size_t)255;
      p.ws_bytes = p.slab_off + (size_t)g * acc;
    }
  }
  return p;
}

template <typename T>
static int launch_lin_fwd_t(const TtShape& s, const LinPlan& p, int64_t n_rows, const float* packed, const void* bias,
                            const void* x, void* y, void* ws, hipStream_t stream, int ilv_h, int ilv_mode, int epi, float* aux) {
#define TT_LAUNCH(WL, BG)                                                                                          \
  do {                                                                                                             \
    auto kern = k_ttlinear_fwd<T, WL, BG>;                                                                         \
    if (set_lds(kern, p.lds_bytes) != TTRNN_OK) return TTRNN_ERR_LAUNCH;                                           \
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(NT_LIN), p.lds_bytes, stream, s, n_rows, p.nb, p.bs, packed,       \
                       (const T*)bias, (const T*)x, (T*)y, (float*)ws, ilv_h, ilv_mode, epi, aux);                 \
  } while (0)
  if (p.w_lds && !p.buf_global) TT_LAUNCH(true, false);
  else if (!p.w_lds && !p.buf_global) TT_LAUNCH(false, false);
  else if (p.w_lds && p.buf_global) TT_LAUNCH(true, true);
  else TT_LAUNCH(false, true);
#undef TT_LAUNCH
  return check_launch();
}

int launch_ttlinear_fwd(const TtShape& s, const LinPlan& p, int dtype, int64_t n_rows, const float* packed,
                        const void* bias, const void* x, void* y, void* ws, hipStream_t stream, int ilv_h,
                        int ilv_mode, int epi, float* aux) {
  if (n_rows == 0) return TTRNN_OK;
  if (epi != 0 && ilv_h != 0) return TTRNN_ERR_UNSUPPORTED;      // the in-kernel epilogue works on plain rows
  return dtype == TTRNN_F32 ? launch_lin_fwd_t<float>(s, p, n_rows, packed, bias, x, y, ws, stream, ilv_h, ilv_mode, epi, aux)
                            : launch_lin_fwd_t<bf16_t>(s, p, n_rows, packed, bias, x, y, ws, stream, ilv_h, ilv_mode, epi, aux);
}

template <typename T, typename TDY>
static int launch_lin_bwd_t(const TtShape& s, const LinPlan& p, int64_t n_rows, const float* packed, const void* x,
                            const void* dy, void* dx, float* d_packed, float* d_bias, void* ws, hipStream_t stream) {
  float* slabs = (p.acc_slab || p.acc_fixed) ? (float*)((char*)ws + p.slab_off) : nullptr;
#define TT_LAUNCH(BG, AL)                                                                                          \
  do {                                                                                                             \
    auto kern = k_ttlinear_bwd<T, TDY, BG, AL>;                                                                         \
    if (set_lds(kern, p.lds_bytes) != TTRNN_OK) return TTRNN_ERR_LAUNCH;                                           \
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(NT_LIN), p.lds_bytes, stream, s, n_rows, p.nb, p.bs, p.ss, packed, \
                       (const T*)x, (const TDY*)dy, (T*)dx, d_packed, d_bias, (float*)ws, slabs, p.buf_mixed ? 1 : 0); \
  } while (0)
  const bool slab = p.acc_slab && (d_packed || d_bias) && ws;
  const bool fixed = p.acc_fixed && p.acc_lds && (d_packed || d_bias) && ws;
  if (!p.buf_global && fixed) TT_LAUNCH(false, 3);
  else if (p.buf_global && fixed) TT_LAUNCH(true, 3);
  else if (!p.buf_global && p.acc_lds) TT_LAUNCH(false, 1);
  else if (!p.buf_global && slab) TT_LAUNCH(false, 2);
  else if (!p.buf_global) TT_LAUNCH(false, 0);
  else if (p.acc_lds) TT_LAUNCH(true, 1);
  else if (slab) TT_LAUNCH(true, 2);
  else TT_LAUNCH(true, 0);
#undef TT_LAUNCH
  if ((slab && !p.acc_lds) || fixed) {
    const int per = s.wtotal + s.out_size;
    hipLaunchKernelGGL(k_slab_reduce, dim3((per + 255) / 256), dim3(256), 0, stream, (const float*)slabs, p.grid, s.wtotal,
                       s.out_size, d_packed, d_bias);
  }
  return check_launch();
}

int launch_ttlinear_bwd(const TtShape& s, const LinPlan& p, int dtype, int dy_dtype, int64_t n_rows,
                        const float* packed, const void* x, const void* dy, void* dx, float* d_packed, float* d_bias,
                        void* ws, hipStream_t stream) {
  if (n_rows == 0) return TTRNN_OK;
  if (dtype == TTRNN_F32)
    return dy_dtype == TTRNN_F32
               ? launch_lin_bwd_t<float, float>(s, p, n_rows, packed, x, dy, dx, d_packed, d_bias, ws, stream)
               : launch_lin_bwd_t<float, bf16_t>(s, p, n_rows, packed, x, dy, dx, d_packed, d_bias, ws, stream);
  return dy_dtype == TTRNN_F32
             ? launch_lin_bwd_t<bf16_t, float>(s, p, n_rows, packed, x, dy, dx, d_packed, d_bias, ws, stream)
             : launch_lin_bwd_t<bf16_t, bf16_t>(s, p, n_rows, packed, x, dy, dx, d_packed, d_bias, ws, stream);
}

// ---- recurrent plans --------------------------------------------------------------------------
RnnPlan plan_rnn_generic(const RnnShape& rs, bool backward) {
  RnnPlan p{};
  p.nb = 1;
  const size_t state = backward ? (size_t)3 * rs.H * 4 : ((size_t)2 * rs.H + (size_t)rs.G * rs.H) * 4;
  const size_t bufs = (size_t)2 * rs.bs * 4;
  const size_t wbytes = backward ? (size_t)rs.hid_s.wtotal * 4 : ((size_t)rs.in_s.wtotal + rs.hid_s.wtotal) * 4;
  p.buf_global = state + bufs > LDS_LIMIT;
  size_t lds = state + (p.buf_global ? 0 : bufs);
  p.w_lds = lds + wbytes <= LDS_LIMIT;
  if (p.w_lds) lds += wbytes;
  p.lds_bytes = lds;
  p.grid = (rs.B + p.nb - 1) / p.nb;
  if (p.grid < 1) p.grid = 1;
  p.ws_bytes = p.buf_global ? (size_t)p.grid * p.nb * bufs : 0;
  return p;
}

template <typename T>
static int launch_rnn_fwd_t(const RnnShape& rs, const RnnPlan& p, const void* x, const void* h0, const void* c0,
                            const float* packed_in, const void* bias_in, const float* packed_hid, const void* bias_hid,
                            void* out, void* hT, void* cT, float* reserve, void* ws, hipStream_t stream, const int* lens) {
#define TT_LAUNCH(WL, BG)                                                                                          \
  do {                                                                                                             \
    auto kern = k_rnn_fwd<T, WL, BG>;                                                                              \
    if (set_lds(kern, p.lds_bytes) != TTRNN_OK) return TTRNN_ERR_LAUNCH;                                           \
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(NT_RNN), p.lds_bytes, stream, rs, p.nb, (const T*)x, (const T*)h0, \
                       (const T*)c0, packed_in, (const T*)bias_in, packed_hid, (const T*)bias_hid, (T*)out,        \
                       (T*)hT, (T*)cT, reserve, (float*)ws, lens);                                                 \
  } while (0)
  if (p.w_lds && !p.buf_global) TT_LAUNCH(true, false);
  else if (!p.w_lds && !p.buf_global) TT_LAUNCH(false, false);
  else if (p.w_lds && p.buf_global) TT_LAUNCH(true, true);
  else TT_LAUNCH(false, true);
#undef TT_LAUNCH
  return check_launch();
}

int launch_rnn_fwd_generic(const RnnShape& rs, const RnnPlan& p, int dtype, const void* x, const void* h0,
                           const void* c0, const float* packed_in, const void* bias_in, const float* packed_hid,
                           const void* bias_hid, void* out, void* hT, void* cT, float* reserve, void* ws,
                           hipStream_t stream, const int* lens) {
  return dtype == TTRNN_F32
             ? launch_rnn_fwd_t<float>(rs, p, x, h0, c0, packed_in, bias_in, packed_hid, bias_hid, out, hT, cT, reserve, ws, stream, lens)
             : launch_rnn_fwd_t<bf16_t>(rs, p, x, h0, c0, packed_in, bias_in, packed_hid, bias_hid, out, hT, cT, reserve, ws, stream, lens);
}

template <typename T>
static int launch_rnn_bwd_t(const RnnShape& rs, const RnnPlan& p, const void* out, const void* h0, const void* c0,
                            const float* packed_hid, const float* reserve, const void* d_out, const void* d_hT,
                            const void* d_cT, float* dg_in, float* dg_hid, void* d_h0, void* d_c0, void* ws,
                            hipStream_t stream, float* dstate) {
#define TT_LAUNCH(WL, BG)                                                                                          \
  do {                                                                                                             \
    auto kern = k_rnn_bwd<T, WL, BG>;                                                                              \
    if (set_lds(kern, p.lds_bytes) != TTRNN_OK) return TTRNN_ERR_LAUNCH;                                           \
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(NT_RNN), p.lds_bytes, stream, rs, p.nb, (const T*)out,             \
                       (const T*)h0, (const T*)c0, packed_hid, reserve, (const T*)d_out, (const T*)d_hT,           \
                       (const T*)d_cT, dg_in, dg_hid, (T*)d_h0, (T*)d_c0, (float*)ws, dstate);                     \
  } while (0)
  if (p.w_lds && !p.buf_global) TT_LAUNCH(true, false);
  else if (!p.w_lds && !p.buf_global) TT_LAUNCH(false, false);
  else if (p.w_lds && p.buf_global) TT_LAUNCH(true, true);
  else TT_LAUNCH(false, true);
#undef TT_LAUNCH
  return check_launch();
}

int launch_rnn_bwd_generic(const RnnShape& rs, const RnnPlan& p, int dtype, const void* out, const void* h0,
                           const void* c0, const float* packed_hid, const float* reserve, const void* d_out,
                           const void* d_hT, const void* d_cT, float* dg_in, float* dg_hid, void* d_h0, void* d_c0,
                           void* ws, hipStream_t stream, float* dstate) {
  return dtype == TTRNN_F32
             ? launch_rnn_bwd_t<float>(rs, p, out, h0, c0, packed_hid, reserve, d_out, d_hT, d_cT, dg_in, dg_hid, d_h0, d_c0, ws, stream, dstate)
             : launch_rnn_bwd_t<bf16_t>(rs, p, out, h0, c0, packed_hid, reserve, d_out, d_hT, d_cT, dg_in, dg_hid, d_h0, d_c0, ws, stream, dstate);
}

}  // namespace ttrnn
