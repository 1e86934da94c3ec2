// TEST INFRASTRUCTURE ONLY — serial host executor for the kernel bodies in
// tensorized-rnn_amd/csrc/ttrnn_core.h.  It lets `pytest -m "not gpu"` check the index arithmetic
// of the generic kernels (packing, chain stages, cell updates, BPTT, weight gradients) against the
// golden fixtures in the build container, where no GPU exists.  It is compiled by
// tests/test_hostemu.py into tests/hostemu/libttrnn_hostemu.so and is never loaded by the product.
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ttrnn_core.h"

using namespace ttrnn;

struct HostExec {
  int nthr;
  template <class F>
  void par(F f) {
    for (int t = 0; t < nthr; ++t) f(t, nthr);
  }
};

struct AddHost {
  void operator()(float* p, float v) const { *p += v; }
};

extern "C" {

int64_t hostemu_packed_elems(const ttrnn_ttm* w) {
  TtShape s;
  if (tt_shape_init(&s, w) != TTRNN_OK) return -1;
  return 2 * (int64_t)s.wtotal;
}

int hostemu_pack(const ttrnn_ttm* w, const float* const* cores, const int64_t* strides, float* packed) {
  TtShape s;
  int st = tt_shape_init(&s, w);
  if (st != TTRNN_OK) return st;
  for (int k = 0; k < s.d; ++k)
    for (int t = 0; t < 7; ++t) pack_core_elems<float>(t, 7, s, k, cores[k], strides + 4 * k, packed);
  return 0;
}

int hostemu_unpack(const ttrnn_ttm* w, const float* packed_grad, float* const* grads, const int64_t* strides) {
  TtShape s;
  int st = tt_shape_init(&s, w);
  if (st != TTRNN_OK) return st;
  for (int k = 0; k < s.d; ++k)
    for (int t = 0; t < 5; ++t) unpack_core_grad_elems<float>(t, 5, s, k, packed_grad, grads[k], strides + 4 * k);
  return 0;
}

// epi / aux: the row-wise epilogue inside the tile (TTRNN_EPI_*, 0 = none) and where it leaves the log-sum-exp / L2 norm (may be NULL)
int hostemu_ttlinear_forward(const ttrnn_ttm* w, int64_t n_rows, const float* packed, const float* bias,
                             const float* x, float* y, int nb, int nthr, int epi, float* aux) {
  TtShape s;
  int st = tt_shape_init(&s, w);
  if (st != TTRNN_OK) return st;
  const int bs = (s.maxbuf + 3) & ~3;
  std::vector<float> A((size_t)nb * bs), B((size_t)nb * bs);
  HostExec ex{nthr};
  for (int64_t n0 = 0; n0 < n_rows; n0 += nb) {
    const int n = (int)tmin<int64_t>(nb, n_rows - n0);
    ttlinear_fwd_tile<HostExec, float>(ex, s, packed, bias, x, y, n0, n, A.data(), B.data(), bs, 0, 0, epi, aux);
  }
  return 0;
}

int hostemu_ttlinear_backward(const ttrnn_ttm* w, int64_t n_rows, const float* packed, const float* x,
                              const float* dy, float* dx, float* d_packed, float* d_bias, int nb, int nthr) {
  TtShape s;
  int st = tt_shape_init(&s, w);
  if (st != TTRNN_OK) return st;
  const int bs = (s.maxbuf + 3) & ~3;
  const int ss = stash_floats(s);
  std::vector<float> A((size_t)nb * bs), B((size_t)nb * bs), S((size_t)nb * ss);
  HostExec ex{nthr};
  for (int64_t n0 = 0; n0 < n_rows; n0 += nb) {
    const int n = (int)tmin<int64_t>(nb, n_rows - n0);
    ttlinear_bwd_tile<HostExec, float, float>(ex, s, packed, packed + s.wtotal, x, dy, dx, d_packed, d_bias, n0, n,
                                              S.data(), ss, A.data(), B.data(), bs, AddHost());
  }
  return 0;
}

int hostemu_rnn_forward(const ttrnn_rnn_desc* desc, const float* x, const float* h0, const float* c0,
                        const float* packed_in, const float* bias_in, const float* packed_hid,
                        const float* bias_hid, float* out, float* hT, float* cT, float* reserve, int nb, int nthr) {
  RnnShape rs;
  int st = rnn_shape_init(&rs, desc);
  if (st != TTRNN_OK) return st;
  std::vector<float> A((size_t)nb * rs.bs), B((size_t)nb * rs.bs), hb((size_t)nb * rs.H), cb((size_t)nb * rs.H),
      gin((size_t)nb * rs.G * rs.H);
  HostExec ex{nthr};
  for (int b0 = 0; b0 < rs.B; b0 += nb) {
    const int n = tmin(nb, rs.B - b0);
    rnn_fwd_body<HostExec, float>(ex, rs, b0, n, x, h0, c0, packed_in, rs.has_bias_in ? bias_in : nullptr,
                                  packed_hid, rs.has_bias_hid ? bias_hid : nullptr, out, hT, cT, reserve, A.data(),
                                  B.data(), hb.data(), cb.data(), gin.data());
  }
  return 0;
}

int hostemu_rnn_backward(const ttrnn_rnn_desc* desc, const float* out, const float* h0, const float* c0,
                         const float* packed_hid, const float* reserve, const float* d_out, const float* d_hT,
                         const float* d_cT, float* dg_in, float* dg_hid, float* d_h0, float* d_c0, int nb, int nthr) {
  RnnShape rs;
  int st = rnn_shape_init(&rs, desc);
  if (st != TTRNN_OK) return st;
  std::vector<float> A((size_t)nb * rs.bs), B((size_t)nb * rs.bs), dh((size_t)nb * rs.H), dc((size_t)nb * rs.H),
      dhd((size_t)nb * rs.H);
  HostExec ex{nthr};
  for (int b0 = 0; b0 < rs.B; b0 += nb) {
    const int n = tmin(nb, rs.B - b0);
    rnn_bwd_body<HostExec, float>(ex, rs, b0, n, out, h0, c0, packed_hid + rs.hid_s.wtotal, reserve, d_out, d_hT,
                                  d_cT, dg_in, dg_hid, d_h0, d_c0, A.data(), B.data(), dh.data(), dc.data(),
                                  dhd.data());
  }
  return 0;
}

}  // extern "C"
