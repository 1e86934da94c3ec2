// TEST INFRASTRUCTURE ONLY — the serial host executor of hostemu.cpp plus one entry point that drives rnn_fwd_body with
// per-sample sequence lengths (include/ttrnn.h, TTRNN_HAS_VARLEN).  tests/test_varlen_host.py compiles it into
// tests/hostemu/libttrnn_hostemu_varlen.so and runs the UNCHANGED rnn_bwd_body (hostemu_rnn_backward) on the frozen records the
// forward leaves: the design claim that no reverse kernel has to know about lengths, checked where no GPU exists.
#include "hostemu.cpp"

extern "C" {

// lens: [B] on the host.  Tiles of nb samples, so that a tile mixes lengths and the last tile may be partial.
int hostemu_rnn_forward_varlen(const ttrnn_rnn_desc* desc, const int32_t* lens, const float* x, const float* h0, const float* c0,
                               const float* packed_in, const float* bias_in, const float* packed_hid, const float* bias_hid,
                               float* out, float* hT, float* cT, float* reserve, int nb, int nthr) {
  RnnShape rs;
  int st = rnn_shape_init(&rs, desc);
  if (st != TTRNN_OK) return st;
  std::vector<float> A((size_t)nb * rs.bs), B((size_t)nb * rs.bs), hb((size_t)nb * rs.H), cb((size_t)nb * rs.H),
      gin((size_t)nb * rs.G * rs.H);
  std::vector<int> l(lens, lens + rs.B);
  HostExec ex{nthr};
  for (int b0 = 0; b0 < rs.B; b0 += nb) {
    const int n = tmin(nb, rs.B - b0);
    rnn_fwd_body<HostExec, float>(ex, rs, b0, n, x, h0, c0, packed_in, rs.has_bias_in ? bias_in : nullptr, packed_hid,
                                  rs.has_bias_hid ? bias_hid : nullptr, out, hT, cT, reserve, A.data(), B.data(), hb.data(),
                                  cb.data(), gin.data(), l.data());
  }
  return 0;
}

}  // extern "C"
