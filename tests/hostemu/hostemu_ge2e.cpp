// Serial host executor for the GE2E phase bodies of tensorized-rnn_amd/csrc/ttrnn_ge2e.h: the arithmetic of
// ttrnn_fast_ge2e.hip's four kernels, workgroup after workgroup and thread after thread, on the CPU.  Test infrastructure only
// (tests/test_ge2e_fused_host.py builds it with g++); with -DHOSTEMU_GE2E_MAIN it is a stand-alone program over the same
// bodies, which is the form a sanitizer build takes (g++ -fsanitize=address,undefined -DHOSTEMU_GE2E_MAIN ...).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ttrnn_ge2e.h"

using namespace ttrnn;

namespace {
struct HostExec {
  int nthr;
  template <class F>
  void par(F f) {
    for (int t = 0; t < nthr; ++t) f(t, nthr);
  }
};
}  // namespace

extern "C" {

long hostemu_ge2e_workspace_floats(const ttrnn_ge2e_desc* desc) {
  Ge2ePlan p;
  if (ge2e_plan_init(&p, desc) != TTRNN_OK) return 0;
  return (long)p.total;
}

// forward (phases 1-3) + backward (phase 4) as the library's two calls make them; ws: hostemu_ge2e_workspace_floats floats,
// filled with NaN here first so that a read of anything a phase did not write shows in the results
int hostemu_ge2e(const ttrnn_ge2e_desc* desc, const float* E, const float* A, const float* w, const float* b, const float* g,
                 float* loss, float* sim_out, int need_grad, float* dE, float* dw, float* db, float* ws) {
  Ge2ePlan p;
  const int st = ge2e_plan_init(&p, desc);
  if (st != TTRNN_OK) return st;
  const int T = TTRNN_GE2E_THREADS;
  HostExec ex{T};
  for (size_t i = 0; i < p.total; ++i) ws[i] = NAN;
  std::vector<float> lds(p.lds_rows + p.lds_cgrad + p.lds_dE + (size_t)p.D + TTRNN_GE2E_RED, NAN);
  const bool train = p.Ue == 0;
  for (int j = 0; j < p.S; ++j) ge2e_centroid_body(ex, p, j, train ? E : A, train ? p.U : p.Ue, ws, lds.data(), T);
  for (int wg = 0; wg < p.nrow_wg; ++wg) ge2e_rows_body(ex, p, wg, E, w, b, sim_out, need_grad, ws, lds.data(), T);
  ge2e_finalize_body(ex, p, loss, need_grad, ws, lds.data(), T);
  if (need_grad && train)
  {
    for (int kj = 0; kj < p.K * p.S; ++kj) ge2e_cgrad_body(ex, p, kj, E, ws, lds.data(), T);
    for (int s = 0; s < p.S; ++s) ge2e_asum_body(ex, p, s, E, ws, lds.data());
  }
  if (dE || dw || db) {
    const int grid = dE ? p.S * p.UTn : 1;
    for (int wg = 0; wg < grid; ++wg) ge2e_dE_body(ex, p, wg, E, w, g, dE, dw, db, ws, lds.data());
  }
  return TTRNN_OK;
}

}  // extern "C"

#ifdef HOSTEMU_GE2E_MAIN
// every shape class the kernels distinguish (tails in D, one class, U = 2, a speaker past a 64 tile, the enrollment form) on
// seeded inputs; prints the losses, exits non-zero on a non-finite result
int main() {
  const int shapes[][4] = {{1, 2, 8, 0}, {5, 2, 32, 0}, {3, 7, 30, 0}, {65, 3, 256, 0}, {16, 32, 256, 0}, {7, 3, 36, 2}, {300, 2, 5, 0}};
  unsigned seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f - 0.5f; };
  for (const auto& sh : shapes) {
    ttrnn_ge2e_desc d{sh[0], sh[1], sh[2], sh[3]};
    const size_t n = (size_t)d.S * d.U * d.D, na = (size_t)d.S * d.U_enroll * d.D;
    std::vector<float> E(n), A(na), dE(n), sim((size_t)d.S * d.U * d.S), ws(hostemu_ge2e_workspace_floats(&d));
    for (auto& v : E) v = rnd();
    for (auto& v : A) v = rnd();
    float w = 10.f, b = -5.f, g = 3.5f, loss = 0.f, dw = 0.f, db = 0.f;
    const int st = hostemu_ge2e(&d, E.data(), na ? A.data() : nullptr, &w, &b, &g, &loss, sim.data(), 1, dE.data(), &dw, &db, ws.data());
    float amax = 0.f;      // a sum, so that one NaN shows
    for (float v : dE) amax += fabsf(v);
    std::printf("S %d U %d D %d Ue %d: status %d loss %.6f d_w %.3e d_b %.3e sum|d_E| %.3e\n", d.S, d.U, d.D, d.U_enroll, st, loss, dw,
                db, amax);
    if (st != TTRNN_OK || !(loss == loss) || !(amax == amax) || !(dw == dw)) return 1;
  }
  return 0;
}
#endif
