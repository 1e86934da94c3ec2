// ttrnn_ge2e.h — plan and phase bodies of the fused GE2E similarity / softmax loss / gradients (ttrnn_fast_ge2e.hip).
//
// Restates ttrnn_hip/ge2e.py:14-48 (= experiments/speaker_verification/encoder/speaker_encoder.py:93-170 of the reference) for
// embeddings that are NOT assumed normalised.  Four data-dependent phases, one launch each, every body written against the
// executor concept of ttrnn_core.h (`ex.par(f)` = run f for every thread, then barrier), so tests/hostemu/hostemu_ge2e.cpp
// runs the very same arithmetic serially on the CPU:
//   1  centroids   one workgroup per speaker j:  c_j = sum_u src[j,u],  incl_j = normalize(c_j / U)          (src = E or A)
//   2  rows        R rows per workgroup:  raw[row,j] = E[row] . incl_j  (training form, j == s: E[row] . normalize(v),
//                  v = (c_s - E[row]) / (U - 1)),  out = w raw + b,  max-subtracted softmax,  dout = (p - onehot) / N,
//                  per-workgroup partial sums of the loss, of dout . raw (d_w) and of dout (d_b)
//   3  centroid gradients  workgroup (k, j): slab[k][j][:] = sum over the rows of chunk k with s != j of dout[row,j] E[row]
//                  (and tpart[k][j] = the same sum of dout[row,j] raw[row,j] = incl_j . d_incl_j, so that the normalisation
//                  Jacobian needs no reduction over D); workgroup s of a second group: asum[s][:] = sum_u d_v_su, the gradient
//                  through the speaker's exclusive centroids; workgroup 0 sums the row phase's partials in a fixed order
//   4  d_E         workgroup (s, utterance tile): slabs summed in a fixed order, the Jacobians of both normalisations, the
//                  direct term; everything is linear in G = w dout, so w and the upstream gradient g multiply the result once
// Phases 1-3 are the forward call, phase 4 the backward call: four launches for loss plus all gradients.  Every sum is taken
// in an order fixed by the plan alone: no atomics, results repeatable bit for bit.  fp32 VALU arithmetic throughout.  The sums
// whose length is U or a chunk of rows keep their error independent of that length up to the row limit: the centroid sum of
// phase 1 is compensated (over batches of sixteen), the sums of phase 3 are taken per tile of 256 rows from 0 and the tile totals added to the carry.
// The operands are a few hundred KB and L2-resident: what the loops are shaped for is load latency — sixteen independent loads
// are issued before the sixteen dependent FMAs that consume them, and values that every lane needs go through LDS.
#pragma once
#include "ttrnn_core.h"

namespace ttrnn {

#define TTRNN_GE2E_THREADS 256
#define TTRNN_GE2E_EPS 1e-12f          // F.normalize's eps
#define TTRNN_GE2E_MAX_S 2048
#define TTRNN_GE2E_MAX_D 4096
#define TTRNN_GE2E_MAX_ROWS (1 << 22)
#define TTRNN_GE2E_TILE 256            // rows / utterances whose per-row scalars are staged in LDS at a time (phase 3)
#define TTRNN_GE2E_RED (TTRNN_GE2E_THREADS + 17)

struct Ge2ePlan {
  int S, U, D, Ue, N;
  int R;         // rows per workgroup of the row phase
  int P, DC;     // ... whose dot products are split over P threads of DC consecutive components each
  int C;         // threads that share one row's softmax reductions
  int nrow_wg;   // workgroups of the row phase
  int K, CH;     // centroid-gradient phase: K chunks of CH rows
  int UT, UTn;   // d_E phase: utterances per workgroup, tiles per speaker
  // workspace regions (offsets in floats)
  size_t o_csum, o_csumT, o_incl, o_inclT, o_cstat, o_raw, o_dout, o_rstat, o_part, o_scal, o_slab, o_tpart, o_asum, total;
  size_t lds_rows, lds_cgrad, lds_dE;      // floats of LDS per workgroup of phases 2, 3, 4
};

// pure host arithmetic; TTRNN_OK, TTRNN_ERR_BAD_DESC or TTRNN_ERR_UNSUPPORTED
inline int ge2e_plan_init(Ge2ePlan* p, const ttrnn_ge2e_desc* d) {
  if (!p || !d) return TTRNN_ERR_NULL;
  if (d->S < 1 || d->U < 1 || d->D < 1 || d->U_enroll < 0) return TTRNN_ERR_BAD_DESC;
  if (d->U_enroll == 0 && d->U < 2) return TTRNN_ERR_BAD_DESC;
  if (d->S > TTRNN_GE2E_MAX_S || d->D > TTRNN_GE2E_MAX_D) return TTRNN_ERR_UNSUPPORTED;
  if ((int64_t)d->S * d->U > TTRNN_GE2E_MAX_ROWS || (int64_t)d->S * d->U_enroll > TTRNN_GE2E_MAX_ROWS) return TTRNN_ERR_UNSUPPORTED;
  p->S = d->S; p->U = d->U; p->D = d->D; p->Ue = d->U_enroll; p->N = d->S * d->U;
  int R = 32 / p->S;
  if (R > 16) R = 16;
  if (R < 1) R = 1;
  p->R = R;
  int P = TTRNN_GE2E_THREADS / (R * p->S);
  if (P > 16) P = 16;
  if (P < 1) P = 1;
  p->P = P;
  p->DC = (p->D + P - 1) / P;
  p->C = 16;
  p->nrow_wg = (p->N + R - 1) / R;
  int K = (p->N + 31) / 32;
  if (K > 16) K = 16;
  p->CH = (p->N + K - 1) / K;
  p->K = (p->N + p->CH - 1) / p->CH;
  p->UT = p->U < 2 ? p->U : 2;
  p->UTn = (p->U + p->UT - 1) / p->UT;
  const size_t SD = (size_t)p->S * p->D, NS = (size_t)p->N * p->S;
  size_t o = 0;
  p->o_csum = o; o += SD;
  p->o_csumT = o; o += SD;
  p->o_incl = o; o += SD;
  p->o_inclT = o; o += SD;
  p->o_cstat = o; o += 2 * (size_t)p->S;
  p->o_raw = o; o += NS;
  p->o_dout = o; o += NS;
  p->o_rstat = o; o += 2 * (size_t)p->N;
  p->o_part = o; o += 4 * (size_t)p->nrow_wg;
  p->o_scal = o; o += 4;
  p->o_slab = o; o += (size_t)p->K * SD;
  p->o_tpart = o; o += (size_t)p->K * p->S;
  p->o_asum = o; o += SD;
  p->total = o;
  // raw + out + the split dot products' two partials + softmax partials + row max / sum / loss + reduction scratch
  p->lds_rows = 2 * (size_t)R * p->S + 2 * (size_t)R * p->S * P + (size_t)R * p->C + 3 * (size_t)R + 3 * TTRNN_GE2E_RED;
  p->lds_cgrad = 4 * TTRNN_GE2E_TILE + 3 * TTRNN_GE2E_RED;
  p->lds_dE = (size_t)p->UT * p->S + 4 * (size_t)p->UT + 16;
  return TTRNN_OK;
}

// sum of red[0 .. nthr) (one value per thread, written in the caller's preceding par) in a fixed order: 16 strided partial sums,
// then those in sequence.  The result is left in red[nthr + 16]; red has nthr + 17 floats.
template <class Ex>
TT_HD void ge2e_block_sum(Ex& ex, float* red) {
  ex.par([&](int tid, int nthr) {
    if (tid < 16) {
      float a = 0.f;
      for (int i = tid; i < nthr; i += 16) a += red[i];
      red[nthr + tid] = a;
    }
  });
  ex.par([&](int tid, int nthr) {
    if (tid == 0) {
      float a = 0.f;
      for (int i = 0; i < 16; ++i) a += red[nthr + i];
      red[nthr + 16] = a;
    }
  });
}

// the same for three arrays laid out back to back (red, red + TTRNN_GE2E_RED, red + 2 TTRNN_GE2E_RED; nthr = TTRNN_GE2E_THREADS)
template <class Ex>
TT_HD void ge2e_block_sum3(Ex& ex, float* red) {
  ex.par([&](int tid, int nthr) {
    if (tid < 48) {
      float* r = red + (tid / 16) * TTRNN_GE2E_RED;
      float a = 0.f;
      for (int i = tid % 16; i < nthr; i += 16) a += r[i];
      r[nthr + tid % 16] = a;
    }
  });
  ex.par([&](int tid, int nthr) {
    if (tid < 3) {
      float* r = red + tid * TTRNN_GE2E_RED;
      float a = 0.f;
      for (int i = 0; i < 16; ++i) a += r[nthr + i];
      r[nthr + 16] = a;
    }
  });
}

// acc(i, load(i)) for i = n0 .. n1 - 1 in order, sixteen loads in flight at a time (the last batch re-reads element n1 - 1 in
// its idle slots, so every load is unconditional)
template <class L, class A>
TT_HD void ge2e_batch16(int n0, int n1, L load, A acc) {
  for (int i0 = n0; i0 < n1; i0 += 16) {
    float v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = load(i0 + m < n1 ? i0 + m : n1 - 1);
#pragma unroll
    for (int m = 0; m < 16; ++m)
      if (i0 + m < n1) acc(i0 + m, v[m]);
  }
}
// ... with two operands per element
template <class L, class M, class A>
TT_HD void ge2e_batch16x2(int n0, int n1, L load, M load2, A acc) {
  for (int i0 = n0; i0 < n1; i0 += 16) {
    float v[16], x[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = load(i0 + m < n1 ? i0 + m : n1 - 1);
#pragma unroll
    for (int m = 0; m < 16; ++m) x[m] = load2(i0 + m < n1 ? i0 + m : n1 - 1);
#pragma unroll
    for (int m = 0; m < 16; ++m)
      if (i0 + m < n1) acc(v[m], x[m]);
  }
}

// phase 1: workgroup j.  src = E (training form, Usrc = U) or A (enrollment form, Usrc = U_enroll).  lds: D + nthr + 17 floats.
template <class Ex>
TT_HD void ge2e_centroid_body(Ex& ex, const Ge2ePlan& p, int j, const float* src, int Usrc, float* ws, float* lds, int nthr_red) {
  const int D = p.D, S = p.S;
  float* x = lds;
  float* red = lds + D;
  ex.par([&](int tid, int nthr) {
    float nn = 0.f;
    for (int d = tid; d < D; d += nthr) {
      const float* col = src + (size_t)j * Usrc * D + d;
      // sixteen loads in flight, their sum as a tree of depth 4, and the batch totals in a compensated (Kahan) sum: `lost` carries
      // what the running sum rounded away, so the error does not grow with Usrc and the dependent chain is 8 operations per batch
      float c = 0.f, lost = 0.f;
      for (int u0 = 0; u0 < Usrc; u0 += 16) {
        float v[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = col[(size_t)(u0 + m < Usrc ? u0 + m : Usrc - 1) * D];
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = u0 + m < Usrc ? v[m] : 0.f;
#pragma unroll
        for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
          for (int m = 0; m < h; ++m) v[m] += v[m + h];
        const float y = v[0] - lost;
        const float t = c + y;
        lost = (t - c) - y;
        c = t;
      }
      ws[p.o_csum + (size_t)j * D + d] = c;
      ws[p.o_csumT + (size_t)d * S + j] = c;
      const float m = c / (float)Usrc;
      x[d] = m;
      nn += m * m;
    }
    red[tid] = nn;
  });
  ge2e_block_sum(ex, red);
  ex.par([&](int tid, int nthr) {
    const float nrm = sqrtf(red[nthr_red + 16]);
    const float den = fmaxf(nrm, TTRNN_GE2E_EPS);
    for (int d = tid; d < D; d += nthr) {
      const float v = x[d] / den;
      ws[p.o_incl + (size_t)j * D + d] = v;
      ws[p.o_inclT + (size_t)d * S + j] = v;
    }
    if (tid == 0) {
      ws[p.o_cstat + 2 * (size_t)j] = den;
      ws[p.o_cstat + 2 * (size_t)j + 1] = nrm > TTRNN_GE2E_EPS ? 1.f : 0.f;
    }
  });
}

// phase 2: workgroup wg owns rows [wg R, wg R + R).  sim_out (NULL-able) receives out = w raw + b.  lds: p.lds_rows floats.
template <class Ex>
TT_HD void ge2e_rows_body(Ex& ex, const Ge2ePlan& p, int wg, const float* E, const float* wp, const float* bp, float* sim_out,
                          int need_grad, float* ws, float* lds, int nthr_red) {
  const int D = p.D, S = p.S, U = p.U, N = p.N, R = p.R, C = p.C, P = p.P, DC = p.DC;
  const bool train = p.Ue == 0;
  const int r0 = wg * R;
  const int nr = N - r0 < R ? N - r0 : R;
  const int npair = nr * S;
  float* raw = lds;
  float* out = raw + (size_t)R * S;
  float* pa = out + (size_t)R * S;
  float* pb = pa + (size_t)R * S * P;
  float* part = pb + (size_t)R * S * P;
  float* rmax = part + (size_t)R * C;
  float* rsum = rmax + R;
  float* rloss = rsum + R;
  float* red_l = rloss + R;
  float* red_w = red_l + TTRNN_GE2E_RED;
  float* red_b = red_w + TTRNN_GE2E_RED;
  const float w = *wp, b = *bp;
  const float um1 = (float)(U - 1);
  // dot products: thread (c, r, j) — j fastest, so a wave's loads of a centroid component are one contiguous segment — takes the
  // components [c DC, c DC + DC) of E[row] . incl_j, or of E[row] . v and v . v for the row's own speaker
  ex.par([&](int tid, int nthr) {
    for (int q = tid; q < npair * P; q += nthr) {
      const int c = q / npair, pair = q - c * npair;
      const int r = pair / S, j = pair - r * S;
      const int s = (r0 + r) / U;
      const float* er = E + (size_t)(r0 + r) * D;
      const int d0 = c * DC, d1 = d0 + DC < D ? d0 + DC : D;
      float a = 0.f, vv = 0.f;
      if (train && j == s) {
        const float* col = ws + p.o_csumT + s;
        ge2e_batch16x2(d0, d1, [&](int d) { return col[(size_t)d * S]; }, [&](int d) { return er[d]; }, [&](float cs, float x) {
          const float t = (cs - x) / um1;
          a += x * t;
          vv += t * t;
        });
      } else {
        const float* col = ws + p.o_inclT + j;
        ge2e_batch16x2(d0, d1, [&](int d) { return col[(size_t)d * S]; }, [&](int d) { return er[d]; },
                       [&](float v, float x) { a += x * v; });
      }
      pa[q] = a;
      pb[q] = vv;
    }
  });
  ex.par([&](int tid, int nthr) {
    for (int q = tid; q < npair; q += nthr) {
      const int r = q / S, j = q - r * S;
      const int row = r0 + r, s = row / U;
      float val = 0.f, vv = 0.f;
      for (int c = 0; c < P; ++c) {
        val += pa[(size_t)c * npair + q];
        vv += pb[(size_t)c * npair + q];
      }
      if (train && j == s) {      // the speaker against the centroid of its OTHER utterances
        const float nrm = sqrtf(vv);
        const float den = fmaxf(nrm, TTRNN_GE2E_EPS);
        val = val / den;
        ws[p.o_rstat + 2 * (size_t)row] = den;
        ws[p.o_rstat + 2 * (size_t)row + 1] = nrm > TTRNN_GE2E_EPS ? 1.f : 0.f;
      }
      const float o = w * val + b;
      raw[q] = val;
      out[q] = o;
      if (need_grad) ws[p.o_raw + (size_t)row * S + j] = val;
      if (sim_out) sim_out[(size_t)row * S + j] = o;
    }
  });
  // max-subtracted softmax: C threads per row take strided partial maxima / sums, one thread per row folds them in sequence
  ex.par([&](int tid, int nthr) {
    for (int q = tid; q < nr * C; q += nthr) {
      const int r = q / C, k = q - r * C;
      float m = -INFINITY;
      for (int j = k; j < S; j += C) m = fmaxf(m, out[(size_t)r * S + j]);
      part[q] = m;
    }
  });
  ex.par([&](int tid, int nthr) {
    for (int r = tid; r < nr; r += nthr) {
      float m = part[(size_t)r * C];
      for (int k = 1; k < C; ++k) m = fmaxf(m, part[(size_t)r * C + k]);
      rmax[r] = m;
    }
  });
  ex.par([&](int tid, int nthr) {
    for (int q = tid; q < nr * C; q += nthr) {
      const int r = q / C, k = q - r * C;
      float a = 0.f;
      for (int j = k; j < S; j += C) a += expf(out[(size_t)r * S + j] - rmax[r]);
      part[q] = a;
    }
  });
  ex.par([&](int tid, int nthr) {
    for (int r = tid; r < nr; r += nthr) {
      float a = 0.f;
      for (int k = 0; k < C; ++k) a += part[(size_t)r * C + k];
      rsum[r] = a;
      const int s = (r0 + r) / U;
      // log(sum) - (out_s - max): the difference is exact where the true class is the maximum (or near it), so a small loss
      // keeps its own precision, not that of |out|
      rloss[r] = logf(a) - (out[(size_t)r * S + s] - rmax[r]);
    }
  });
  ex.par([&](int tid, int nthr) {
    float aw = 0.f, ab = 0.f;
    for (int q = tid; q < npair; q += nthr) {
      const int r = q / S, j = q - r * S;
      const int row = r0 + r, s = row / U;
      const float pr = expf(out[q] - rmax[r]) / rsum[r];
      const float g = (pr - (j == s ? 1.f : 0.f)) / (float)N;
      if (need_grad) ws[p.o_dout + (size_t)row * S + j] = g;
      aw += g * raw[q];
      ab += g;
    }
    float al = 0.f;
    for (int r = tid; r < nr; r += nthr) al += rloss[r];
    red_l[tid] = al;
    red_w[tid] = aw;
    red_b[tid] = ab;
  });
  ge2e_block_sum3(ex, red_l);
  ex.par([&](int tid, int) {
    if (tid == 0) {
      float* o = ws + p.o_part + 4 * (size_t)wg;
      o[0] = red_l[nthr_red + 16];
      o[1] = red_w[nthr_red + 16];
      o[2] = red_b[nthr_red + 16];
      o[3] = 0.f;
    }
  });
}

// phase 3, workgroup 0: the row phase's partial sums in a fixed order -> loss (mean over the N rows), and the g = 1 values of
// d_w, d_b for the backward call.  scal[3] = 1 when the forward prepared gradients, NaN otherwise: the backward call multiplies
// by it, so gradients asked of a forward-only workspace come out NaN, never stale.  lds: 3 (nthr + 17) floats.
template <class Ex>
TT_HD void ge2e_finalize_body(Ex& ex, const Ge2ePlan& p, float* loss, int need_grad, float* ws, float* lds, int nthr_red) {
  float* red[3] = {lds, lds + TTRNN_GE2E_RED, lds + 2 * TTRNN_GE2E_RED};
  const float* part = ws + p.o_part;
  ex.par([&](int tid, int nthr) {
    float a[3] = {0.f, 0.f, 0.f};
    for (int i = tid; i < p.nrow_wg; i += nthr)
      for (int c = 0; c < 3; ++c) a[c] += part[4 * (size_t)i + c];
    for (int c = 0; c < 3; ++c) red[c][tid] = a[c];
  });
  ge2e_block_sum3(ex, red[0]);
  ex.par([&](int tid, int) {
    if (tid == 0) {
      const float l = red[0][nthr_red + 16] / (float)p.N;
      if (loss) *loss = l;
      float* sc = ws + p.o_scal;
      sc[0] = l;
      sc[1] = red[1][nthr_red + 16];
      sc[2] = red[2][nthr_red + 16];
      sc[3] = need_grad ? 1.f : NAN;
    }
  });
}

// phase 3, workgroup 1 + k S + j (training form only).  The speaker's own rows reach its inclusive centroid through c_j, not
// here: their dout is staged as 0.  lds: TILE + nthr + 17 floats.
template <class Ex>
TT_HD void ge2e_cgrad_body(Ex& ex, const Ge2ePlan& p, int kj, const float* E, float* ws, float* lds, int nthr_red) {
  const int D = p.D, S = p.S, U = p.U, N = p.N;
  const int k = kj / S, j = kj - k * S;
  const int row0 = k * p.CH, row1 = row0 + p.CH < N ? row0 + p.CH : N;
  const float* dout = ws + p.o_dout;
  const float* raw = ws + p.o_raw;
  const int own0 = j * U, own1 = own0 + U;
  float* gl = lds;
  float* red = lds + TTRNN_GE2E_TILE;
  float* slab = ws + p.o_slab + ((size_t)k * S + j) * D;
  for (int t0 = row0; t0 < row1; t0 += TTRNN_GE2E_TILE) {
    const int nt = row1 - t0 < TTRNN_GE2E_TILE ? row1 - t0 : TTRNN_GE2E_TILE;
    ex.par([&](int tid, int nthr) {
      float t = 0.f;
      for (int i = tid; i < nt; i += nthr) {
        const int row = t0 + i;
        const float g = (row < own0 || row >= own1) ? dout[(size_t)row * S + j] : 0.f;
        gl[i] = g;
        t += g * raw[(size_t)row * S + j];
      }
      red[tid] = t0 == row0 ? t : red[tid] + t;
    });
    ex.par([&](int tid, int nthr) {
      for (int d = tid; d < D; d += nthr) {
        const float* col = E + (size_t)t0 * D + d;
        float a = 0.f;
        ge2e_batch16(0, nt, [&](int i) { return col[(size_t)i * D]; }, [&](int i, float v) { a += gl[i] * v; });
        slab[d] = t0 == row0 ? a : slab[d] + a;
      }
    });
  }
  ge2e_block_sum(ex, red);
  ex.par([&](int tid, int) {
    if (tid == 0) ws[p.o_tpart + (size_t)k * S + j] = red[nthr_red + 16];
  });
}

// d(normalize(v) . e)/dv for one component, v = (c - e) / (U - 1): the row's own-centroid term, for upstream gss = dout[row, s]
TT_HD float ge2e_dv(float c, float e, float um1, float den, float fl, float gss, float own) {
  const float ex_ = ((c - e) / um1) / den;
  const float q = gss * e;
  return (fl != 0.f ? (q - ex_ * (gss * own)) / den : q / den) / um1;
}

// phase 3, workgroup 1 + K S + s (training form only): asum[s][d] = sum_u d_v_su[d].  lds: 4 TILE floats.
template <class Ex>
TT_HD void ge2e_asum_body(Ex& ex, const Ge2ePlan& p, int s, const float* E, float* ws, float* lds) {
  const int D = p.D, S = p.S, U = p.U;
  const float um1 = (float)(U - 1);
  float* sc = lds;      // per utterance of the tile: den, flag, dout[row, s], raw[row, s]
  float* asum = ws + p.o_asum + (size_t)s * D;
  for (int u0 = 0; u0 < U; u0 += TTRNN_GE2E_TILE) {
    const int nt = U - u0 < TTRNN_GE2E_TILE ? U - u0 : TTRNN_GE2E_TILE;
    ex.par([&](int tid, int nthr) {
      for (int i = tid; i < nt; i += nthr) {
        const size_t row = (size_t)s * U + u0 + i;
        sc[4 * i] = ws[p.o_rstat + 2 * row];
        sc[4 * i + 1] = ws[p.o_rstat + 2 * row + 1];
        sc[4 * i + 2] = ws[p.o_dout + row * S + s];
        sc[4 * i + 3] = ws[p.o_raw + row * S + s];
      }
    });
    ex.par([&](int tid, int nthr) {
      for (int d = tid; d < D; d += nthr) {
        const float c = ws[p.o_csum + (size_t)s * D + d];
        const float* col = E + ((size_t)s * U + u0) * D + d;
        float a = 0.f;
        ge2e_batch16(0, nt, [&](int i) { return col[(size_t)i * D]; }, [&](int i, float v) {
          const float* q = sc + 4 * i;
          a += ge2e_dv(c, v, um1, q[0], q[1], q[2], q[3]);
        });
        asum[d] = u0 == 0 ? a : asum[d] + a;
      }
    });
  }
}

// phase 4: workgroup wg = s UTn + tile.  gp (NULL = 1): upstream gradient of the loss.  Any of dE, dw, db may be NULL.
// lds: p.lds_dE floats (the tile's dout rows — the own column as 0 in the training form — and its per-row scalars).
template <class Ex>
TT_HD void ge2e_dE_body(Ex& ex, const Ge2ePlan& p, int wg, const float* E, const float* wp, const float* gp, float* dE, float* dw,
                        float* db, const float* ws, float* lds) {
  const int D = p.D, S = p.S, U = p.U;
  const bool train = p.Ue == 0;
  const int s = wg / p.UTn, tile = wg - s * p.UTn;
  const int u0 = tile * p.UT, nu = (u0 + p.UT < U ? u0 + p.UT : U) - u0;
  const float* scal = ws + p.o_scal;
  const float gg = (gp ? *gp : 1.f) * scal[3];
  const float scale = gg * *wp;
  const float* incl = ws + p.o_incl;
  const float um1 = (float)(U - 1);
  float* gl = lds;
  float* sc = lds + (size_t)p.UT * S;
  float* tp = sc + 4 * (size_t)p.UT;      // tpart[0 .. K)[s], K <= 16
  ex.par([&](int tid, int nthr) {
    if (train && dE && tid < p.K) tp[tid] = ws[p.o_tpart + (size_t)tid * S + s];
    if (wg == 0 && tid == 0) {
      if (dw) *dw = gg * scal[1];
      if (db) *db = gg * scal[2];
    }
    if (!dE) return;
    for (int q = tid; q < nu * S; q += nthr) {
      const int i = q / S, j = q - i * S;
      const size_t row = (size_t)s * U + u0 + i;
      const float g = ws[p.o_dout + row * S + j];
      gl[q] = (train && j == s) ? 0.f : g;
      if (train && j == s) {
        sc[4 * i] = ws[p.o_rstat + 2 * row];
        sc[4 * i + 1] = ws[p.o_rstat + 2 * row + 1];
        sc[4 * i + 2] = g;
        sc[4 * i + 3] = ws[p.o_raw + row * S + j];
      }
    }
  });
  ex.par([&](int tid, int nthr) {
    if (!dE) return;
    for (int d = tid; d < D; d += nthr) {
      float shared = 0.f, c = 0.f;
      if (train) {
        // through the inclusive centroid of this speaker: x = c / U, incl = x / max(|x|, eps)
        float dincl = 0.f, t = 0.f, v[16];
        for (int k = 0; k < 16; ++k) v[k] = k < p.K ? ws[p.o_slab + ((size_t)k * S + s) * D + d] : 0.f;
        for (int k = 0; k < p.K; ++k) {
          dincl += v[k];
          t += tp[k];
        }
        const float den = ws[p.o_cstat + 2 * (size_t)s], fl = ws[p.o_cstat + 2 * (size_t)s + 1];
        const float dx = fl != 0.f ? (dincl - incl[(size_t)s * D + d] * t) / den : dincl / den;
        // ... and through the exclusive centroids of all utterances of this speaker
        shared = dx / (float)U + ws[p.o_asum + (size_t)s * D + d];
        c = ws[p.o_csum + (size_t)s * D + d];
      }
      for (int i = 0; i < nu; ++i) {
        const size_t row = (size_t)s * U + u0 + i;
        const float* g = gl + (size_t)i * S;
        const float* col = incl + d;
        float a = 0.f;
        ge2e_batch16(0, S, [&](int j) { return col[(size_t)j * D]; }, [&](int j, float v) { a += g[j] * v; });
        if (train) {
          const float* q = sc + 4 * i;
          const float e = E[row * D + d];
          a += q[2] * (((c - e) / um1) / q[0]);
          a += shared - ge2e_dv(c, e, um1, q[0], q[1], q[2], q[3]);
        }
        dE[row * D + d] = scale * a;
      }
    }
  });
}

}  // namespace ttrnn
