// ttrnn_eer.h — plan and phase bodies of the equal error rate of a GE2E similarity matrix (ttrnn_fast_eer.hip).
//
// sim is fp32 [S][U][S]; element e = (s U + u) S + j is a positive iff j == s.  P = S U positives, Nn = S U (S - 1) negatives.
// The ROC polyline's vertices are the counts (fp, tp) of negatives / positives at or above each distinct score, taken in
// descending order from (0, 0).  The EER (roc_curve + interp1d + brentq of ttrnn_hip/ge2e.py:36-44 = speaker_encoder.py:160-168
// of the reference) is where that polyline meets tpr = 1 - fpr: with theta the LARGEST score whose at-or-above counts satisfy
//     fp P + tp Nn >= Nn P                                                                                       (*)
// and (fp', tp') the counts strictly above theta,
//     a = Nn P - (fp' P + tp' Nn),   b = (fp - fp') P + (tp - tp') Nn,   eer = (fp' + (a / b) (fp - fp')) / Nn.
// No sort: theta is found by a radix selection, most significant digit first, over a monotone 32-bit key of the fp32 bits
// (four digits of eight bits).  A pass histograms, separately for positives and negatives, the current digit of the elements
// whose higher digits equal the prefix chosen so far; the left side of (*) grows as the threshold falls, so the digit is the
// largest bin whose at-or-above counts (the carried counts of everything above the prefix, plus the bins above, plus the bin)
// satisfy (*).  That bin is never empty: the carried counts fail (*) and only a non-empty bin changes them.  After the fourth
// pass the prefix is theta's key, the carried counts are (tp', fp') and adding the bin gives (tp, fp).
//
// All counts are integers: the result does not depend on the order of threads or workgroups.  Written against the executor
// concept of ttrnn_core.h (`ex.par(f)`: run f for every thread, then barrier) plus `ex.add(p, v)`: an integer add to a
// workgroup-local (LDS) counter that other threads of the same par may add to as well — an LDS atomic on the device, a
// plain += in the serial host executor of tests/hostemu/hostemu_eer.cpp.
//   route 1  one workgroup, one launch: the four passes in sequence, histograms in LDS, sim re-read (from L2) each pass
//   route 2  G workgroups: one launch per pass; workgroup g histograms the contiguous chunk [g CH, g CH + CH) and writes its
//            513 counters as a partial with plain stores; every workgroup of the next launch adds the G partials in index order
//            and derives the same prefix and carried counts (workgroup 0 records them for the launch after); a one-workgroup
//            fifth launch derives the last digit and evaluates the formula.  No global atomics, no workgroup waits on another.
#pragma once
#include "ttrnn_core.h"

namespace ttrnn {

#define TTRNN_EER_THREADS1 1024        // route 1's workgroup
#define TTRNN_EER_THREADS2 256         // route 2's workgroups
#define TTRNN_EER_MAX_WG 256           // route 2: the most workgroups a descriptor may ask for
#define TTRNN_EER_MAX_S 2048
#define TTRNN_EER_MAX_ROWS (1 << 22)
#define TTRNN_EER_MAX_ELEMS (1 << 30)  // element indices and every counter fit 32 bits
#define TTRNN_EER_AUTO_ROUTE1_MAX 24576        // route 0: one workgroup up to this many scores (the measured crossing)
#define TTRNN_EER_AUTO_SQRT_DIV 12.0           // route 2, workgroups == 0: sqrt(scores) / 12 workgroups, 1 .. MAX_WG
#define TTRNN_EER_BINS 256
#define TTRNN_EER_NCNT 513             // positives' bins, negatives' bins, NaN count
#define TTRNN_EER_PART 516             // a partial's stride in the workspace (16-byte multiple)
#define TTRNN_EER_BATCH 16             // loads in flight per thread

// LDS image (uint32 words)
#define TTRNN_EER_L_HIST 0                                   // [516] hp[256], hn[256], nan
#define TTRNN_EER_L_GRP (TTRNN_EER_L_HIST + TTRNN_EER_PART)  // [32]  sums of 16 bins
#define TTRNN_EER_L_SP (TTRNN_EER_L_GRP + 32)                // [256] positives at or above bin b (carried included)
#define TTRNN_EER_L_SN (TTRNN_EER_L_SP + 256)                // [256] negatives
#define TTRNN_EER_L_OK (TTRNN_EER_L_SN + 256)                // [256] (*) holds at bin b
#define TTRNN_EER_L_ST (TTRNN_EER_L_OK + 256)                // [8]   state
#define TTRNN_EER_LDS_WORDS (TTRNN_EER_L_ST + 8)
// state words: the key's chosen digits, positives / negatives strictly above them, NaN seen, positives / negatives of the chosen bin
enum { EER_ST_PREFIX = 0, EER_ST_CP, EER_ST_CN, EER_ST_NAN, EER_ST_BP, EER_ST_BN, EER_ST_WORDS = 8 };

struct EerPlan {
  int S, U;
  int route;        // 1 or 2
  int G;            // workgroups of route 2 (1 for route 1)
  int N;            // scores
  int CH;           // route 2: scores per workgroup
  int64_t P, Nn;
  size_t o_state, o_part, total;      // workspace, in uint32 words: state[5][8], partials[2][G][516]
};

// pure host arithmetic; TTRNN_OK, TTRNN_ERR_NULL, TTRNN_ERR_BAD_DESC or TTRNN_ERR_UNSUPPORTED
inline int eer_plan_init(EerPlan* p, const ttrnn_eer_desc* d) {
  if (!p || !d) return TTRNN_ERR_NULL;
  if (d->S < 2 || d->U < 1 || d->route < 0 || d->route > 2) return TTRNN_ERR_BAD_DESC;
  if (d->workgroups < 0 || d->workgroups > TTRNN_EER_MAX_WG || (d->workgroups != 0 && d->route != 2)) return TTRNN_ERR_BAD_DESC;
  if (d->S > TTRNN_EER_MAX_S) return TTRNN_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)d->S * d->U;
  if (rows > TTRNN_EER_MAX_ROWS || rows * d->S > TTRNN_EER_MAX_ELEMS) return TTRNN_ERR_UNSUPPORTED;
  p->S = d->S; p->U = d->U;
  p->N = (int)(rows * d->S);
  p->P = rows;
  p->Nn = rows * (d->S - 1);
  p->route = d->route ? d->route : (p->N <= TTRNN_EER_AUTO_ROUTE1_MAX ? 1 : 2);
  int G = 1;
  if (p->route == 2) {
    G = d->workgroups;
    if (G == 0) {
      // a pass costs ~ N / G for the chunk plus ~ G for the partials every workgroup adds: the optimum grows as sqrt(N)
      G = (int)(sqrt((double)p->N) / TTRNN_EER_AUTO_SQRT_DIV + 0.5);
      if (G < 1) G = 1;
      if (G > TTRNN_EER_MAX_WG) G = TTRNN_EER_MAX_WG;
    }
  }
  p->G = G;
  p->CH = (p->N + G - 1) / G;
  p->o_state = 0;
  p->o_part = 5 * EER_ST_WORDS;
  p->total = p->o_part + (p->route == 2 ? 2 * (size_t)G * TTRNN_EER_PART : 0);
  return TTRNN_OK;
}

TT_HD uint32_t eer_bits(const float* p) {
  uint32_t u;
  __builtin_memcpy(&u, p, sizeof u);
  return u;
}
TT_HD bool eer_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
// order-preserving key: -0 is +0; negative values are complemented, the others get the sign bit set
TT_HD uint32_t eer_key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}
TT_HD uint32_t eer_unkey(uint32_t key) { return (key & 0x80000000u) ? key & 0x7fffffffu : ~key; }

// One digit pass over the scores [e0, e1): hist[0 .. 513) (LDS) is zeroed and receives the counts of digit `pass` of the
// elements that match `prefix` in the digits above it; hist[512] counts the threads that met a NaN (pass 0 only).  A thread
// walks e0 + tid, e0 + tid + nthr, ...: its column advances by nthr mod S with a carry into the row, so the label costs no
// division (row in [col U, col U + U) <=> col is the row's speaker), and a run of equal counters costs one add.
template <class Ex>
TT_HD void eer_hist_body(Ex& ex, const EerPlan& p, int pass, uint32_t prefix, int e0, int e1, const float* sim, uint32_t* hist) {
  ex.par([&](int tid, int nthr) {
    for (int i = tid; i < TTRNN_EER_NCNT; i += nthr) hist[i] = 0u;
  });
  const int shift = 24 - 8 * pass;
  ex.par([&](int tid, int nthr) {
    const int S = p.S, U = p.U;
    const int dcol = nthr % S, drow = nthr / S;
    int e = e0 + tid;
    if (e >= e1) return;
    int row = e / S, col = e - row * S;
    int cur = -1;
    uint32_t cnt = 0u, nan = 0u;
    for (; e < e1; e += TTRNN_EER_BATCH * nthr) {
      uint32_t v[TTRNN_EER_BATCH];
#pragma unroll
      for (int m = 0; m < TTRNN_EER_BATCH; ++m) {
        const int idx = e + m * nthr;      // < 2^30 + 16 * 1024
        v[m] = idx < e1 ? eer_bits(sim + idx) : 0u;
      }
#pragma unroll
      for (int m = 0; m < TTRNN_EER_BATCH; ++m) {
        if (e + m * nthr < e1) {
          const uint32_t key = eer_key(v[m]);
          if (pass == 0 && eer_is_nan(v[m])) nan = 1u;
          if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) {
            const bool pos = (unsigned)(row - col * U) < (unsigned)U;
            const int slot = (int)((key >> shift) & 255u) + (pos ? 0 : TTRNN_EER_BINS);
            if (slot == cur) {
              ++cnt;
            } else {
              if (cnt) ex.add(hist + cur, cnt);
              cur = slot;
              cnt = 1u;
            }
          }
        }
        col += dcol;
        row += drow;
        if (col >= S) {
          col -= S;
          ++row;
        }
      }
    }
    if (cnt) ex.add(hist + cur, cnt);
    if (nan) ex.add(hist + 2 * TTRNN_EER_BINS, 1u);
  });
}

// The digit of `pass` from its total histogram tot[0 .. 512) (LDS): st (LDS) holds the prefix and carried counts before the
// pass on entry and after it on return, with the chosen bin's own counts in BP / BN.  Uniform: every workgroup that runs it on
// the same totals and state gets the same result.
template <class Ex>
TT_HD void eer_select_body(Ex& ex, const EerPlan& p, int pass, const uint32_t* tot, uint32_t* lds) {
  uint32_t* grp = lds + TTRNN_EER_L_GRP;
  uint32_t* sp = lds + TTRNN_EER_L_SP;
  uint32_t* sn = lds + TTRNN_EER_L_SN;
  uint32_t* ok = lds + TTRNN_EER_L_OK;
  uint32_t* st = lds + TTRNN_EER_L_ST;
  ex.par([&](int tid, int nthr) {
    for (int q = tid; q < 32; q += nthr) {
      uint32_t a = 0u;
      for (int i = 0; i < 16; ++i) a += tot[q * 16 + i];
      grp[q] = a;
    }
  });
  ex.par([&](int tid, int nthr) {
    for (int b = tid; b < TTRNN_EER_BINS; b += nthr) {
      const int g = b >> 4;
      uint32_t ap = st[EER_ST_CP], an = st[EER_ST_CN];
      for (int k = g + 1; k < 16; ++k) {
        ap += grp[k];
        an += grp[16 + k];
      }
      for (int i = b; i < (g + 1) * 16; ++i) {
        ap += tot[i];
        an += tot[TTRNN_EER_BINS + i];
      }
      sp[b] = ap;
      sn[b] = an;
      ok[b] = ((int64_t)an * p.P + (int64_t)ap * p.Nn >= p.Nn * p.P) ? 1u : 0u;
    }
  });
  ex.par([&](int tid, int nthr) {
    for (int b = tid; b < TTRNN_EER_BINS; b += nthr) {
      if (ok[b] && (b == TTRNN_EER_BINS - 1 || !ok[b + 1])) {      // exactly one b: ok is monotone and ok[0] holds
        const uint32_t hp = tot[b], hn = tot[TTRNN_EER_BINS + b];
        st[EER_ST_PREFIX] |= (uint32_t)b << (24 - 8 * pass);
        st[EER_ST_CP] = sp[b] - hp;
        st[EER_ST_CN] = sn[b] - hn;
        st[EER_ST_BP] = hp;
        st[EER_ST_BN] = hn;
      }
    }
  });
}

// the formula, by thread 0, from the state after the last pass
template <class Ex>
TT_HD void eer_final_body(Ex& ex, const EerPlan& p, const uint32_t* st, double* eer, float* threshold, int64_t* counts) {
  ex.par([&](int tid, int) {
    if (tid != 0) return;
    if (st[EER_ST_NAN]) {
      *eer = (double)NAN;
      if (threshold) *threshold = NAN;
      if (counts) counts[0] = counts[1] = counts[2] = counts[3] = -1;
      return;
    }
    const int64_t tp0 = st[EER_ST_CP], fp0 = st[EER_ST_CN];
    const int64_t tp1 = tp0 + st[EER_ST_BP], fp1 = fp0 + st[EER_ST_BN];
    const int64_t a = p.Nn * p.P - (fp0 * p.P + tp0 * p.Nn);      // every product < 2^53
    const int64_t b = (fp1 - fp0) * p.P + (tp1 - tp0) * p.Nn;      // > 0: the chosen bin is not empty
    *eer = ((double)fp0 + ((double)a / (double)b) * (double)(fp1 - fp0)) / (double)p.Nn;
    if (threshold) {
      const uint32_t bits = eer_unkey(st[EER_ST_PREFIX]);
      __builtin_memcpy(threshold, &bits, sizeof bits);
    }
    if (counts) {
      counts[0] = tp0;
      counts[1] = fp0;
      counts[2] = tp1;
      counts[3] = fp1;
    }
  });
}

TT_HD void eer_state_init(uint32_t* st, int tid, int nthr) {
  for (int i = tid; i < EER_ST_WORDS; i += nthr) st[i] = 0u;
}

// route 1: the whole call in one workgroup.  lds: TTRNN_EER_LDS_WORDS words.
template <class Ex>
TT_HD void eer_route1_body(Ex& ex, const EerPlan& p, const float* sim, double* eer, float* threshold, int64_t* counts,
                           uint32_t* lds) {
  uint32_t* hist = lds + TTRNN_EER_L_HIST;
  uint32_t* st = lds + TTRNN_EER_L_ST;
  ex.par([&](int tid, int nthr) { eer_state_init(st, tid, nthr); });
  for (int pass = 0; pass < 4; ++pass) {
    eer_hist_body(ex, p, pass, st[EER_ST_PREFIX], 0, p.N, sim, hist);
    if (pass == 0) ex.par([&](int tid, int) { if (tid == 0) st[EER_ST_NAN] = hist[2 * TTRNN_EER_BINS]; });
    eer_select_body(ex, p, pass, hist, lds);
  }
  eer_final_body(ex, p, st, eer, threshold, counts);
}

// route 2, the start of launch `pass` (1 .. 4): the totals of pass - 1's partials, added in workgroup order, into the LDS
// histogram; the state before pass - 1 (zeros for pass 1, else what workgroup 0 of the launch before recorded); the selection.
// Leaves the state after pass - 1 in LDS; workgroup 0 records it in the workspace's slot `pass`.
template <class Ex>
TT_HD void eer_resume_body(Ex& ex, const EerPlan& p, int pass, int wg, uint32_t* ws, uint32_t* lds) {
  uint32_t* hist = lds + TTRNN_EER_L_HIST;
  uint32_t* st = lds + TTRNN_EER_L_ST;
  const uint32_t* part = ws + p.o_part + (size_t)((pass - 1) & 1) * p.G * TTRNN_EER_PART;
  const uint32_t* prev = ws + p.o_state + (size_t)(pass - 1) * EER_ST_WORDS;
  ex.par([&](int tid, int nthr) {
    // the NaN counter is pass 0's alone; sixteen partials' loads in flight at a time
    for (int i = tid; i < (pass == 1 ? TTRNN_EER_NCNT : 2 * TTRNN_EER_BINS); i += nthr) {
      uint32_t a = 0u;
      for (int g0 = 0; g0 < p.G; g0 += 16) {
        uint32_t v[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = g0 + m < p.G ? part[(size_t)(g0 + m) * TTRNN_EER_PART + i] : 0u;
#pragma unroll
        for (int m = 0; m < 16; ++m) a += v[m];
      }
      hist[i] = a;
    }
    if (pass == 1) eer_state_init(st, tid, nthr);
    else
      for (int i = tid; i < EER_ST_WORDS; i += nthr) st[i] = prev[i];
  });
  if (pass == 1) ex.par([&](int tid, int) { if (tid == 0) st[EER_ST_NAN] = hist[2 * TTRNN_EER_BINS]; });
  eer_select_body(ex, p, pass - 1, hist, lds);
  if (wg == 0) {
    uint32_t* rec = ws + p.o_state + (size_t)pass * EER_ST_WORDS;
    ex.par([&](int tid, int nthr) {
      for (int i = tid; i < EER_ST_WORDS; i += nthr) rec[i] = st[i];
    });
  }
}

// route 2, launch `pass` (0 .. 3), workgroup wg: (resume), this workgroup's chunk's histogram of digit `pass`, its partial
template <class Ex>
TT_HD void eer_pass_body(Ex& ex, const EerPlan& p, int pass, int wg, const float* sim, uint32_t* ws, uint32_t* lds) {
  uint32_t* hist = lds + TTRNN_EER_L_HIST;
  uint32_t prefix = 0u;
  if (pass > 0) {
    eer_resume_body(ex, p, pass, wg, ws, lds);
    prefix = lds[TTRNN_EER_L_ST + EER_ST_PREFIX];
  }
  const int64_t b0 = (int64_t)wg * p.CH, b1 = b0 + p.CH;
  const int e0 = (int)(b0 < p.N ? b0 : p.N), e1 = (int)(b1 < p.N ? b1 : p.N);
  eer_hist_body(ex, p, pass, prefix, e0, e1, sim, hist);
  uint32_t* mine = ws + p.o_part + ((size_t)(pass & 1) * p.G + wg) * TTRNN_EER_PART;
  ex.par([&](int tid, int nthr) {
    for (int i = tid; i < TTRNN_EER_NCNT; i += nthr) mine[i] = hist[i];
  });
}

// route 2, the fifth launch (one workgroup): the last digit and the formula
template <class Ex>
TT_HD void eer_last_body(Ex& ex, const EerPlan& p, uint32_t* ws, double* eer, float* threshold, int64_t* counts, uint32_t* lds) {
  eer_resume_body(ex, p, 4, 0, ws, lds);
  eer_final_body(ex, p, lds + TTRNN_EER_L_ST, eer, threshold, counts);
}

}  // namespace ttrnn
