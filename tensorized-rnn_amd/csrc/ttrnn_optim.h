// ttrnn_optim.h — plan and phase bodies of the fused gradient scaling / norm clipping / Adam step (ttrnn_fast_optim.hip).
//
// The tail of the reference's training steps (speaker_encoder.py:61-67 do_gradient_ops + main.py:77-78 optimizer.step();
// pmnist_test.py:139,160-163; benchmarking.py:43,56) over a table of n fp32 tensors, in 1024-element CHUNKS:
//   * a chunk never spans two tensors; tensor i owns ceil(numel[i] / 1024) chunks, numbered consecutively over the table, and
//     its segment of m / v starts at 1024 x (its first chunk): the state is padded per tensor to whole chunks;
//   * phase P (partials): one fp32 sum of (grad_scale g)^2 per chunk, folded in an order fixed by the element index inside the
//     chunk — lane l of 256 takes elements 4 l .. 4 l + 3 in turn, 16 consecutive lanes are added in turn, the 16 results are
//     added in turn — whatever the number of threads;
//   * phase S (scalars, one thread): t = *step + 1, the bias corrections 1 - beta^t in double by repeated squaring from the
//     integer counter, step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t); *step = t;
//   * phase T (total): ALL chunk partials added in double, virtual lane j of 256 taking chunks j, j + 256, ... in turn, then a
//     binary tree over the 256 lanes; total_norm = (float)sqrt(sum); coef = min(max_norm / (total_norm + 1e-6), 1), NaN kept;
//   * phase U (update): per element, update_one() below.
// Written against the executor concept of ttrnn_core.h (`ex.par(f)`: run f for every thread, then barrier); the serial host
// executor of tests/hostemu/hostemu_optim.cpp runs the same bodies.  Nothing depends on the number of threads, on which
// workgroup takes which chunk, or on the order either runs in: p, m, v, g and total_norm are the same bits on every route.
//   route 1  one workgroup of 1024 threads; a table of one argument group: ONE launch (S, P, barrier, T, U; the partials pass
//            through the workspace, the gradients are re-read from L2); longer tables: the grid's launches with one workgroup
//   route 2  W workgroups of 256 threads, two launches per argument group: A = P of the workgroup's chunks (+ S in workgroup 0
//            of the first group), B = T (every workgroup, the same sum) + U of the workgroup's chunks.  All A launches precede
//            the first B launch: the norm spans every group.  Without clipping and without a total_norm request A is one
//            one-workgroup launch for S alone.
// The pointer tables travel by value in the kernel arguments (OptimGroup, 128 tensors: 3.6 KB of the 4 KB argument block).
#pragma once
#include "ttrnn_core.h"

namespace ttrnn {

#define TTRNN_OPTIM_THREADS1 1024      // route 1's workgroup
#define TTRNN_OPTIM_THREADS2 256       // route 2's workgroups
#define TTRNN_OPTIM_LANES 256          // virtual lanes of a chunk: 4 elements each
#define TTRNN_OPTIM_BATCH 16           // chunks a workgroup folds between two barriers
#define TTRNN_OPTIM_MAX_TENSORS 4096
#define TTRNN_OPTIM_MAX_WG 4096        // route 2: the most workgroups a descriptor may ask for
// route 0: one workgroup up to this many chunks, a grid above.  Measured per eager call (profiles/r13/optim_bench_first_run.txt,
// tools/optim_bench.py call): route 1 costs 23.3 / 23.4 / 30.1 / 54.6 us at 8 / 16 / 32 / 64 chunks (the first two are the host's
// floor for one launch; then +0.8 us per chunk on its one CU), the grid's two launches 26.0 ... 26.4 us up to 1024 chunks: the two
// lines cross at 24 chunks.  The reference encoder's one-layer table (20 chunks) takes one launch.
#define TTRNN_OPTIM_AUTO_ROUTE1_MAX_CHUNKS 24
#define TTRNN_OPTIM_AUTO_CHUNKS_PER_WG 4       // route 2, workgroups == 0: ceil(chunks of the group / 4), at most 1024
#define TTRNN_OPTIM_AUTO_MAX_WG 1024

// workspace, in floats: [0] step_size, [1] sqrt(1 - beta2^t), [2 .. 3] unused, [4 ..) one partial per chunk
#define TTRNN_OPTIM_WS_HEAD 4

struct alignas(16) OptimF4 { float a[4]; };

// one argument group: the tensors [first, first + n) of the table, by value in the kernel arguments
struct OptimGroup {
  float* p[TTRNN_OPTIM_GROUP];
  float* g[TTRNN_OPTIM_GROUP];
  int32_t cstart[TTRNN_OPTIM_GROUP + 1];   // first chunk of each tensor relative to c0; [n] = the group's chunk count
  int32_t numel[TTRNN_OPTIM_GROUP];
  float scale[TTRNN_OPTIM_GROUP];
  int32_t n;                               // tensors in this group
  int32_t c0;                              // the group's first chunk in the table's numbering
};

struct OptimPlan {
  int n, mode, route, write_grads;
  int W;              // route 2: workgroups asked for (0 = per group: optim_group_wg)
  int groups;         // argument groups = launches per phase
  int need_norm;      // clipping on, or total_norm wanted: phases P and T run
  int clip;           // max_norm > 0
  int64_t chunks;     // of the whole table
  float beta1, beta2, eps, weight_decay, max_norm;
};

// pure host arithmetic; TTRNN_OK, TTRNN_ERR_NULL, TTRNN_ERR_BAD_DESC or TTRNN_ERR_UNSUPPORTED.  want_norm: total_norm != NULL.
inline int optim_plan_init(OptimPlan* p, const ttrnn_optim_desc* d, const int64_t* numel, int want_norm) {
  if (!p || !d || !numel) return TTRNN_ERR_NULL;
  if (d->n_tensors < 1 || d->route < 0 || d->route > 2) return TTRNN_ERR_BAD_DESC;
  if (d->mode != TTRNN_OPTIM_ADAM && d->mode != TTRNN_OPTIM_CLIP_ONLY) return TTRNN_ERR_BAD_DESC;
  if (d->workgroups < 0 || d->workgroups > TTRNN_OPTIM_MAX_WG || (d->workgroups != 0 && d->route != 2)) return TTRNN_ERR_BAD_DESC;
  if (!(d->beta1 >= 0.f && d->beta1 < 1.f) || !(d->beta2 >= 0.f && d->beta2 < 1.f)) return TTRNN_ERR_BAD_DESC;
  if (!(d->eps > 0.f) || !(d->eps <= 3.0e38f) || !(d->weight_decay >= 0.f) || !(d->weight_decay <= 3.0e38f)) return TTRNN_ERR_BAD_DESC;
  if (d->max_norm != d->max_norm) return TTRNN_ERR_BAD_DESC;
  if (d->n_tensors > TTRNN_OPTIM_MAX_TENSORS) return TTRNN_ERR_UNSUPPORTED;
  int64_t total = 0, chunks = 0;
  for (int i = 0; i < d->n_tensors; ++i) {
    if (numel[i] < 1) return TTRNN_ERR_BAD_DESC;
    if (numel[i] >= ((int64_t)1 << 31)) return TTRNN_ERR_UNSUPPORTED;
    total += numel[i];
    chunks += (numel[i] + TTRNN_OPTIM_CHUNK - 1) / TTRNN_OPTIM_CHUNK;
    if (total >= ((int64_t)1 << 31)) return TTRNN_ERR_UNSUPPORTED;
  }
  p->n = d->n_tensors;
  p->mode = d->mode;
  p->write_grads = (d->write_grads != 0 || d->mode == TTRNN_OPTIM_CLIP_ONLY) ? 1 : 0;
  p->chunks = chunks;                       // < 2^21 + 4096
  p->groups = (d->n_tensors + TTRNN_OPTIM_GROUP - 1) / TTRNN_OPTIM_GROUP;
  p->route = d->route ? d->route : (chunks <= TTRNN_OPTIM_AUTO_ROUTE1_MAX_CHUNKS ? 1 : 2);
  p->W = d->workgroups;
  p->clip = d->max_norm > 0.f ? 1 : 0;
  p->need_norm = (p->clip || want_norm) ? 1 : 0;
  p->beta1 = d->beta1; p->beta2 = d->beta2; p->eps = d->eps; p->weight_decay = d->weight_decay; p->max_norm = d->max_norm;
  return TTRNN_OK;
}

inline int64_t optim_state_elems(const OptimPlan& p) { return p.chunks * TTRNN_OPTIM_CHUNK; }
inline size_t optim_ws_bytes(const OptimPlan& p) { return (size_t)(TTRNN_OPTIM_WS_HEAD + p.chunks) * sizeof(float); }

// the argument group `k` of the table (host); params may be NULL (CLIP_ONLY)
inline void optim_group_init(OptimGroup* gr, const OptimPlan& p, int k, const int64_t* numel, void* const* params, void* const* grads,
                             const float* grad_scale) {
  const int first = k * TTRNN_OPTIM_GROUP;
  int64_t c0 = 0;
  for (int i = 0; i < first; ++i) c0 += (numel[i] + TTRNN_OPTIM_CHUNK - 1) / TTRNN_OPTIM_CHUNK;
  gr->n = p.n - first < TTRNN_OPTIM_GROUP ? p.n - first : TTRNN_OPTIM_GROUP;
  gr->c0 = (int32_t)c0;
  int32_t c = 0;
  for (int i = 0; i < TTRNN_OPTIM_GROUP; ++i) {
    const bool in = i < gr->n;
    gr->p[i] = in && params ? (float*)params[first + i] : nullptr;
    gr->g[i] = in ? (float*)grads[first + i] : nullptr;
    gr->numel[i] = in ? (int32_t)numel[first + i] : 0;
    gr->scale[i] = in && grad_scale ? grad_scale[first + i] : 1.f;
    gr->cstart[i] = c;
    if (in) c += (int32_t)((numel[first + i] + TTRNN_OPTIM_CHUNK - 1) / TTRNN_OPTIM_CHUNK);
  }
  gr->cstart[TTRNN_OPTIM_GROUP] = c;
  for (int i = gr->n; i < TTRNN_OPTIM_GROUP; ++i) gr->cstart[i] = c;
}

// route 2: workgroups of a group's launches
inline int optim_group_wg(const OptimPlan& p, const OptimGroup& gr) {
  if (p.route == 1) return 1;
  if (p.W) return p.W;
  int w = (gr.cstart[TTRNN_OPTIM_GROUP] + TTRNN_OPTIM_AUTO_CHUNKS_PER_WG - 1) / TTRNN_OPTIM_AUTO_CHUNKS_PER_WG;
  return w < 1 ? 1 : (w > TTRNN_OPTIM_AUTO_MAX_WG ? TTRNN_OPTIM_AUTO_MAX_WG : w);
}

// LDS image of a workgroup
struct OptimLds {
  double tot[TTRNN_OPTIM_LANES];
  float lane[TTRNN_OPTIM_BATCH * TTRNN_OPTIM_LANES];
  float grp[TTRNN_OPTIM_BATCH * 16];
  float sc[4];       // step_size, sqrt(1 - beta2^t), coef, unused
};
enum { OPT_SC_STEP = 0, OPT_SC_BC2 = 1, OPT_SC_COEF = 2 };

// tensor of the group's chunk c (0 <= c < cstart[GROUP]): the last i with cstart[i] <= c among the first n
TT_HD int optim_find(const OptimGroup& gr, int c) {
  int lo = 0, hi = gr.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (gr.cstart[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

TT_HD bool optim_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// elements [off, off + 4) of a chunk of `len` elements at `base`; vec: base is 16-byte aligned.  Elements past len read as 0.
TT_HD OptimF4 optim_load4(const float* base, int off, int len, bool vec) {
  OptimF4 r;
  if (vec && off + 4 <= len) {
    __builtin_memcpy(&r, __builtin_assume_aligned(base + off, 16), sizeof r);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) r.a[e] = off + e < len ? base[off + e] : 0.f;
  }
  return r;
}
TT_HD void optim_store4(float* base, int off, int len, bool vec, const OptimF4& r) {
  if (vec && off + 4 <= len) {
    __builtin_memcpy(__builtin_assume_aligned(base + off, 16), &r, sizeof r);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (off + e < len) base[off + e] = r.a[e];
  }
}

// every product and sum below is rounded on its own (no contraction into fused multiply-adds the source does not spell out):
// the same bits from every kernel the bodies are compiled into, and from the host executor
#if defined(__clang__)
#define TTRNN_OPTIM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TTRNN_OPTIM_NO_CONTRACT
#endif

// a lane's share of its chunk's partial: the squares of its four scaled gradients, added in turn
TT_HD float optim_sq4(const OptimF4& g, float scale) {
  TTRNN_OPTIM_NO_CONTRACT
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = scale * g.a[e];
    s = s + x * x;
  }
  return s;
}

struct OptimCoefs {
  float scale, coef, beta1, beta2, omb1, omb2, eps, wd, step_size, bc2_sqrt;
};

// one element: include/ttrnn.h "Semantics".  g comes in raw and leaves scaled and clipped.
TT_HD void optim_update_one(const OptimCoefs& k, float& p, float& g, float& m, float& v) {
  TTRNN_OPTIM_NO_CONTRACT
  g = k.coef * (k.scale * g);
  const float gd = g + k.wd * p;
  m = k.beta1 * m + k.omb1 * gd;
  v = k.beta2 * v + (k.omb2 * gd) * gd;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p - k.step_size * (m / denom);
}

// beta^t, t >= 0, by repeated squaring in double: the same operations on the device and on the host
TT_HD double optim_powi(double b, int64_t t) {
  TTRNN_OPTIM_NO_CONTRACT
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r = r * b;
    b = b * b;
    t >>= 1;
  }
  return r;
}

// phase S by thread 0: sc[0 .. 1] (LDS or the workspace's head) and the counter
template <class Ex>
TT_HD void optim_scalars_body(Ex& ex, const OptimPlan& p, int64_t* step, const float* lr, float* sc) {
  ex.par([&](int tid, int) {
    if (tid != 0) return;
    const int64_t t = *step + 1;
    const double bc1 = 1.0 - optim_powi((double)p.beta1, t), bc2 = 1.0 - optim_powi((double)p.beta2, t);
    sc[OPT_SC_STEP] = (float)((double)*lr / bc1);
    sc[OPT_SC_BC2] = (float)sqrt(bc2);
    *step = t;
  });
}

// phase P: the partials of the group's chunks [c_lo, c_hi) into part[c0 + c]
template <class Ex>
TT_HD void optim_partials_body(Ex& ex, const OptimGroup& gr, int c_lo, int c_hi, float* part, OptimLds* lds) {
  for (int cb = c_lo; cb < c_hi; cb += TTRNN_OPTIM_BATCH) {
    const int nb = c_hi - cb < TTRNN_OPTIM_BATCH ? c_hi - cb : TTRNN_OPTIM_BATCH;
    ex.par([&](int tid, int nthr) {
      for (int idx = tid; idx < nb * TTRNN_OPTIM_LANES; idx += nthr) {
        const int c = cb + idx / TTRNN_OPTIM_LANES, l = idx % TTRNN_OPTIM_LANES;
        const int i = optim_find(gr, c);
        const int e0 = (c - gr.cstart[i]) * TTRNN_OPTIM_CHUNK;
        const int len = gr.numel[i] - e0 < TTRNN_OPTIM_CHUNK ? gr.numel[i] - e0 : TTRNN_OPTIM_CHUNK;
        const float* g = gr.g[i] + e0;
        lds->lane[idx] = optim_sq4(optim_load4(g, 4 * l, len, optim_aligned(g)), gr.scale[i]);
      }
    });
    ex.par([&](int tid, int nthr) {
      for (int idx = tid; idx < nb * 16; idx += nthr) {
        TTRNN_OPTIM_NO_CONTRACT
        float s = 0.f;
        for (int q = 0; q < 16; ++q) s = s + lds->lane[idx * 16 + q];
        lds->grp[idx] = s;
      }
    });
    ex.par([&](int tid, int nthr) {
      for (int idx = tid; idx < nb; idx += nthr) {
        TTRNN_OPTIM_NO_CONTRACT
        float s = 0.f;
        for (int q = 0; q < 16; ++q) s = s + lds->grp[idx * 16 + q];
        part[gr.c0 + cb + idx] = s;
      }
    });
  }
}

// phase T: every chunk partial of the table -> lds->sc[COEF]; total_norm (NULL-able) is written where `record` is set
template <class Ex>
TT_HD void optim_total_body(Ex& ex, const OptimPlan& p, const float* part, float* total_norm, bool record, OptimLds* lds) {
  const int nc = (int)p.chunks;
  ex.par([&](int tid, int nthr) {
    for (int j = tid; j < TTRNN_OPTIM_LANES; j += nthr) {
      TTRNN_OPTIM_NO_CONTRACT
      double a = 0.0;
      for (int c = j; c < nc; c += TTRNN_OPTIM_LANES) a = a + (double)part[c];
      lds->tot[j] = a;
    }
  });
  for (int s = TTRNN_OPTIM_LANES / 2; s >= 1; s >>= 1)
    ex.par([&](int tid, int nthr) {
      for (int j = tid; j < s; j += nthr) lds->tot[j] = lds->tot[j] + lds->tot[j + s];
    });
  ex.par([&](int tid, int) {
    TTRNN_OPTIM_NO_CONTRACT
    if (tid != 0) return;
    const float norm = (float)sqrt(lds->tot[0]);
    float coef = 1.f;
    if (p.clip) {
      coef = p.max_norm / (norm + 1e-6f);
      coef = coef > 1.f ? 1.f : coef;      // a NaN stays a NaN, as torch.clamp(max=1) keeps it
    }
    lds->sc[OPT_SC_COEF] = coef;
    if (record && total_norm) *total_norm = norm;
  });
}

// phase U over the group's chunks [c_lo, c_hi); sc: step_size and sqrt(1 - beta2^t) (ADAM mode)
template <class Ex>
TT_HD void optim_update_body(Ex& ex, const OptimPlan& p, const OptimGroup& gr, int c_lo, int c_hi, float coef, const float* sc,
                             float* m, float* v) {
  ex.par([&](int tid, int nthr) {
    OptimCoefs k;
    k.coef = coef;
    k.beta1 = p.beta1; k.beta2 = p.beta2; k.omb1 = 1.f - p.beta1; k.omb2 = 1.f - p.beta2;
    k.eps = p.eps; k.wd = p.weight_decay;
    const bool adam = p.mode == TTRNN_OPTIM_ADAM;
    k.step_size = adam ? sc[OPT_SC_STEP] : 0.f;
    k.bc2_sqrt = adam ? sc[OPT_SC_BC2] : 1.f;
    const int n = (c_hi - c_lo) * TTRNN_OPTIM_LANES;
    for (int idx = tid; idx < n; idx += nthr) {
      const int c = c_lo + idx / TTRNN_OPTIM_LANES, off = 4 * (idx % TTRNN_OPTIM_LANES);
      const int i = optim_find(gr, c);
      const int e0 = (c - gr.cstart[i]) * TTRNN_OPTIM_CHUNK;
      const int len = gr.numel[i] - e0 < TTRNN_OPTIM_CHUNK ? gr.numel[i] - e0 : TTRNN_OPTIM_CHUNK;
      if (off >= len) continue;
      k.scale = gr.scale[i];
      float* gp = gr.g[i] + e0;
      if (!adam) {
        const bool vec = optim_aligned(gp);
        OptimF4 g = optim_load4(gp, off, len, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          TTRNN_OPTIM_NO_CONTRACT
          g.a[e] = k.coef * (k.scale * g.a[e]);
        }
        optim_store4(gp, off, len, vec, g);
        continue;
      }
      float* pp = gr.p[i] + e0;
      float* mp = m + (size_t)(gr.c0 + c) * TTRNN_OPTIM_CHUNK;
      float* vp = v + (size_t)(gr.c0 + c) * TTRNN_OPTIM_CHUNK;
      const bool vec = optim_aligned(gp) && optim_aligned(pp) && optim_aligned(mp) && optim_aligned(vp);
      OptimF4 g = optim_load4(gp, off, len, vec), w = optim_load4(pp, off, len, vec);
      OptimF4 mm = optim_load4(mp, off, len, vec), vv = optim_load4(vp, off, len, vec);
#pragma unroll
      for (int e = 0; e < 4; ++e) optim_update_one(k, w.a[e], g.a[e], mm.a[e], vv.a[e]);
      optim_store4(pp, off, len, vec, w);
      optim_store4(mp, off, len, vec, mm);
      optim_store4(vp, off, len, vec, vv);
      if (p.write_grads) optim_store4(gp, off, len, vec, g);
    }
  });
}

// the group's chunks of workgroup wg of W: contiguous shares of ceil(chunks / W), the last ones short or empty
TT_HD void optim_share(const OptimGroup& gr, int wg, int W, int* c_lo, int* c_hi) {
  const int nc = gr.cstart[TTRNN_OPTIM_GROUP];
  const int per = (nc + W - 1) / W;
  const int64_t lo = (int64_t)wg * per, hi = lo + per;
  *c_lo = (int)(lo < nc ? lo : nc);
  *c_hi = (int)(hi < nc ? hi : nc);
}

// route 1, a table of one group: the whole call in one workgroup.  ws: TTRNN_OPTIM_WS_HEAD + chunks floats.
template <class Ex>
TT_HD void optim_route1_body(Ex& ex, const OptimPlan& p, const OptimGroup& gr, float* m, float* v, int64_t* step, const float* lr,
                             float* total_norm, float* ws, OptimLds* lds) {
  const int nc = gr.cstart[TTRNN_OPTIM_GROUP];
  if (p.mode == TTRNN_OPTIM_ADAM) optim_scalars_body(ex, p, step, lr, lds->sc);
  if (p.need_norm) {
    optim_partials_body(ex, gr, 0, nc, ws + TTRNN_OPTIM_WS_HEAD, lds);
    optim_total_body(ex, p, ws + TTRNN_OPTIM_WS_HEAD, total_norm, true, lds);
  }
  optim_update_body(ex, p, gr, 0, nc, p.need_norm ? lds->sc[OPT_SC_COEF] : 1.f, lds->sc, m, v);
}

// launch A of a group, workgroup wg of W: its chunks' partials; workgroup 0 of the first group also runs phase S
template <class Ex>
TT_HD void optim_a_body(Ex& ex, const OptimPlan& p, const OptimGroup& gr, int wg, int W, int64_t* step, const float* lr, float* ws,
                        OptimLds* lds) {
  if (wg == 0 && gr.c0 == 0 && p.mode == TTRNN_OPTIM_ADAM) optim_scalars_body(ex, p, step, lr, ws);
  if (!p.need_norm) return;
  int c_lo, c_hi;
  optim_share(gr, wg, W, &c_lo, &c_hi);
  optim_partials_body(ex, gr, c_lo, c_hi, ws + TTRNN_OPTIM_WS_HEAD, lds);
}

// launch B of a group, workgroup wg of W: the total (every workgroup, the same sum), then its chunks' update
template <class Ex>
TT_HD void optim_b_body(Ex& ex, const OptimPlan& p, const OptimGroup& gr, int wg, int W, float* m, float* v, float* total_norm,
                        const float* ws, OptimLds* lds) {
  if (p.need_norm) optim_total_body(ex, p, ws + TTRNN_OPTIM_WS_HEAD, total_norm, wg == 0 && gr.c0 == 0, lds);
  int c_lo, c_hi;
  optim_share(gr, wg, W, &c_lo, &c_hi);
  optim_update_body(ex, p, gr, c_lo, c_hi, p.need_norm ? lds->sc[OPT_SC_COEF] : 1.f, ws, m, v);
}

}  // namespace ttrnn
