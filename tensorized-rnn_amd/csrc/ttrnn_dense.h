// ttrnn_dense.h — plan and index maps of the dense (d = 1, nn.Linear) step kernels (ttrnn_fast_dense.hip): route TTRNN_ROUTE_DENSE_STEP.
//
// One launch per time step computes  [x_t | h_{t-1}] . [W_in ; W_hh]  as a GEMM on v_mfma_f32_16x16x32_bf16 (three bf16 pieces per
// operand, six terms, fp32 accumulation) with the cell as its epilogue.  Everything below is plain integer arithmetic shared by the
// host (workspace queries) and the kernels; tests/test_dense_route_host.py rehearses the same maps in numpy.
//
//   tiles     workgroup = 4 waves = 32 batch rows x 32 hidden units; wave w: rows 16 (w & 1) .. + 16, units 16 (w >> 1) .. + 16
//   K         Kxp = in rounded up to 32 (zero columns), then the H columns of h: K = Kxp + H, k-blocks of 32
//   slots     a wave's four accumulators are the four gate slots of its 16 units — lane (n, q) holds unit n, rows 4q .. 4q + 3:
//               LSTM  i, g, f, o  (the reserve record's order; gates 0, 2, 1, 3 of lstm.py:26-29)
//               GRU   r, z, n_x, n_h: slot 2 sees only the x columns (W_in x), slot 3 only the h columns (W_hn h), gru.py:42-43
//   WF planes [H/16][K/32][slot 4][piece 3][lane 64][8] bf16: the B fragment of (unit tile, k-block, slot, piece) is ONE 1 KB read;
//             lane (n, q), element e  <->  k = 32 kb + 8 q + e, unit 16 ut + n
//   WR planes [H/16][G H/32][piece 3][lane 64][8] bf16 of W_hh as seen by dh = dg_hid . W_hh: k = column of d_gates_hid
//   A planes  [piece 3][Bp][cols] bf16 row-major (Bp = B rounded up to 32; rows >= B are never initialised: a row of the product
//             depends on its own row of A only, and those rows are never stored)
#pragma once
#include <stddef.h>
#include "ttrnn_core.h"

namespace ttrnn {

static constexpr int DENSE_UNIT_TILE = 32;      // hidden units per workgroup (H must be a multiple)
static constexpr int DENSE_BATCH_TILE = 32;     // batch rows per workgroup
static constexpr int DENSE_MIN_H = 128;

struct DensePlan {
  int Bp, Kxp, K, nkx, nkb, nkr;      // padded batch; padded x columns; forward K; k-blocks of x / forward / reverse
  size_t wf_bytes, hpl_bytes, c_bytes, h32_bytes, fwd_bytes;       // forward workspace regions, in this order
  size_t wr_bytes, dgpl_bytes, carry_bytes, bwd_bytes;             // reverse workspace regions, in this order
};

inline DensePlan dense_plan(const RnnShape& rs) {
  DensePlan p{};
  const size_t H = (size_t)rs.H, GH = (size_t)rs.G * rs.H;
  p.Bp = (rs.B + DENSE_BATCH_TILE - 1) / DENSE_BATCH_TILE * DENSE_BATCH_TILE;
  p.Kxp = (rs.in + 31) / 32 * 32;
  p.K = p.Kxp + rs.H;
  p.nkx = p.Kxp / 32;
  p.nkb = p.K / 32;
  p.nkr = (int)(GH / 32);
  p.wf_bytes = (H / 16) * p.nkb * 4 * 3 * 1024;         // = 24 K H
  p.hpl_bytes = 2 * 3 * (size_t)p.Bp * H * 2;           // two buffers (step parity) of three planes
  p.c_bytes = (size_t)p.Bp * H * 4;
  p.h32_bytes = 2 * (size_t)p.Bp * H * 4;               // fp32 h ping-pong of an out == NULL call (the GRU's h_{t-1} term)
  // One formula for both cells, at the price of regions a cell does not use: the GRU's planes hold the all-zero h k-blocks of
  // slot 2 and x k-blocks of slot 3 (about a quarter of wf_bytes, written by prep, never read); the LSTM never touches h32, the
  // GRU never touches c.  Dropping them means per-cell formulas and a per-cell fragment stride.
  p.fwd_bytes = p.wf_bytes + p.hpl_bytes + p.c_bytes + p.h32_bytes;      // = 24 K H + 24 Bp H
  p.wr_bytes = (H / 16) * p.nkr * 3 * 1024;             // = 6 G H H
  p.dgpl_bytes = 2 * 3 * (size_t)p.Bp * GH * 2;
  p.carry_bytes = (size_t)p.Bp * H * 4;                 // dc (LSTM) / dh z (GRU) handed to the next launch
  p.bwd_bytes = p.wr_bytes + p.dgpl_bytes + p.carry_bytes;               // = 6 G H H + 12 Bp G H + 4 Bp H
  return p;
}

// LSTM: slot -> gate of lstm.py's i, f, g, o order
TT_HD int dense_lstm_gate_of_slot(int slot) { return slot == 1 ? 2 : (slot == 2 ? 1 : slot); }

}  // namespace ttrnn
