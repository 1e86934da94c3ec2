// ttrnn_fast_f10t.hip — the fused-core TT-LSTM forward kernel with cores 0·1 contracted FIRST (gfx950, rounds 7 and 8).
// The kernel template is in ttrnn_f10t_kernel.h; this file instantiates its default time loop (ADJ = true, round 8, below),
// ttrnn_fast_f10t_r7.hip round 7's loop (ADJ = false, option f10t_r7_loop).
//
// k_lstm_fwd_f10q keeps the reference's order: core 2 first (S2), then the fused core W10 = cores 1·0 (S10).  In that order every
// wave needs ALL of C2 for its S10 tile: a 16 KB image in LDS, sixteen ds_read_b128 per wave and a barrier in front of them, every
// step.  Here the order is the other one (the scales and layouts: ttrnn_f10_dev.h, "cores 0·1 FIRST"):
//     stage 1   D[(m, r2)][j2] = sum_{k = (j0, j1)} W10[m][k][r2] h[k][j2]        per wave: 16 rows m, one 16x16x32 tile per r2
//     stage 2   out[m][i2]     = sum_{(r2, j2)} D[m][(r2, j2)] G2[(r2, j2)][i2]    per wave: 16 rows m, K = 64
// Stage 1 needs only h: 256 values, 1 KB as two fp16 pieces, ONE ds_read_b128 per lane.  h is the A operand, W10[., ., r2] of the
// wave's 16 rows the B operand: the result tile has m on the lane and h's rows in the registers.  Folded (first-piece sum +
// second-piece sum) and split again, the eight tiles already ARE stage 2's A operand (row = m, k = 8 q + j), no LDS, no barrier
// in between.  Per wave and step: 16 + 6 MFMAs (28 before), one LDS read (20 before), one barrier (two before).
//   Round 7 (ADJ = false): rows 0-7 = first pieces of j2 = row, rows 8-15 = second pieces; a unit's two sums land 32 lanes apart and
// one v_permlane32_swap per register folds a PAIR of tiles (r2 = p, p + 4).  cfg2 (profiles/r7/): 478.5 -> 378.5 us per call.
//   Round 8 (ADJ = true, the default): row 2 j2 + piece.  Lane (c, q) of tile r2 holds in registers 0/1 the two sums of j2 = 2 q and
// in 2/3 those of j2 = 2 q + 1: the fold is two adds in the lane (the same two addends as before: the same bits), one split_pair_h
// per tile, tile r2 -> dword r2 & 3 of k-block r2 >> 2, i.e. k = 8 q + j <-> r2 = 4 kb + (j >> 1), j2 = 2 q + (j & 1)
// (f10t_load_g2<S, true> builds core 2's fragment in that order; stage 2 sums in another order than round 7, so the two loops agree
// to rounding, not bit for bit: tests/test_f10t_loop.py).  The image's rows are 96 bytes apart and a row's four 16-byte chunks are
// XORed with row >> 2 (f10t_img_off): by the LDS rules the ds_read_b128 (four 16-lane groups, 64 banks) and both ds_write_b16 (two
// 32-lane halves, 32 banks) are conflict-free (degree 1; tests/test_f10t_layout.py counts it; 64-byte rows: read 2-way, writes
// 8-way).  The next step's fragment is read right behind the barrier, at the END of the step, so that the pointer bumps and the loop
// control issue in the read's shadow and not in front of it.  The file is built with -fno-slp-vectorize (csrc/Makefile): with the
// vectoriser on, every tile's two adds become a v_pk_add_f32 behind three v_mov (24 v_mov per step) and the layout gains nothing.
// Time loop of the benchmark's instantiation <S, false, true, true, true>, per step: 153 instructions (round 7: 147) — 22 v_mfma,
// 0 v_permlane32_swap (16), 21 v_add_f32 (5), 16 v_cvt_pk_f16_f32, 16 v_fma_mix_f32, 6 v_fma_f32, 5 v_exp_f32, 5 v_rcp_f32,
// 3 packed f32 (the accumulators' un-scaling behind the last MFMA; round 7: 13), 7 v_mov, 21 cycles of s_nop pads (round 7: 24), 2 ds_write_b16, 1 ds_read_b128, 1 global store (3 with reserve records), 1 barrier.
// Measured on cfg2 (profiles/r8/ab_cfg2_f10t_loop.txt): 378.1 -> 317.3 us per call; layout alone (vectoriser on) no gain, layout +
// flag -8.7 %, + read behind the barrier -15.4 %; the input term x_{t+1} moved behind the read too was 3.7 % SLOWER and is not in.
// The stage-1 fragments are built in the prologue from the packed cores (f10t_build_w10: the workspace of the shape has no room
// for a second set), core 2's fragment too; from the workspace only the header's eu / ev are read.
// Resources (-Rpass-analysis=kernel-resource-usage): 184 ... 192 VGPRs over the instantiations (round 7's loop: 191 ... 196; the
// prologue's peak; the time loop holds 64 + 16 of fragments), 0 AGPRs, 0 scratch, 3 136 bytes of LDS (round 7's loop: 2 112).
// Same unit ownership as k_lstm_fwd_f10q (lane (c, q) of wave w: unit (4 w + q) 16 + c, accumulator registers = gates i, f, g, o),
// same gate phase, input paths, reserve records and stores.
// Replaces the same reference code as ttrnn_fast_f10.hip: tensorized_rnn/lstm.py:23-32,123-133 + t3nsor/ops.py:78-93.
#include "ttrnn_f10t_kernel.h"

namespace ttrnn {

// Default for cfg2's shape in split mode while every sample has a CU of its own (measured: profiles/r7/ab_cfg2_forward.txt);
// option f10t_off keeps k_lstm_fwd_f10q.  More samples than CUs (two workgroups per CU) stay on k_lstm_fwd_f10q: not measured.
bool f10t_available(const RnnShape& rs) {
  if (opt(OPT_F10T_OFF)) return false;
  return shape_matches<ShpH256R8L>(rs.hid_s) && rs.B <= device_cu_count();
}

// ws: the scale header of k_f10h_scale / the fused set-up launch (eu, ev); the old-order fragments behind it are not read.
// Option f10t_r7_loop: round 7's time loop (fold across the wave's halves; ttrnn_fast_f10t_r7.hip) instead of the fold in the lane (A/B).
int launch_rnn_fwd_f10_t(const RnnShape& rs, GinSrc gin, const void* h0, const void* c0, const float* packed_hid,
                         const void* ws, const float* bias_hid, void* out, void* hT, void* cT, float* reserve,
                         hipStream_t stream) {
  using S = ShpH256R8L;
  if (!shape_matches<S>(rs.hid_s)) return TTRNN_ERR_UNSUPPORTED;
  if (opt(OPT_F10T_R7_LOOP)) return launch_rnn_fwd_f10_t_r7(rs, gin, h0, c0, packed_hid, ws, bias_hid, out, hT, cT, reserve, stream);
  return launch_f10t<S, true>(rs, gin, h0, c0, packed_hid, reinterpret_cast<const float*>(ws), bias_hid, out, hT, cT, reserve, stream);
}

}  // namespace ttrnn
