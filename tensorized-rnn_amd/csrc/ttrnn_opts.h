// ttrnn_opts.h — process-wide library options (kernel-route A/B switches and the fp32 math mode): ONE table, from which the ids,
// the names, the TTRNN_<NAME> environment variables, the defaults and the range checks are generated (ttrnn_api.hip).
// Read ONCE from the environment at first use, afterwards only through ttrnn_set_option / ttrnn_get_option (include/ttrnn.h): no
// getenv on any launch path, and every value is a relaxed atomic, so host threads may launch while another flips a switch.
#pragma once
#include <atomic>

// X(id, "name", kind, default, legacy word, legacy mask, "description")
//   kind: BOOL 0|1, R02 0..2, S023 one of {0, 2, 3}, MATH TTRNN_MATH_EXACT|TTRNN_MATH_SPLIT, WORD 0..0x3FFFFFFF.
//   legacy word / mask: the switch was this bit of `dev` / `dev2` once; setting the word by number sets the switch and setting the
//   switch shows in the word, so old command lines (TTRNN_DEV=..., TTRNN_DEV2=...) keep their meaning.  Where both are in the
//   environment the named variable wins: the two words come first in the table and the rows are read in order.
#define TTRNN_OPTIONS(X)                                                                                                          \
  X(DEV,  "dev",  WORD, 0, NONE, 0, "raw word: old numeric command lines, and the -DTTRNN_ABLATIONS build's bits 2 / 8 / 16 / 32 / 64") \
  X(DEV2, "dev2", WORD, 0, NONE, 0, "raw word: old numeric command lines, and the -DTTRNN_ABLATIONS chain kernels' switches (bits 16 and up)") \
  X(FP32_MATH, "fp32_math", MATH, TTRNN_MATH_SPLIT, NONE, 0, "exact | split: how fp32 operands are multiplied")                 \
  X(FORCE_GENERIC, "force_generic", BOOL, 0, NONE, 0, "any-shape VALU kernels for everything")                                   \
  X(NO_GEMM, "no_gemm", BOOL, 0, NONE, 0, "batched projections / gradients through the TT chain kernels")                        \
  X(NO_IN1, "no_in1", BOOL, 0, NONE, 0, "no input_size == 1 shortcut")                                                           \
  X(NO_F10, "no_f10", BOOL, 0, NONE, 0, "no fused-core kernels (stage-wise MFMA kernels instead)")                               \
  X(NO_G2, "no_g2", BOOL, 0, NONE, 0, "no runtime-shape two-stage MFMA kernels (any-shape VALU kernels instead)")                \
  X(FORCE_G2, "force_g2", BOOL, 0, NONE, 0, "runtime-shape kernels even where a shape-specialised kernel exists")                \
  X(DIAG, "diag", BOOL, 0, NONE, 0, "diagnostic builds with s_memtime stamps")                                                   \
  X(BF16_FP32_MFMA, "bf16_fp32_mfma", BOOL, 0, NONE, 0, "bf16 storage on the fp32 MFMA kernels")                                 \
  X(BIG_MERGE, "big_merge", R02, 2, NONE, 0, "pairs of cores contracted per launch (big shape)")                                 \
  X(BIG_NO_GEMM, "big_no_gemm", BOOL, 0, NONE, 0, "big shape: no batched GEMM")                                                  \
  X(BIG_NO_PAIR, "big_no_pair", BOOL, 0, NONE, 0, "big shape: one workgroup per sample")                                         \
  X(NO_BIGB, "no_bigb", BOOL, 0, NONE, 0, "any-shape backward for the big shape")                                                \
  X(BIGW_SLICES, "bigw_slices", BOOL, 0, NONE, 0, "big shape: weight gradient in slices")                                        \
  X(F10_NB1, "f10_nb1", BOOL, 0, NONE, 0, "one sample per workgroup even when B > #CUs")                                         \
  X(DENSE_FP32, "dense_fp32", BOOL, 0, NONE, 0, "dense weight gradient on the fp32 MFMA")                                        \
  X(F10_NB2, "f10_nb2", BOOL, 0, NONE, 0, "B > #CUs: two samples per eight-wave workgroup instead of four-wave workgroups")      \
  X(GEMM_PIECES, "gemm_pieces", S023, 0, NONE, 0, "forward input-projection GEMMs: 0 by size, 2 two fp16 pieces, 3 three bf16 pieces") \
  X(BIG_FP32_MFMA, "big_fp32_mfma", BOOL, 0, NONE, 0, "big-shape pair kernel on the fp32 MFMA even in split mode")               \
  X(PAIR_FAULT, "pair_fault", BOOL, 0, NONE, 0, "tests only: forward pair kernels one workgroup short (exercises the time-out path)") \
  X(NO_GEMM3, "no_gemm3", BOOL, 0, NONE, 0, "two-piece fp16 K-in GEMM, x split on the fly, instead of the pre-split LDS-DMA GEMM") \
  /* ---- A/B route switches between kernels that compute the same result ---- */                                                \
  X(GEMM3_PINGPONG, "gemm3_pingpong", BOOL, 0, DEV, 1, "gemm3: the ping-pong schedule")                                          \
  X(F10GQ_BF16, "f10gq_bf16", BOOL, 0, DEV, 4, "bf16 TT-GRU forward on k_gru_fwd_f10gq (measured slower)")                       \
  X(GRU_EIGHT_WAVE, "gru_eight_wave", BOOL, 0, DEV, 32, "fused-core GRU forward: the eight-wave kernel instead of four waves with S2 in the gate waves") \
  X(GEMM3_WG_PER_TILE, "gemm3_wg_per_tile", BOOL, 0, DEV, 64, "gemm3: one workgroup per tile instead of the persistent grid")    \
  X(F10BL_ALWAYS, "f10bl_always", BOOL, 0, DEV, 128, "wave-local fused-core reverse LSTM kernel (k_lstm_bwd_f10l) whatever the batch") \
  X(GRU_FWD_ON_TIER, "gru_fwd_on_tier", BOOL, 0, DEV, 256, "fp32 TT-GRU forward on the runtime tier instead of k_gru_fwd_f10vh / its H = 512 kin") \
  X(F10S, "f10s", BOOL, 0, DEV, 512, "single-barrier LSTM forward kernel k_lstm_fwd_f10s instead of k_lstm_fwd_f10q (measured slower)") \
  X(NO_PROJ3, "no_proj3", BOOL, 0, DEV, 1024, "dense weight gradient pulled back by the fused-core wgrad kernel on unit rows, not the three-core launches") \
  X(G2_BWD_HEAD_STREAMED, "g2_bwd_head_streamed", BOOL, 0, DEV, 2048, "tier reverse kernel: head^T fragments of per-gate sets streamed, not resident") \
  X(G2_FOUR_WAVE_STREAMED, "g2_four_wave_streamed", BOOL, 0, DEV, 4096, "tier: four-wave streamed plans where the eight-wave plan would keep the head resident") \
  X(H512_FWD_ON_TIER, "h512_fwd_on_tier", BOOL, 0, DEV, 8192, "H = 512 r = 8 forward recurrence on the runtime tier")            \
  X(H512_BWD_ON_TIER, "h512_bwd_on_tier", BOOL, 0, DEV, 16384, "H = 512 r = 8 reverse recurrence on the runtime tier")           \
  X(F10BL_NEVER, "f10bl_never", BOOL, 0, DEV, 32768, "four-barrier eight-wave fused-core reverse LSTM kernel whatever the batch") \
  X(NO_FUSED_SETUP, "no_fused_setup", BOOL, 0, DEV, 1 << 16, "no fused set-up launch (ttrnn_rnn_forward_cores = pack + forward)") \
  X(F10P, "f10p", BOOL, 0, DEV, 1 << 17, "k_lstm_bwd_f10p (gate factors precomputed by the helper waves) instead of k_lstm_bwd_f10h (measured slower)") \
  X(HEAD_SPLIT_EPILOGUE, "head_split_epilogue", BOOL, 0, DEV, 1 << 18, "head forward as chain + separate epilogue launch")       \
  X(G2_PAIR_NEVER, "g2_pair_never", BOOL, 0, DEV, 1 << 19, "tier: never the two-samples-per-workgroup forward kernel k_g2_fwd_p") \
  X(G2_PAIR_ALWAYS, "g2_pair_always", BOOL, 0, DEV, 1 << 20, "tier: k_g2_fwd_p for every batch of two or more")                  \
  X(G2_BWD_FOUR_WAVE, "g2_bwd_four_wave", BOOL, 0, DEV, 1 << 21, "tier reverse kernel on four-wave workgroups even where only one fits a CU") \
  X(G2_BWD_T2_GENERAL, "g2_bwd_t2_general", BOOL, 0, DEV, 1 << 22, "tier reverse kernel: streamed T2 on the general per-position loop") \
  X(NO_PROJ4, "no_proj4", BOOL, 0, DEV, 1 << 23, "d = 4 dense weight gradient pulled back by the any-shape chain kernel on identity rows") \
  X(G2_DENSE_FROM_MERGED, "g2_dense_from_merged", BOOL, 0, DEV, 1 << 24, "tier: K-in dense matrix from the merged cores (k_g2_dense; no difference measured)") \
  X(NAIVE_FWD_ON_TIER, "naive_fwd_on_tier", BOOL, 0, DEV, 1 << 25, "naive TT-LSTM / TT-GRU H = 256 forward on the runtime tier instead of k_rnn_fwd_f10n") \
  X(GRU_R16_BWD_STAGEWISE, "gru_r16_bwd_stagewise", BOOL, 0, DEV, 1 << 26, "TT-GRU r = 16 reverse recurrence on the stage-wise kernel") \
  X(G2_NO_CIN, "g2_no_cin", BOOL, 0, DEV, 1 << 27, "tier forward plans without column tiles inside a stage-2 unit (G2Mat::cin)")  \
  X(DENSE_ONE_ROUND_RULE, "dense_one_round_rule", BOOL, 0, DEV, 1 << 28, "dense weight gradient: row ranges by the one-round rule everywhere") \
  X(G2_BWD_ONE_TILE, "g2_bwd_one_tile", BOOL, 0, DEV, 1 << 29, "tier reverse kernel resident for one column tile only")          \
  X(NO_CHAIN_WGRAD, "no_chain_wgrad", BOOL, 0, DEV2, 1, "no chain weight gradient (ttrnn_rnn_wgrad_workspace answers 0)")        \
  X(CHAIN_WGRAD_HID_ONLY, "chain_wgrad_hid_only", BOOL, 0, DEV2, 2, "chain weight gradient for the hidden matrix only")          \
  X(C2_RUNTIME_PLAN, "c2_runtime_plan", BOOL, 0, DEV2, 4, "chain kernel with the run-time plan even where a compile-time instantiation exists") \
  X(CHAIN_WGRAD_LARGE, "chain_wgrad_large", BOOL, 0, DEV2, 8, "offer the chain kernel's large variant too (measured slower; tests only)") \
  X(ENC_FWD_ON_TIER, "enc_fwd_on_tier", BOOL, 0, DEV2, 16, "speaker encoder's shape forward on the runtime tier instead of k_lstm_fwd_w2") \
  X(ENC_BWD_ON_TIER, "enc_bwd_on_tier", BOOL, 0, DEV2, 32, "the same for the reverse-time kernel")                               \
  X(C2R_OFF, "c2r_off", BOOL, 0, DEV2, 64, "k_c2w (C1 / dC1 images in LDS) for the calls k_c2r (register hand-offs) would take") \
  X(GRU_R16_BWD_ON_TIER, "gru_r16_bwd_on_tier", BOOL, 0, DEV2, 128, "TT-GRU H = 256 r = 16 reverse recurrence on the tier's kernel") \
  X(GRU_H512_BWD_ON_TIER, "gru_h512_bwd_on_tier", BOOL, 0, DEV2, 256, "TT-GRU H = 512 r = 8 reverse recurrence on the tier's kernel") \
  X(NAIVE_BWD_ON_TIER, "naive_bwd_on_tier", BOOL, 0, DEV2, 512, "naive per-gate sets of H = 256 on the tier's reverse kernel instead of k_rnn_bwd_f10n") \
  X(F10BH_NO_WL, "f10bh_no_wl", BOOL, 0, DEV2, 1024, "four-barrier fused-core LSTM reverse kernel instead of its wave-local form") \
  X(F10T_OFF, "f10t_off", BOOL, 0, DEV2, 2048, "k_lstm_fwd_f10q (core 2 first) for the calls k_lstm_fwd_f10t (cores 0·1 first) would take") \
  X(F10T_R7_LOOP, "f10t_r7_loop", BOOL, 0, DEV2, 4096, "k_lstm_fwd_f10t with round 7's time loop (pieces eight MFMA rows apart, fold by v_permlane32_swap)")

namespace ttrnn {

enum OptId {
#define TTRNN_OPT_ID(id, name, kind, def, word, mask, desc) OPT_##id,
  TTRNN_OPTIONS(TTRNN_OPT_ID)
#undef TTRNN_OPT_ID
  OPT_COUNT, OPT_NONE = OPT_COUNT
};
// what -DTTRNN_ABLATIONS builds read of the raw words: result-destroying ablations, by number only (the gemm3 and dense-gradient
// kernels take all of `dev` as an argument and test bits 2 / 8 / 16 / 32 / 64 of it themselves)
constexpr int DEV_ABLATIONS = 8 | 16 | 32 | 64;
constexpr int DEV2_ABLATIONS_SHIFT = 16;      // the chain kernels' switches: dev2 >> 16

int opt(OptId id);                       // current value
const char* opt_name(OptId id);          // "fp32_math", "force_generic", ...
int opt_set(const char* name, int value);   // 0 or -1 (unknown name / bad value)
int opt_get(const char* name, int* value);

}  // namespace ttrnn
