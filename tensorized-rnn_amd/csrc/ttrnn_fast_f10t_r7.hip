// ttrnn_fast_f10t_r7.hip — round 7's time loop of k_lstm_fwd_f10t (a unit's two fp16 pieces eight rows apart in stage 1's A operand,
// one v_permlane32_swap per register to fold them), kept selectable behind option f10t_r7_loop for A/B against the default loop of
// ttrnn_fast_f10t.hip.  A translation unit of its own because that file is built with -fno-slp-vectorize, under which THIS loop is
// 1.3 % slower than it was (profiles/r8/ab_cfg2_f10t_loop.txt): here the plain flags, the code of round 7 instruction for instruction.
#include "ttrnn_f10t_kernel.h"

namespace ttrnn {

int launch_rnn_fwd_f10_t_r7(const RnnShape& rs, GinSrc gin, const void* h0, const void* c0, const float* packed_hid,
                            const void* ws, const float* bias_hid, void* out, void* hT, void* cT, float* reserve,
                            hipStream_t stream) {
  using S = ShpH256R8L;
  if (!shape_matches<S>(rs.hid_s)) return TTRNN_ERR_UNSUPPORTED;
  return launch_f10t<S, false>(rs, gin, h0, c0, packed_hid, reinterpret_cast<const float*>(ws), bias_hid, out, hT, cT, reserve, stream);
}

}  // namespace ttrnn
