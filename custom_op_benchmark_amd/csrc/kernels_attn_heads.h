// Several-head forms of the fused dot-product attention kernels (graphop_attention_*, _dropout_*, _bias_*; DESIGN.md
// 4.5l): the chunk-driver forward (k_attn_bias_fwd_rows_f32) and backward (k_attn_bias_bwd_rows_f32) restated for a row
// of F = H * D floats in the layout of the fused GAT layer (AttnRowsCfg<H, D>, kernels_attn_rows.h):
//   s_ek  = <Q_ik, K_jk> (+ b[e, k])           e = (i, j), b (E, H) by edge id
//   a_ek  = exp(s_ek - m_ik) / l_ik,   o_ik = sum_e a_ek mult_ek V_jk      (mult: dropout multiplier of global head head0 + k)
//   ds_ek = a_ek (mult_ek <dO_ik, V_jk> - D_ik),   db[e, k] = ds_ek,   dQ, dK from ds, dV from a * mult
// The one-head kernels keep their text; nothing is shared with them but the helpers.
// This header emits kernels under fixed names, one of them (k_attn_heads_piece_max) no template, so it belongs to exactly
// one translation unit (attention_heads.hip).  The text it shares with kernels_attn_edge.h lives in the .inc.
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

#define AR_EDGE 0
#define AR_KERNEL(pass) k_attn_heads_##pass
#define AR_TYPE(name) AttnHeads##name
#define AR_FN(name) attn_heads_##name
#include "kernels_attn_rows_passes.inc"
#undef AR_EDGE
#undef AR_KERNEL
#undef AR_TYPE
#undef AR_FN

}  // namespace graphop
