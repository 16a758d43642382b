// Fused dot-product attention with edge features (graphop_attention_edge_*): the edge row xe[e], indexed
// by edge id, is added to the key AND the value of edge e = (i, j):
//   kx_e  = K_j + xe[e]          vx_e = V_j + xe[e]             (each formed once per piece, in this order, in every pass)
//   s_ek  = <Q_ik, kx_ek>        a_ek = exp(s_ek - m_ik) / l_ik,   o_ik = sum_e a_ek mult_ek vx_ek
//   ds_ek = a_ek (mult_ek <dO_ik, vx_ek> - D_ik)
//   dQ_i  = sum_e ds_e kx_e      dK_j = sum_e ds_e Q_i             dV_j = sum_e a_e mult_e dO_i
//   dxe[e] = ds_e Q_i + a_e mult_e dO_i
// The fast kernels are the several-head chunk-driver passes (kernels_attn_rows_passes.inc) with the edge
// row of 4.5i streamed per slot, under this op's names; the row pass stores dxe[e * F4 + p] with one plain float4 per
// lane and real slot.  H = 1 (1 x 64) is an instantiation like the others.  The generic kernels (one wave per chunk,
// fp32 / fp64, any h and d, any chunk layout; kernels_attn_edge_generic.inc, shared with kernels_attn_etype.h) cover
// every other valid call.
// This header emits kernels under fixed names, one of them (k_attn_edge_piece_max) no template, so it belongs to exactly
// one translation unit (attention_edge.hip).  The text it shares with the other forms lives in the two .inc files.
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

#define AR_EDGE 1
#define AR_KERNEL(pass) k_attn_edge_##pass
#define AR_TYPE(name) AttnEdge##name
#define AR_FN(name) attn_edge_##name
#include "kernels_attn_rows_passes.inc"
#include "kernels_attn_edge_generic.inc"
#undef AR_EDGE
#undef AR_KERNEL
#undef AR_TYPE
#undef AR_FN

}  // namespace graphop
