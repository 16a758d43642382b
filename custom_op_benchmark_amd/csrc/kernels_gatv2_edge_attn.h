// Fused GATv2 attention with edge features (extra op, not in the reference; gatv2_edge_attention.hip has the entry
// points): the layer of kernels_gatv2_attn.h with one more row inside the LeakyReLU, for edge e = (i, j):
//   z_ijc = (xl[i, k, c] + xr[j, k, c]) + xe[e, k, c]   (in this order, in every pass),   s_ij = sum_c att[k, c] LeakyReLU(z_ijc)
// xe (n_edges, h, d) is indexed by EDGE ID, so a slot reads the row xe[eid[slot]].  The backward is that of
// kernels_gatv2_attn.h with z as above, plus one output: dxe[e, k, c] = ds_ij att[k, c] t_ijc, the only edge-sized
// tensor written, one plain float4 store per lane and slot from the row-major pass, where every slot is visited once.
// The gather passes are the text of kernels_gatv2_attn_passes.inc compiled twice more with the edge row, as
// k_gv2edge_<pass>_f32 (no dropout) and k_gv2edrop_<pass>_f32 (dropout); the generic ones that of
// kernels_gatv2_attn_generic.inc, as k_gv2edge_<pass>_generic<T, DROP>.  k_gv2attn_pack_*, k_gv2attn_datt_fin_f32 and the
// generic stats init / finish are launched unchanged: P = (m, 1 / l, D, 0) still holds.
// z is formed once per piece (gv2edge_z4) and the score comes from z by ONE expression (gv2edge_dot4) in all three
// passes and both orientations, so a recomputed s is bitwise the forward's.  The xe piece is consumed where z is formed:
// the forward keeps only xr_j for the aggregation, the two backward passes only z (for t and LeakyReLU(z)) once the
// partial s and da exist, so no pass holds a second [SB][NV] array.
// A NULL eid in a row-major pass means eid[slot] == slot (a plan with eid_identity): a kernel-uniform branch.  The
// column pass always reads eid_c; its xe rows are a random read, which is inherent to an edge-id-indexed operand.
#pragma once
#include "kernels_gatv2_attn.h"

namespace graphop {

// z of one piece: (a + b) + e, component by component
__device__ __forceinline__ float4 gv2edge_z4(const float4& a, const float4& b, const float4& e) {
  return make_float4((a.x + b.x) + e.x, (a.y + b.y) + e.y, (a.z + b.z) + e.z, (a.w + b.w) + e.w);
}

// sum_i w_i * LeakyReLU(z_i) over the four components of a piece, in the order of gv2attn_dot4
__device__ __forceinline__ float gv2edge_dot4(const float4& w, const float4& z, float s) {
  return fmaf(w.w, gv2attn_lrelu(z.w, s),
              fmaf(w.z, gv2attn_lrelu(z.z, s), fmaf(w.y, gv2attn_lrelu(z.y, s), w.x * gv2attn_lrelu(z.x, s))));
}

#define GV2_EDGE 1
#define GV2_DROP false
#define GV2_KERNEL(pass) k_gv2edge_##pass##_f32
#include "kernels_gatv2_attn_passes.inc"
#undef GV2_DROP
#undef GV2_KERNEL
#define GV2_DROP true
#define GV2_KERNEL(pass) k_gv2edrop_##pass##_f32
#include "kernels_gatv2_attn_passes.inc"
#undef GV2_DROP
#undef GV2_KERNEL

#define GV2_GKERNEL(pass) k_gv2edge_##pass##_generic
#define GV2_GFN(name) gv2edge_##name
#include "kernels_gatv2_attn_generic.inc"
#undef GV2_GKERNEL
#undef GV2_GFN
#undef GV2_EDGE

}  // namespace graphop
