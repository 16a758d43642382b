// Fused dot-product attention with edge-type embeddings (graphop_attention_etype_*): edge e = (i, j)
// carries a category t_e = etype[e] (by edge id), and the table row R[t_e] is added to its key AND its value:
//   kx_e  = K_j + R[t_e]         vx_e = V_j + R[t_e]            (each formed once per piece, in this order, in every pass)
//   everything else as kernels_attn_edge.h with xe[e] := R[t_e]
//   dR[t] = sum_{e : t_e = t} (ds_e Q_i + a_e mult_e dO_i)
// Nothing edge-sized exists but the int32 per edge.  Every kernel clamps the type into [0, n_types - 1] (one min on the
// unsigned value) before it forms an address: an out-of-range type gives an undefined value and touches no memory
// outside R / dR.  The fast kernels are the third inclusion of kernels_attn_rows_passes.inc, which says how the row pass
// sums dR on chip; k_attn_etype_dr_reduce sums the replicas it leaves.  The generic kernels (one wave per chunk, fp32 /
// fp64, any h and d, any chunk layout, any n_types; kernels_attn_edge_generic.inc, shared with kernels_attn_edge.h)
// cover every other valid call.
// This header emits kernels under fixed names, one of them (k_attn_etype_piece_max) no template, so it belongs to exactly
// one translation unit (attention_etype.hip).
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

#define AR_EDGE 2
#define AR_KERNEL(pass) k_attn_etype_##pass
#define AR_TYPE(name) AttnEtype##name
#define AR_FN(name) attn_etype_##name
#include "kernels_attn_rows_passes.inc"

// The fast row pass holds 4 T F bytes of LDS when dR is wanted; beyond this many bytes that pass alone is the generic one.
constexpr i64 kAttnEtypeTableBytes = 16384;
constexpr i64 attn_etype_max_types(i64 F) { return F > 0 ? kAttnEtypeTableBytes / (4 * F) : 0; }   // kAttnEtypeMaxTypes
// Replicas of dR the row pass's workgroups add into (blockIdx.x % kAttnEtypeReplicas): 64 KiB to 1 MiB of workspace.
constexpr int kAttnEtypeReplicas = 64;

// dR[i] = sum over the replicas of rep[r][i]; every element of dR is written
__global__ void k_attn_etype_dr_reduce(const float* __restrict__ rep, float* __restrict__ dR, int n, int nrep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int r = 0; r < nrep; ++r) acc += rep[(i64)r * n + i];
  dR[i] = acc;
}

// the type of edge id e, clamped: the one place a generic pass reads etype
__device__ __forceinline__ i64 attn_etype_of(const int* __restrict__ etype, i64 e, unsigned tmax) {
  return (i64)min((unsigned)etype[e], tmax);
}

#include "kernels_attn_edge_generic.inc"
#undef AR_EDGE
#undef AR_KERNEL
#undef AR_TYPE
#undef AR_FN

}  // namespace graphop
