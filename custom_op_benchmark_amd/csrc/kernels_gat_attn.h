// Fused GAT attention (extra op, not in the reference; gat_attention.hip has the entry points): the layer
//   s_ij = LeakyReLU(el[i] + er[j]),  a = row-softmax(s),  o[i] = sum_j a_ij V[j]          (per head k)
// and its backward WITHOUT any E-sized tensor.  The forward leaves o and the row statistics (m_i, 1 / l_i); the backward
// recomputes a per slot from them (one add, at most one multiply and one exp):
//   D_i = <dO_i, o_i>,  da_ij = <dO_i, V_j>,  ds_ij = a_ij (da_ij - D_i),  dz_ij = ds_ij * (z > 0 ? 1 : slope)
//   del[i] = sum_j dz_ij (row-major pass),  der[j] = sum_i dz_ij  and  dV[j] = sum_i a_ij dO_i (column-major pass).
// This file holds what the layer has once: the configuration, the pack kernels and the generic stats init / finish.  The
// gather passes (stats, fwd, bwd_row, bwd_col) are the text of kernels_gat_attn_passes.inc, included at the end of this
// file without the edge term and by kernels_gat_edge_attn.h with it.
// Passes (fp32 fast forms; k_gat_attn_*_generic<T> cover fp64, other shapes, NULL plans and any chunk order):
//   stats  : one lane group per row segment of a row_owned plan (rows above kLongSegment slots: one workgroup each),
//            online max / sum over the gathered er[j] only -> stats (n_l, h, 2)
//   fwd    : chunk driver (k_attn_bwd_rows_f32's form): el_i, (m_i, 1/l_i) and the output row stay in registers while
//            the row is unchanged; per slot er_j and V_j are gathered; OWNED rows are stored, split rows added
//   pack   : P[i, k] = (el, m, 1/l, D) as one float4 per (node, head)
//   bwd_row: chunk driver over the row-major chunks, dO_i and P[i] in registers, gathers er_j and V_j -> del
//   bwd_col: chunk driver over the column-major chunks, V_j and er_j in registers, gathers P[i] and dO_i -> der, dV
// A row of V / o / dO is F4 = H * D / 4 float4 pieces; a lane group of L = 16 lanes holds NV = F4 / L of them, piece
// p = v * L + l, so the DQ = D / 4 pieces of one head sit in DQ adjacent lanes: a per-head dot product is a
// group_sum<DQ>.  Partial sums leave at most once per (lane group, row, head): never one atomic per edge.
#pragma once
#include "kernels_base.h"
#include "kernels_gat.h"
#include "kernels_generic.h"
#include "kernels_dropout.h"

namespace graphop {

constexpr float kGatAttnFloor = -1e9f;   // the library's softmax floor (m = max(-1e9, max_j s_ij))

template <int H, int D>
struct GatAttnCfg {
  static constexpr int L = 16;               // lanes per group
  static constexpr int F4 = H * D / 4;       // float4 pieces of a node row
  static constexpr int NV = F4 / L;          // pieces per lane (1, 2, 4)
  static constexpr int DQ = D / 4;           // lanes holding one head's pieces (2 .. 16)
  static constexpr int SB_FWD = 16 / NV;     // slots per batch: 16 gathered float4 pieces in flight per lane
  static constexpr int SB_BWD = 8 / NV;      // the backward passes also gather er / P per piece
  static_assert(NV * L == F4 && DQ <= L && L % DQ == 0, "unsupported (H, D)");
};

// head of lane l's piece v
template <int H, int D>
__device__ __forceinline__ int gat_attn_head(int v, int l) {
  using C = GatAttnCfg<H, D>;
  return (v * C::L + l) / C::DQ;
}

// (m, l) of one head merged with (m2, l2): online softmax
__device__ __forceinline__ void gat_attn_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = s * exp_nonpos(m - mn) + s2 * exp_nonpos(m2 - mn);
  m = mn;
}

// ---- pack: P[i, k] = (el, m, 1/l, <dO, o>) ---------------------------------------------------------------------
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_pack_f32(
    const float* __restrict__ el, const float2* __restrict__ stats, const float* __restrict__ dO,
    const float* __restrict__ o, float4* __restrict__ P, i64 n) {
  using C = GatAttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;   // group-uniform
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float4 g = reinterpret_cast<const float4*>(dO)[i * F4 + v * L + l];
    const float4 y = reinterpret_cast<const float4*>(o)[i * F4 + v * L + l];
    const float dsum = group_sum<DQ>(dot4(g, y));
    if (l % DQ == 0) {
      const int k = gat_attn_head<H, D>(v, l);
      const float2 st = stats[i * H + k];
      P[i * H + k] = make_float4(el[i * H + k], st.x, st.y, dsum);
    }
  }
}

// ---- generic kernels: fp32 / fp64, any h and d, any chunk layout -------------------------------------------------
// stats (n_l, h, 2) doubles as scratch: filled with (-1e9, 0), atomic max, atomic sum of exp(s - m), then 1 / sum.
template <typename T>
__global__ void k_gat_attn_stats_init_generic(T* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    stats[2 * i] = (T)-1e9;
    stats[2 * i + 1] = 0;
  }
}

template <typename T>
__global__ void k_gat_attn_stats_fin_generic(T* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const T s = stats[2 * i + 1];
    stats[2 * i + 1] = s > (T)0 ? (T)1 / s : (T)0;
  }
}

template <typename T>
__global__ void k_gat_attn_pack_generic(const T* __restrict__ el, const T* __restrict__ stats,
                                        const T* __restrict__ dO, const T* __restrict__ o, T* __restrict__ P,
                                        i64 n, i64 d) {   // n = nodes * h
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    T s = 0;
    for (i64 x = 0; x < d; ++x) s += dO[i * d + x] * o[i * d + x];
    P[4 * i] = el[i];
    P[4 * i + 1] = stats[2 * i];
    P[4 * i + 2] = stats[2 * i + 1];
    P[4 * i + 3] = s;
  }
}

// ---- the gather passes without an edge term: k_gat_attn_{stats, fwd, bwd_row, bwd_col}_{f32, generic} ---------------
#define GA_EDGE 0
#define GA_KERNEL(pass, kind) k_gat_attn_##pass##_##kind
#define GA_FN(name) gat_attn_##name
#include "kernels_gat_attn_passes.inc"
#undef GA_EDGE
#undef GA_KERNEL
#undef GA_FN

}  // namespace graphop
