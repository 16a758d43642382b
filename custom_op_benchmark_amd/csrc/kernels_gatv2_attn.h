// Fused GATv2 attention (extra op, not in the reference; gatv2_attention.hip has the entry points): the layer
//   z_ijc = xl[i, k, c] + xr[j, k, c],  s_ij = sum_c att[k, c] LeakyReLU(z_ijc),  a = row-softmax(s),
//   o[i, k, :] = sum_j a_ij xr[j, k, :]                                                         (per head k)
// and its backward WITHOUT any E-sized tensor.  The aggregated table is the gathered one (the GATv2Conv convention), so
// the row xr[j] a pass fetches for the score is the row it aggregates: one row gather per slot and pass.  The forward
// leaves o and the row statistics (m_i, 1 / l_i); the backward recomputes z, s and a per slot from them:
//   D_i = <dO_i, o_i>,  da_ij = <dO_i, xr_j>,  ds_ij = a_ij (da_ij - D_i),  t_ijc = (z_ijc > 0 ? 1 : slope)
//   dxl[i, k, c] = att[k, c] sum_j ds_ij t_ijc                      datt[k, c] = sum_ij ds_ij LeakyReLU(z_ijc)
//   dxr[j, k, c] = sum_i (ds_ij att[k, c] t_ijc + a_ij dO[i, k, c])
// Passes (fp32 fast forms; k_gv2attn_*_generic<T>, below and in kernels_gatv2_attn_generic.inc, cover fp64, other
// shapes, NULL plans and any chunk order):
//   fwd    : one lane group per row segment of a row_owned plan (segments above kLongSegment slots: one workgroup
//            each), ONE pass with an online softmax: a score needs the whole xr row, so a separate statistics pass
//            would cost as much as the aggregation.  A row is never split: no atomics, o and stats bit-reproducible.
//   pack   : P[i, k] = (m, 1 / l, D, 0) as one float4 per (node, head)
//   bwd_row: chunk driver over the row-major chunks; xl_i, dO_i, P[i] and att in registers, xr_j gathered -> dxl and
//            the workgroup's row of datt partials (k_gv2attn_datt_fin_f32 sums them in a fixed order)
//   bwd_col: chunk driver over the column-major chunks; xr_j and att in registers, xl_i, dO_i and P[i] gathered -> dxr
// The lane layout is that of kernels_gat_attn.h / kernels_gatv2.h: a node row is F4 = H * D / 4 float4 pieces, a lane
// group of L = 16 lanes holds NV = F4 / L of them, piece p = v * L + l, so the DQ = D / 4 pieces of one head sit in DQ
// adjacent lanes and a per-head sum is a group_sum<DQ>.  Every lane of a head holds the head's score, so the softmax
// state (m, l) is kept per piece.  The score is evaluated by the same expression in every pass: a recomputed s is
// bitwise the forward's.
// Attention dropout (DROP; kernels_dropout.h has the decision): o[i] = sum_j a_ij m_ij xr[j] with the statistics of the
// undropped scores, da_ij = m_ij <dO_i, xr_j> and dxr[j] sums a_ij m_ij dO_i.  Each gather pass exists ONCE in source,
// in kernels_gatv2_attn_passes.inc, and is compiled twice: as k_gv2attn_* (DROP = false) and as k_gv2drop_*.  The lanes
// that load a batch's neighbour ids run Philox for their slot (gat_drop_lane_bits) and the keep
// bits travel by group_bcast like the id: no pass reads eid or any other new stream.
#pragma once
#include "kernels_base.h"
#include "kernels_gat.h"
#include "kernels_generic.h"
#include "kernels_dropout.h"

namespace graphop {

constexpr float kGv2AttnFloor = -1e9f;   // the library's softmax floor (m = max(-1e9, max_j s_ij))

template <int H, int D>
struct Gv2AttnCfg {
  static constexpr int L = 16;               // lanes per group
  static constexpr int F4 = H * D / 4;       // float4 pieces of a node row
  static constexpr int NV = F4 / L;          // pieces per lane (1, 2, 4)
  static constexpr int DQ = D / 4;           // lanes holding one head's pieces (2 .. 16)
  static constexpr int SB_FWD = 16 / NV;     // slots per batch: 16 gathered float4 pieces in flight per lane
  static constexpr int SB_ROW = 8 / NV;      // the row pass also keeps two rows of sums
  static constexpr int SB_COL = 4 / NV;      // the column pass gathers two rows and a P item per slot
  static_assert(NV * L == F4 && DQ <= L && L % DQ == 0, "unsupported (H, D)");
};

// LeakyReLU(z) = max(z, 0) + s * min(z, 0): the value of z > 0 ? z : z * s without a lane mask.  The score of a slot is
// reduced over the head's lanes between this and the selects that need the sign of z, and masks kept across that
// reduction for every gathered piece exhaust the scalar registers.
__device__ __forceinline__ float gv2attn_lrelu(float z, float s) { return fmaf(s, fminf(z, 0.f), fmaxf(z, 0.f)); }

// sum_i w_i * LeakyReLU(a_i + b_i) over the four components of a piece
__device__ __forceinline__ float gv2attn_dot4(const float4& w, const float4& a, const float4& b, float s) {
  return fmaf(w.w, gv2attn_lrelu(a.w + b.w, s),
              fmaf(w.z, gv2attn_lrelu(a.z + b.z, s),
                   fmaf(w.y, gv2attn_lrelu(a.y + b.y, s), w.x * gv2attn_lrelu(a.x + b.x, s))));
}

// two sums over aligned groups of G lanes in one sequence of lane exchanges
template <int G>
__device__ __forceinline__ void gv2attn_group_sum2(float& a, float& b) {
  if constexpr (G >= 2) { const float ta = dpp_f32<0xB1>(a), tb = dpp_f32<0xB1>(b); a += ta; b += tb; }
  if constexpr (G >= 4) { const float ta = dpp_f32<0x4E>(a), tb = dpp_f32<0x4E>(b); a += ta; b += tb; }
  if constexpr (G >= 8) { const float ta = dpp_f32<0x141>(a), tb = dpp_f32<0x141>(b); a += ta; b += tb; }
  if constexpr (G >= 16) { const float ta = dpp_f32<0x140>(a), tb = dpp_f32<0x140>(b); a += ta; b += tb; }
}

__device__ __forceinline__ void gv2attn_scale4(float4& a, float s) { a.x *= s; a.y *= s; a.z *= s; a.w *= s; }
__device__ __forceinline__ void gv2attn_fma4(float4& acc, float w, const float4& x) {
  acc.x = fmaf(w, x.x, acc.x); acc.y = fmaf(w, x.y, acc.y); acc.z = fmaf(w, x.z, acc.z); acc.w = fmaf(w, x.w, acc.w);
}

// ---- the gather passes: kernels_gatv2_attn_passes.inc, once without and once with dropout ------------------------------
// the dropout argument of a pass: dependent on H so that the undropped text may name its members in discarded branches
template <int H, bool DROP>
struct Gv2DropArg {
  using type = DropArgsIf<DROP, float>;
};

#define GV2_EDGE 0
#define GV2_DROP false
#define GV2_KERNEL(pass) k_gv2attn_##pass##_f32
#include "kernels_gatv2_attn_passes.inc"
#undef GV2_DROP
#undef GV2_KERNEL
#define GV2_DROP true
#define GV2_KERNEL(pass) k_gv2drop_##pass##_f32
#include "kernels_gatv2_attn_passes.inc"
#undef GV2_DROP
#undef GV2_KERNEL
#undef GV2_EDGE

// ---- pack: P[i, k] = (m, 1 / l, <dO_i, o_i>, 0) ---------------------------------------------------------------------
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gv2attn_pack_f32(
    const float2* __restrict__ stats, const float* __restrict__ dO, const float* __restrict__ o,
    float4* __restrict__ P, i64 n) {
  using C = Gv2AttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;   // group-uniform
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float dsum = group_sum<DQ>(dot4(ld4(dO, i * F4 + v * L + l), ld4(o, i * F4 + v * L + l)));
    if (l % DQ == 0) {
      const int k = (v * L + l) / DQ;
      const float2 st = stats[i * H + k];
      P[i * H + k] = make_float4(st.x, st.y, dsum, 0.f);
    }
  }
}

// k_gv2attn_datt_fin_f32, which sums the row pass's datt partials, is no template: it is defined in gatv2_attention.hip
// alone and launched through gv2attn_datt_fin (host_gatv2_attn_ops.h).

// ---- generic kernels: fp32 / fp64, any h and d, any chunk layout; one wave per chunk -----------------------------
// stats (n_l, h, 2) doubles as scratch: filled with (-1e9, 0), atomic max, atomic sum of exp(s - m), then 1 / sum.
template <typename T>
__global__ void k_gv2attn_stats_init_generic(T* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    stats[2 * i] = (T)-1e9;
    stats[2 * i + 1] = 0;
  }
}

template <typename T>
__global__ void k_gv2attn_stats_fin_generic(T* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const T s = stats[2 * i + 1];
    stats[2 * i + 1] = s > (T)0 ? (T)1 / s : (T)0;
  }
}

template <typename T>
__global__ void k_gv2attn_pack_generic(const T* __restrict__ stats, const T* __restrict__ dO, const T* __restrict__ o,
                                       T* __restrict__ P, i64 n, i64 d) {   // n = nodes * h
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    T s = 0;
    for (i64 x = 0; x < d; ++x) s += dO[i * d + x] * o[i * d + x];
    P[4 * i] = stats[2 * i];
    P[4 * i + 1] = stats[2 * i + 1];
    P[4 * i + 2] = s;
    P[4 * i + 3] = 0;
  }
}

// ---- the generic gather passes: kernels_gatv2_attn_generic.inc (kernels_gatv2_edge_attn.h includes it with the edge row)
#define GV2_EDGE 0
#define GV2_GKERNEL(pass) k_gv2attn_##pass##_generic
#define GV2_GFN(name) gv2attn_##name
#include "kernels_gatv2_attn_generic.inc"
#undef GV2_EDGE
#undef GV2_GKERNEL
#undef GV2_GFN

}  // namespace graphop
