// Fused GATv2 attention (extra op, not in the reference; gatv2_attention.hip has the entry points): the layer
//   z_ijc = xl[i, k, c] + xr[j, k, c],  s_ij = sum_c att[k, c] LeakyReLU(z_ijc),  a = row-softmax(s),
//   o[i, k, :] = sum_j a_ij xr[j, k, :]                                                         (per head k)
// and its backward WITHOUT any E-sized tensor.  The aggregated table is the gathered one (the GATv2Conv convention), so
// the row xr[j] a pass fetches for the score is the row it aggregates: one row gather per slot and pass.  The forward
// leaves o and the row statistics (m_i, 1 / l_i); the backward recomputes z, s and a per slot from them:
//   D_i = <dO_i, o_i>,  da_ij = <dO_i, xr_j>,  ds_ij = a_ij (da_ij - D_i),  t_ijc = (z_ijc > 0 ? 1 : slope)
//   dxl[i, k, c] = att[k, c] sum_j ds_ij t_ijc                      datt[k, c] = sum_ij ds_ij LeakyReLU(z_ijc)
//   dxr[j, k, c] = sum_i (ds_ij att[k, c] t_ijc + a_ij dO[i, k, c])
// Passes (fp32 fast forms; k_gv2attn_*_generic<T> below cover fp64, other shapes, NULL plans and any chunk order):
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

// datt[p] = sum over the n_part rows of the row pass's partials, piece p = blockIdx.x: each thread sums its rows in
// order, then the workgroup's 256 sums are added in a fixed tree
__global__ __launch_bounds__(kFastBlock) void k_gv2attn_datt_fin_f32(const float4* __restrict__ part,
                                                                     float4* __restrict__ datt, i64 n_part, int f4) {
  __shared__ float4 red[kFastBlock / kWave];
  const int p = blockIdx.x;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (i64 i = threadIdx.x; i < n_part; i += kFastBlock) {
    const float4 o = part[i * f4 + p];
    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
  }
  t.x = wave_sum(t.x); t.y = wave_sum(t.y); t.z = wave_sum(t.z); t.w = wave_sum(t.w);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < kFastBlock / kWave; ++q) {
      t.x += red[q].x; t.y += red[q].y; t.z += red[q].z; t.w += red[q].w;
    }
    datt[p] = t;
  }
}

// ---- generic kernels: fp32 / fp64, any h and d, any chunk layout; one wave per chunk -----------------------------
// s of one (slot, head): a = xl[i, k, :], b = xr[j, k, :], w = att[k, :].  Every generic pass evaluates it by this
// function, so a recomputed score is bitwise the one the statistics were taken from.
template <typename T>
__device__ __forceinline__ T gv2attn_score(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ w,
                                           i64 d, T slope) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += w[c] * gat_lrelu(a[c] + b[c], slope);
  return s;
}

// stats (n_l, h, 2) doubles as scratch: filled with (-1e9, 0), atomic max, atomic sum of exp(s - m), then 1 / sum.
template <typename T>
__global__ void k_gv2attn_stats_init_generic(T* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    stats[2 * i] = (T)-1e9;
    stats[2 * i + 1] = 0;
  }
}

// lanes over the chunk's slots, one head at a time
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void k_gv2attn_stats_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att, T* __restrict__ stats,
    i64 n_chunks, i64 h, i64 d, T slope) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;   // wave-uniform
  for (i64 k = 0; k < h; ++k) {
    const T m = SUM ? stats[(r * h + k) * 2] : (T)0;
    T acc = SUM ? (T)0 : (T)-1e9;
    for (i64 j = j0 + lane; j < j1; j += kWave) {
      const T s = gv2attn_score<T>(xl + (r * h + k) * d, xr + (indices[j] * h + k) * d, att + k * d, d, slope);
      if constexpr (SUM) acc += exp_t(s - m);
      else acc = s > acc ? s : acc;
    }
    for (int o = 1; o < kWave; o <<= 1) {
      const T t = __shfl_xor(acc, o);
      if constexpr (SUM) acc += t;
      else acc = t > acc ? t : acc;
    }
    if (lane == 0) {
      if constexpr (SUM) atomicAdd(stats + (r * h + k) * 2 + 1, acc);
      else atomic_max_float(stats + (r * h + k) * 2, acc);
    }
  }
}

template <typename T>
__global__ void k_gv2attn_stats_fin_generic(T* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
    const T s = stats[2 * i + 1];
    stats[2 * i + 1] = s > (T)0 ? (T)1 / s : (T)0;
  }
}

// lanes over the h * d elements of the row in steps of the wave; one atomic per (chunk, element).  DROP (here and in
// the two backward kernels): one drop_mult per use.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_gv2attn_fwd_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att, const T* __restrict__ stats,
    T* __restrict__ o, i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T m = stats[(r * h + k) * 2], il = stats[(r * h + k) * 2 + 1];
    T acc = 0;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j];
      const T s = gv2attn_score<T>(xl + (r * h + k) * d, xr + (src * h + k) * d, att + k * d, d, slope);
      T w = exp_t(s - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, k, dr);
      acc += w * xr[src * f + it];
    }
    atomicAdd(o + r * f + it, acc);
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

// ds of one (slot, head): i = the row-major row (P[i, k] holds m, 1 / l, D), j = the column; *a_out = a_ij; mult = the
// slot's dropout multiplier m_ij (1 without dropout)
template <typename T>
__device__ __forceinline__ T gv2attn_ds(const T* __restrict__ xl_ik, const T* __restrict__ xr_jk,
                                        const T* __restrict__ att_k, const T* __restrict__ p,
                                        const T* __restrict__ dO_ik, i64 d, T slope, T mult, T* a_out) {
  const T s = gv2attn_score<T>(xl_ik, xr_jk, att_k, d, slope);
  const T a = exp_t(s - p[0]) * p[1];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += dO_ik[t] * xr_jk[t];
  *a_out = a;
  return a * (mult * da - p[2]);
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_gv2attn_bwd_row_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dxl, T* __restrict__ datt, i64 n_chunks, i64 h, i64 d, T slope,
    DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T a = xl[r * f + it];
    T acc = 0, dw = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j];
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, k, dr);
      const T ds = gv2attn_ds<T>(xl + (r * h + k) * d, xr + (src * h + k) * d, att + k * d, P + (r * h + k) * 4,
                                 dO + (r * h + k) * d, d, slope, mult, &aij);
      const T z = a + xr[src * f + it];
      acc += gat_lrelu_grad(z, ds, slope);
      dw += ds * gat_lrelu(z, slope);
    }
    atomicAdd(dxl + r * f + it, acc * att[it]);
    atomicAdd(datt + it, dw);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_gv2attn_bwd_col_generic(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ att, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dxr, i64 n_chunks, i64 h, i64 d, T slope, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 jc = col[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T b = xr[jc * f + it], w = att[it];
    T acc = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 i = indices[j];
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, k, dr);
      const T ds = gv2attn_ds<T>(xl + (i * h + k) * d, xr + (jc * h + k) * d, att + k * d, P + (i * h + k) * 4,
                                 dO + (i * h + k) * d, d, slope, mult, &aij);
      if constexpr (DROP) aij *= mult;   // a_ij m_ij
      acc += gat_lrelu_grad(xl[i * f + it] + b, ds, slope) * w + aij * dO[i * f + it];
    }
    atomicAdd(dxr + jc * f + it, acc);
  }
}

}  // namespace graphop
