// Fused dot-product attention with edge features (graphop_attention_edge_*): the edge row xe[e], indexed
// by edge id, is added to the key AND the value of edge e = (i, j):
//   kx_e  = K_j + xe[e]          vx_e = V_j + xe[e]             (each formed once per piece, in this order, in every pass)
//   s_ek  = <Q_ik, kx_ek>        a_ek = exp(s_ek - m_ik) / l_ik,   o_ik = sum_e a_ek mult_ek vx_ek
//   ds_ek = a_ek (mult_ek <dO_ik, vx_ek> - D_ik)
//   dQ_i  = sum_e ds_e kx_e      dK_j = sum_e ds_e Q_i             dV_j = sum_e a_e mult_e dO_i
//   dxe[e] = ds_e Q_i + a_e mult_e dO_i
// The fast kernels are the several-head chunk-driver passes (kernels_attn_rows_passes.inc) with the edge
// row of 4.5i streamed per slot, under this op's names; the row pass stores dxe[e * F4 + p] with one plain float4 per
// lane and real slot.  H = 1 (1 x 64) is an instantiation like the others.  The generic kernels below (one wave per
// chunk, fp32 / fp64, any h and d, any chunk layout) cover every other valid call.
// This header emits kernels under fixed names, one of them (k_attn_edge_piece_max) no template, so it belongs to exactly
// one translation unit (attention_edge.hip).  The text it shares with kernels_attn_heads.h lives in the .inc.
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

#define AR_EDGE 1
#define AR_KERNEL(pass) k_attn_edge_##pass
#define AR_TYPE(name) AttnEdge##name
#define AR_FN(name) attn_edge_##name
#include "kernels_attn_rows_passes.inc"
#undef AR_EDGE
#undef AR_KERNEL
#undef AR_TYPE
#undef AR_FN

// ---- the generic passes: fp32 / fp64, any h and d, any chunk layout; one wave per chunk ------------------------------
// s of one (slot, head): q = Q[i, k, :], kj = K[j, k, :], e = xe[eid, k, :].  Every generic pass evaluates it by this
// function, so a recomputed score is bitwise the one the statistics were taken from.
template <typename T>
__device__ __forceinline__ T attn_edge_score(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ e,
                                             i64 d) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += q[c] * (kj[c] + e[c]);
  return s;
}

// stats[i, k] = (-1e9, 0): the floor of the maxima, the start of the sums, and what rows without slots keep
template <typename T>
__global__ void k_attn_edge_stats_init_generic(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { stats[i * 2] = (T)-1e9; stats[i * 2 + 1] = (T)0; }
}
// the sums become 1 / l
template <typename T>
__global__ void k_attn_edge_stats_fin_generic(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const T s = stats[i * 2 + 1]; stats[i * 2 + 1] = s > (T)0 ? (T)1 / s : (T)0; }
}

// lanes over the chunk's slots, one head at a time; SUM = false: the maxima, true: the sums of exp(s - m)
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void k_attn_edge_stats_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ xe,
    T* __restrict__ stats, i64 n_chunks, i64 h, i64 d) {
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
      const T s = attn_edge_score<T>(Q + (r * h + k) * d, K + (indices[j] * h + k) * d, xe + (eid[j] * h + k) * d, d);
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

// lanes over the h * d elements of the row in steps of the wave; one atomic per (chunk, element).  DROP (here and in
// the two backward kernels): one drop_mult per use, for global head head0 + k.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_edge_fwd_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ xe, const T* __restrict__ stats, T* __restrict__ o, i64 n_chunks, i64 h, i64 d, i64 head0,
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
    const T m = stats[(r * h + k) * 2], il = stats[(r * h + k) * 2 + 1];
    T acc = 0;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j], e = eid[j];
      const T s = attn_edge_score<T>(Q + (r * h + k) * d, K + (src * h + k) * d, xe + (e * h + k) * d, d);
      T w = exp_t(s - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, head0 + k, dr);
      acc += w * (V[src * f + it] + xe[e * f + it]);
    }
    atomicAdd(o + r * f + it, acc);
  }
}

// P[i, k] = (m, 1 / l, D = <dO_ik, o_ik>, 0)
template <typename T>
__global__ void k_attn_edge_pack_generic(const T* __restrict__ stats, const T* __restrict__ dO, const T* __restrict__ o,
                                         T* __restrict__ P, i64 n, i64 d) {   // n = n_q * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T dsum = 0;
  for (i64 c = 0; c < d; ++c) dsum += dO[i * d + c] * o[i * d + c];
  P[i * 4] = stats[i * 2]; P[i * 4 + 1] = stats[i * 2 + 1]; P[i * 4 + 2] = dsum; P[i * 4 + 3] = 0;
}

// ds of one (slot, head): p = P[i, k] holds (m, 1 / l, D); *a_out = a_e; mult = the slot's dropout multiplier
template <typename T>
__device__ __forceinline__ T attn_edge_ds(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ vj,
                                          const T* __restrict__ e, const T* __restrict__ p, const T* __restrict__ dO_ik,
                                          i64 d, T mult, T* a_out) {
  const T s = attn_edge_score<T>(q, kj, e, d);
  const T a = exp_t(s - p[0]) * p[1];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += dO_ik[t] * (vj[t] + e[t]);
  *a_out = a;
  return a * (mult * da - p[2]);
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_edge_bwd_row_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ xe, const T* __restrict__ P, const T* __restrict__ dO, T* __restrict__ dQ, T* __restrict__ dxe,
    i64 n_chunks, i64 h, i64 d, i64 head0, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    const T q = Q[r * f + it], g = dO[r * f + it];
    T acc = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j], e = eid[j];
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, head0 + k, dr);
      const T ds = attn_edge_ds<T>(Q + (r * h + k) * d, K + (src * h + k) * d, V + (src * h + k) * d,
                                   xe + (e * h + k) * d, P + (r * h + k) * 4, dO + (r * h + k) * d, d, mult, &aij);
      acc += ds * (K[src * f + it] + xe[e * f + it]);
      if (dxe != nullptr) dxe[e * f + it] = ds * q + aij * mult * g;   // a slot is visited once
    }
    atomicAdd(dQ + r * f + it, acc);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_edge_bwd_col_generic(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ xe, const T* __restrict__ P, const T* __restrict__ dO, T* __restrict__ dK, T* __restrict__ dV,
    i64 n_chunks, i64 h, i64 d, i64 head0, DropArgsIf<DROP, T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 jc = col[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  if (j1 <= j0) return;
  const i64 f = h * d;
  for (i64 it = lane; it < f; it += kWave) {
    const i64 k = it / d;
    T acc_k = 0, acc_v = 0, aij;
    for (i64 j = j0; j < j1; ++j) {
      const i64 i = indices[j], e = eid[j];
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, head0 + k, dr);
      const T ds = attn_edge_ds<T>(Q + (i * h + k) * d, K + (jc * h + k) * d, V + (jc * h + k) * d,
                                   xe + (e * h + k) * d, P + (i * h + k) * 4, dO + (i * h + k) * d, d, mult, &aij);
      acc_k += ds * Q[i * f + it];
      acc_v += aij * mult * dO[i * f + it];
    }
    atomicAdd(dK + jc * f + it, acc_k);
    atomicAdd(dV + jc * f + it, acc_v);
  }
}

}  // namespace graphop
