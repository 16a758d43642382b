// Fused dot-product attention with edge-type embeddings (graphop_attention_etype_*): edge e = (i, j)
// carries a category t_e = etype[e] (by edge id), and the table row R[t_e] is added to its key AND its value:
//   kx_e  = K_j + R[t_e]         vx_e = V_j + R[t_e]            (each formed once per piece, in this order, in every pass)
//   everything else as kernels_attn_edge.h with xe[e] := R[t_e]
//   dR[t] = sum_{e : t_e = t} (ds_e Q_i + a_e mult_e dO_i)
// Nothing edge-sized exists but the int32 per edge.  Every kernel clamps the type into [0, n_types - 1] (one min on the
// unsigned value) before it forms an address: an out-of-range type gives an undefined value and touches no memory
// outside R / dR.  The fast kernels are the third inclusion of kernels_attn_rows_passes.inc, which says how the row pass
// sums dR on chip; k_attn_etype_dr_reduce sums the replicas it leaves.  The generic kernels below (one wave per chunk,
// fp32 / fp64, any h and d, any chunk layout, any n_types) cover every other valid call.
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
#undef AR_EDGE
#undef AR_KERNEL
#undef AR_TYPE
#undef AR_FN

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

// ---- the generic passes: fp32 / fp64, any h and d, any chunk layout; one wave per chunk ------------------------------
// the type of edge id e, clamped: the one place a generic pass reads etype
__device__ __forceinline__ i64 attn_etype_of(const int* __restrict__ etype, i64 e, unsigned tmax) {
  return (i64)min((unsigned)etype[e], tmax);
}

// s of one (slot, head): q = Q[i, k, :], kj = K[j, k, :], r = R[t, k, :].  Every generic pass evaluates it by this
// function, so a recomputed score is bitwise the one the statistics were taken from.
template <typename T>
__device__ __forceinline__ T attn_etype_score(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ r,
                                              i64 d) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += q[c] * (kj[c] + r[c]);
  return s;
}

// stats[i, k] = (-1e9, 0): the floor of the maxima, the start of the sums, and what rows without slots keep
template <typename T>
__global__ void k_attn_etype_stats_init_generic(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { stats[i * 2] = (T)-1e9; stats[i * 2 + 1] = (T)0; }
}
// the sums become 1 / l
template <typename T>
__global__ void k_attn_etype_stats_fin_generic(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const T s = stats[i * 2 + 1]; stats[i * 2 + 1] = s > (T)0 ? (T)1 / s : (T)0; }
}

// lanes over the chunk's slots, one head at a time; SUM = false: the maxima, true: the sums of exp(s - m)
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void k_attn_etype_stats_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ R,
    const int* __restrict__ etype, unsigned tmax, T* __restrict__ stats, i64 n_chunks, i64 h, i64 d) {
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
      const i64 t = attn_etype_of(etype, eid[j], tmax);
      const T s = attn_etype_score<T>(Q + (r * h + k) * d, K + (indices[j] * h + k) * d, R + (t * h + k) * d, d);
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
__global__ __launch_bounds__(kGenericBlock) void k_attn_etype_fwd_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ R, const int* __restrict__ etype, unsigned tmax, const T* __restrict__ stats,
    T* __restrict__ o, i64 n_chunks, i64 h, i64 d, i64 head0, DropArgsIf<DROP, T> dr) {
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
      const i64 src = indices[j], t = attn_etype_of(etype, eid[j], tmax);
      const T s = attn_etype_score<T>(Q + (r * h + k) * d, K + (src * h + k) * d, R + (t * h + k) * d, d);
      T w = exp_t(s - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, head0 + k, dr);
      acc += w * (V[src * f + it] + R[t * f + it]);
    }
    atomicAdd(o + r * f + it, acc);
  }
}

// P[i, k] = (m, 1 / l, D = <dO_ik, o_ik>, 0)
template <typename T>
__global__ void k_attn_etype_pack_generic(const T* __restrict__ stats, const T* __restrict__ dO, const T* __restrict__ o,
                                          T* __restrict__ P, i64 n, i64 d) {   // n = n_q * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T dsum = 0;
  for (i64 c = 0; c < d; ++c) dsum += dO[i * d + c] * o[i * d + c];
  P[i * 4] = stats[i * 2]; P[i * 4 + 1] = stats[i * 2 + 1]; P[i * 4 + 2] = dsum; P[i * 4 + 3] = 0;
}

// ds of one (slot, head): p = P[i, k] holds (m, 1 / l, D); *a_out = a_e; mult = the slot's dropout multiplier
template <typename T>
__device__ __forceinline__ T attn_etype_ds(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ vj,
                                           const T* __restrict__ r, const T* __restrict__ p, const T* __restrict__ dO_ik,
                                           i64 d, T mult, T* a_out) {
  const T s = attn_etype_score<T>(q, kj, r, d);
  const T a = exp_t(s - p[0]) * p[1];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += dO_ik[t] * (vj[t] + r[t]);
  *a_out = a;
  return a * (mult * da - p[2]);
}

// dR (may be NULL) is added into with global atomics, one per (run of slots of one type, element): a lane sums what
// consecutive slots of one type give before it adds.  The slow path; dR is zero-filled by the caller.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_etype_bwd_row_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ R, const int* __restrict__ etype, unsigned tmax, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dQ, T* __restrict__ dR, i64 n_chunks, i64 h, i64 d, i64 head0,
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
    const T q = Q[r * f + it], g = dO[r * f + it];
    T acc = 0, aij, run = 0;
    i64 t_run = attn_etype_of(etype, eid[j0], tmax);
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j], t = attn_etype_of(etype, eid[j], tmax);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, head0 + k, dr);
      const T ds = attn_etype_ds<T>(Q + (r * h + k) * d, K + (src * h + k) * d, V + (src * h + k) * d,
                                    R + (t * h + k) * d, P + (r * h + k) * 4, dO + (r * h + k) * d, d, mult, &aij);
      acc += ds * (K[src * f + it] + R[t * f + it]);
      if (dR != nullptr) {
        if (t != t_run) { atomicAdd(dR + t_run * f + it, run); run = 0; t_run = t; }
        run += ds * q + aij * mult * g;
      }
    }
    atomicAdd(dQ + r * f + it, acc);
    if (dR != nullptr) atomicAdd(dR + t_run * f + it, run);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_etype_bwd_col_generic(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ R, const int* __restrict__ etype, unsigned tmax, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dK, T* __restrict__ dV, i64 n_chunks, i64 h, i64 d, i64 head0,
    DropArgsIf<DROP, T> dr) {
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
      const i64 i = indices[j], t = attn_etype_of(etype, eid[j], tmax);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, head0 + k, dr);
      const T ds = attn_etype_ds<T>(Q + (i * h + k) * d, K + (jc * h + k) * d, V + (jc * h + k) * d,
                                    R + (t * h + k) * d, P + (i * h + k) * 4, dO + (i * h + k) * d, d, mult, &aij);
      acc_k += ds * Q[i * f + it];
      acc_v += aij * mult * dO[i * f + it];
    }
    atomicAdd(dK + jc * f + it, acc_k);
    atomicAdd(dV + jc * f + it, acc_v);
  }
}

}  // namespace graphop
