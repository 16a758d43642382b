// Attention weights of the fused dot-product attention ops (graphop_attention_weights): the weights the
// layer used, from the row statistics (m_i, linv_i) = stats[i, k, :] its forward left.  For edge e = (i, j), head k:
//   plain: s_e = <Q_i, K_j>        bias: s_e = <Q_i, K_j> + b[e]        edge: s_e = <Q_i, K_j + xe[e]>
//   a_e = exp(min(s_e - m_i, 0)) * linv_i                               a, b, xe indexed by edge id
// The min(..., 0) is deliberate: the statistics may come from a kernel that summed the score in another order (the
// walk forward, the several-head forward, a generic one), so a recomputed s_e can sit an ulp above the m_i that kernel
// took; the clamp keeps a_e <= linv_i <= 1 whichever forward made them.
//   k_attn_weights_norm<T, BIAS>     plain and bias modes: a holds s (written by the library's SDDMM) and is normalised
//                                    in place, chunk by chunk: a stream pass over (E, h)
//   k_attn_weights_xe_f32<H, D>      edge mode, fp32, the (h, d) pairs of GO_DISPATCH_GAT_HD: the chunk driver of
//                                    k_gatv2_fwd_f32 on the layout AttnRowsCfg<H, D>; gathers K_j, streams xe[e]
//   k_attn_weights_xe_generic<T>     edge mode, everything else: one wave per chunk
// Every edge id a slot names is written once, by a plain vector store; nothing else is touched: no atomics, no
// workspace, results reproducible bit for bit.
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

// a_e from the score and the row's statistics; fp32 by the exp2 of the fused passes, fp64 by exp
__device__ __forceinline__ float attn_weight(float s, float m, float linv) {
  return attn_rows_exp(fminf(s - m, 0.f)) * linv;
}
__device__ __forceinline__ double attn_weight(double s, double m, double linv) {
  const double x = s - m;
  return exp_t(x < 0.0 ? x : 0.0) * linv;
}

// ---- plain and bias modes: a[e, k] = weight(a[e, k] (+ b[e, k])) in place -------------------------------------------
// A lane group of 16 lanes takes chunks_per_group consecutive chunks.  The items of a chunk are its flattened (slot,
// head) pairs, item q = lane + 16 * step, so with identity edge ids (eid == NULL) lane l of a group reads and writes
// element j0 * h + q: a wave's loads of a / b and its stores are contiguous.  Where h divides 16 a lane sees one head
// for the whole chunk and loads that head's (m, linv) once per chunk; other h look them up per item (L1 hits).
template <typename T, bool BIAS>
__global__ __launch_bounds__(kFastBlock) void k_attn_weights_norm(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const T* __restrict__ stats, const T* __restrict__ b, T* __restrict__ a, i64 n_chunks, i64 h, int chunks_per_group) {
  constexpr int L = 16;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  const bool one_head_per_lane = h <= L && L % h == 0;   // kernel-uniform
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (one_head_per_lane) {
      const i64 t = l % h, step = L / h;
      i64 j = j0 + l / h;
      if (j >= j1) continue;
      const T m = stats[(r * h + t) * 2], linv = stats[(r * h + t) * 2 + 1];
      for (; j < j1; j += step) {
        const i64 o = (eid ? eid[j] : j) * h + t;
        T s = a[o];
        if constexpr (BIAS) s += b[o];
        a[o] = attn_weight(s, m, linv);
      }
    } else {
      const i64 items = (j1 - j0) * h;
      for (i64 q = l; q < items; q += L) {
        const i64 j = j0 + q / h, t = q % h;
        const i64 o = (eid ? eid[j] : j) * h + t;
        T s = a[o];
        if constexpr (BIAS) s += b[o];
        a[o] = attn_weight(s, stats[(r * h + t) * 2], stats[(r * h + t) * 2 + 1]);
      }
    }
  }
}

// ---- edge mode, fp32 fast form ----------------------------------------------------------------------------------------
// A lane group keeps Q_i's pieces and (m, linv) of its pieces' heads while the row is unchanged.  Per slot it gathers K_j
// (the only gathered row: GatAttnCfg::SB_FWD slots, 16 float4 pieces, in flight per lane) and streams xe[e] with
// non-temporal loads (each edge row is read once; e * F4 is 64-bit), forms kx = K_j + xe[e] once and takes
// s = group_sum<DQ>(dot4(q, kx)): the expression of the three passes of kernels_attn_rows_passes.inc, so against
// statistics of that forward the row maximum gives a = linv exactly.  The head's first lane stores a[e * H + k]; for
// H = 1 a batch's weights are collected across the group and leave in one store instruction.
// A NULL eid means eid[slot] == slot (a plan with eid_identity): a kernel-uniform branch.
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_weights_xe_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ stats, const float* __restrict__ xe, float* __restrict__ a, i64 n_chunks,
    int chunks_per_group) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::G::SB_FWD;
  constexpr i64 F4 = C::F4;
  static_assert(H > 1 || (NV == 1 && SB == L), "H = 1: one piece per lane, one slot per lane and batch");
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 q[NV];
  float2 st[NV];   // (m, linv) of the piece's head
  i64 cur_row = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        q[v] = ld4(Q, r * F4 + v * L + l);
        st[v] = reinterpret_cast<const float2*>(stats)[r * H + kv[v]];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the ids of slot l % SB; slots past the end re-read the batch's last slot and store nothing
      const int t = l % SB;
      const i64 j = jb + (t < nb ? t : nb - 1);
      const int my_src = (int)indices[j];
      const int my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      float4 x[SB][NV];
      int ed[SB];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        ed[u] = group_bcast<L, u>(my_e);
        const float4* kp = reinterpret_cast<const float4*>(K) + src * F4 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) x[u][v] = kp[v * L];
      });
      float res = 0.f;
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 eo = (i64)ed[u] * F4;   // the slot's edge row
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float4 kx = attn_rows_add4(x[u][v], ld4_nt(xe, eo + v * L + l));
          const float w = attn_weight(group_sum<DQ>(dot4(q[v], kx)), st[v].x, st[v].y);
          if constexpr (H == 1) {
            if (l == u) res = w;
          } else {
            if (u < nb && l % DQ == 0) a[(i64)ed[u] * H + kv[v]] = w;
          }
        }
      });
      if constexpr (H == 1) {
        if (l < nb) a[my_e] = res;
      }
    }
  }
}

// ---- edge mode, generic form: fp32 / fp64, any h and d, any chunk layout; one wave per chunk ------------------------
// s of one (slot, head): kernels_attn_edge.h's attn_edge_score restated (that header emits kernels under fixed names
// and belongs to one translation unit), so against statistics of the generic forward the score is bitwise the one
// they were taken from.
template <typename T>
__device__ __forceinline__ T attn_weights_edge_score(const T* __restrict__ q, const T* __restrict__ kj,
                                                     const T* __restrict__ e, i64 d) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += q[c] * (kj[c] + e[c]);
  return s;
}

// lanes over the chunk's flattened (slot, head) pairs
template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_attn_weights_xe_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ stats,
    const T* __restrict__ xe, T* __restrict__ a, i64 n_chunks, i64 h, i64 d) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  const i64 items = (j1 - j0) * h;
  for (i64 it = lane; it < items; it += kWave) {
    const i64 j = j0 + it / h, k = it % h;
    const i64 e = eid[j];
    const T s = attn_weights_edge_score<T>(Q + (r * h + k) * d, K + (indices[j] * h + k) * d, xe + (e * h + k) * d, d);
    a[e * h + k] = attn_weight(s, stats[(r * h + k) * 2], stats[(r * h + k) * 2 + 1]);
  }
}

}  // namespace graphop
