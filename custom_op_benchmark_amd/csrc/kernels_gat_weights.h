// Attention weights of the fused GAT and GATv2 layers (graphop_gat_attention_weights, graphop_gatv2_attention_weights;
// DESIGN.md 4.5q): the weights the layer used, from the row statistics (m_i, linv_i) = stats[i, k, :] its forward left.
// For edge e = (i, j), head k:
//   GAT  :  s_e = LeakyReLU((el[i, k] + er[j, k]) [+ ee[e, k]])
//   GATv2:  s_e = sum_c att[k, c] LeakyReLU((xl[i, k, c] + xr[j, k, c]) [+ xe[e, k, c]])
//   a_e = exp(min(s_e - m_i, 0)) * linv_i                               a, ee, xe indexed by edge id
// The scores are written with the expressions of the fused forwards (gat_lrelu on (el + er) + ee; gv2attn_dot4, or
// gv2edge_dot4 on gv2edge_z4).  The min(..., 0) is that of kernels_attn_weights.h: the statistics may come from a kernel
// that summed in another order (the long-segment LDS merge of k_gv2attn_fwd_f32, a generic kernel, a contracted
// z * slope - m), so a recomputed s_e can sit an ulp above m_i; the clamp keeps a_e <= linv_i <= 1 whichever forward
// made them.
//   k_gatw_f32<H, EDGE>        fp32, H in {1, 2, 4, 8}: the driver of k_gat_fwd_f32 (GatCfg<H>, U chunks in flight)
//   k_gv2w_f32<H, D, EDGE>     fp32, the (h, d) pairs of GO_DISPATCH_GAT_HD: the chunk driver of k_gatv2_fwd_f32 on
//                              Gv2AttnCfg<H, D>; gathers xr_j, streams xe[e]
//   k_gatw_generic<T, EDGE>, k_gv2w_generic<T, EDGE>   everything else: one wave per chunk
// EDGE is a template argument here (the kernels are new: no older name or kernarg layout has to survive), so each
// kernel has one parameter list; ee / xe is NULL and never read without the edge term.
// Every edge id a slot names is written once, by a plain vector store; nothing else is touched: no atomics, no
// workspace, results reproducible bit for bit.  No kernel owns a row, so shuffled and partial chunk lists take the fast
// kernels too.  A NULL eid in a fast kernel means eid[slot] == slot (a plan with eid_identity): a kernel-uniform branch,
// and the ee / xe loads and the stores of a are then contiguous.
#pragma once
#include "kernels_gat_edge_attn.h"
#include "kernels_gatv2_edge_attn.h"

namespace graphop {

// a_e from the score and the row's statistics; fp32 by exp_nonpos after the clamp, fp64 by exp
__device__ __forceinline__ float gatw_weight(float s, float m, float linv) {
  return exp_nonpos(fminf(s - m, 0.f)) * linv;
}
__device__ __forceinline__ double gatw_weight(double s, double m, double linv) {
  const double x = s - m;
  return exp_t(x < 0.0 ? x : 0.0) * linv;
}

// ---- GAT, fp32 fast form -----------------------------------------------------------------------------------------------
// k_gat_fwd_f32's walk: lane l of a group of G holds item q = l % Q (W heads) of slot l / Q; the first B lanes load a
// batch's ids.  The chunk's el item and the (m, linv) of its W heads stay in registers while the row is unchanged; per
// slot er[j] is gathered and, with EDGE, ee[e] loaded at the slot's edge id; one vector store of a per item.
template <int H, bool EDGE>
__global__ __launch_bounds__(kFastBlock) void k_gatw_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ el, const float* __restrict__ er,
    const float* __restrict__ ee, const float2* __restrict__ stats, float* __restrict__ a, i64 n_chunks,
    int chunks_per_group, float s) {
  using C = GatCfg<H>;
  constexpr int Q = C::Q, W = C::W, G = C::G, B = C::B, U = C::U;
  const int l = threadIdx.x % G;
  const int sl = l / Q, q = l % Q;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / G) + threadIdx.x / G;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  GatItem<W> x[U];
  float2 st[U][W];   // (m, linv) of the item's heads
  i64 cur[U];
#pragma unroll
  for (int u = 0; u < U; ++u) cur[u] = -1;
  for (i64 c = c0; c < c1; c += U) {
    i64 jb[U];
    int n[U];
    int nmax = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      n[u] = 0;
      jb[u] = 0;
      if (c + u < c1) {
        const i64 r = row[c + u];
        if (r != cur[u]) {
          x[u] = gat_ld<W>(el + r * H + q * W);
#pragma unroll
          for (int i = 0; i < W; ++i) st[u][i] = stats[r * H + q * W + i];
          cur[u] = r;
        }
        jb[u] = indptr[c + u];
        n[u] = (int)(indptr[c + u + 1] - jb[u]);
        nmax = n[u] > nmax ? n[u] : nmax;
      }
    }
    for (int off = 0; off < nmax; off += B) {
      int e[U], src[U];
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int nb = n[u] - off;
        int my_e = 0, my_s = 0;
        if (l < B && l < nb) {
          const i64 j = jb[u] + off + l;
          my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
          my_s = (int)indices[j];
        }
        live[u] = sl < nb;
        e[u] = Q > 1 ? __shfl(my_e, sl, G) : my_e;
        src[u] = Q > 1 ? __shfl(my_s, sl, G) : my_s;
      }
      GatItem<W> b[U], g[EDGE ? U : 1];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live[u]) {
          b[u] = gat_ld<W>(er + (i64)src[u] * H + q * W);
          if constexpr (EDGE) g[u] = gat_ld<W>(ee + (i64)e[u] * H + q * W);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live[u]) {
          GatItem<W> o;
#pragma unroll
          for (int i = 0; i < W; ++i) {
            float z = x[u].v[i] + b[u].v[i];
            if constexpr (EDGE) z = z + g[u].v[i];
            o.v[i] = gatw_weight(gat_lrelu(z, s), st[u][i].x, st[u][i].y);
          }
          gat_st<W>(a + (i64)e[u] * H + q * W, o);
        }
      }
    }
  }
}

// ---- GAT, generic form: fp32 / fp64, any h, any chunk layout; one wave per chunk, lanes over (slot, head) ----------------
template <typename T, bool EDGE>
__global__ __launch_bounds__(kGenericBlock) void k_gatw_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ el, const T* __restrict__ er, const T* __restrict__ ee,
    const T* __restrict__ stats, T* __restrict__ a, i64 n_chunks, i64 h, T s) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c];
  const i64 items = (indptr[c + 1] - j0) * h;
  for (i64 it = lane; it < items; it += kWave) {
    const i64 j = j0 + it / h, k = it % h;
    const i64 e = eid[j];
    T z = el[r * h + k] + er[indices[j] * h + k];
    if constexpr (EDGE) z = z + ee[e * h + k];
    a[e * h + k] = gatw_weight(gat_lrelu(z, s), stats[(r * h + k) * 2], stats[(r * h + k) * 2 + 1]);
  }
}

// ---- GATv2, fp32 fast form ---------------------------------------------------------------------------------------------
// A lane group keeps xl_i's pieces, its pieces of att and (m, linv) of its pieces' heads while the row is unchanged.  Per
// slot it gathers xr_j (the only gathered row: SB_FWD slots, 16 float4 pieces, in flight per lane) and, with EDGE,
// streams xe[e] with non-temporal loads at the 64-bit offset e * F4, consumed where z is formed: no second [SB][NV]
// array.  s = group_sum<DQ>(...) of the forward's expression; the head's first lane stores a[e * H + k]; for H = 1 a
// batch's weights are collected across the group and leave in one store instruction.
template <int H, int D, bool EDGE>
__global__ __launch_bounds__(kFastBlock) void k_gv2w_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ xl, const float* __restrict__ xr,
    const float* __restrict__ xe, const float* __restrict__ att, const float* __restrict__ stats,
    float* __restrict__ a, i64 n_chunks, int chunks_per_group, float slope) {
  using C = Gv2AttnCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_FWD;
  constexpr i64 F4 = C::F4;
  static_assert(H > 1 || (NV == 1 && SB == L), "H = 1: one piece per lane, one slot per lane and batch");
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  int kv[NV];
  float4 w[NV], xi[NV];
  float2 st[NV];   // (m, linv) of the piece's head
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = (v * L + l) / DQ;
    w[v] = ld4(att, v * L + l);
  }
  i64 cur_row = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        xi[v] = ld4(xl, r * F4 + v * L + l);
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
#pragma unroll
        for (int v = 0; v < NV; ++v) x[u][v] = ld4(xr, src * F4 + v * L + l);
      });
      float res = 0.f;
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          float p;
          if constexpr (EDGE) {
            const i64 eo = (i64)ed[u] * F4;   // the slot's edge row
            p = gv2edge_dot4(w[v], gv2edge_z4(xi[v], x[u][v], ld4_nt(xe, eo + v * L + l)), slope);
          } else {
            p = gv2attn_dot4(w[v], xi[v], x[u][v], slope);
          }
          const float wt = gatw_weight(group_sum<DQ>(p), st[v].x, st[v].y);
          if constexpr (H == 1) {
            if (l == u) res = wt;
          } else {
            if (u < nb && l % DQ == 0) a[(i64)ed[u] * H + kv[v]] = wt;
          }
        }
      });
      if constexpr (H == 1) {
        if (l < nb) a[my_e] = res;
      }
    }
  }
}

// ---- GATv2, generic form: fp32 / fp64, any h and d, any chunk layout; one wave per chunk ---------------------------------
// s of one (slot, head): kernels_gatv2_attn_generic.inc's score restated with EDGE as a template argument (that file
// emits kernels under fixed names), so against statistics of the generic forward the score is bitwise the one they were
// taken from.
template <typename T, bool EDGE>
__device__ __forceinline__ T gv2w_score(const T* __restrict__ xi, const T* __restrict__ xj, const T* __restrict__ e,
                                        const T* __restrict__ w, i64 d, T slope) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) {
    T z = xi[c] + xj[c];
    if constexpr (EDGE) z = z + e[c];
    s += w[c] * gat_lrelu(z, slope);
  }
  return s;
}

// lanes over the chunk's flattened (slot, head) pairs
template <typename T, bool EDGE>
__global__ __launch_bounds__(kGenericBlock) void k_gv2w_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ xl, const T* __restrict__ xr, const T* __restrict__ xe,
    const T* __restrict__ att, const T* __restrict__ stats, T* __restrict__ a, i64 n_chunks, i64 h, i64 d, T slope) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c], j1 = indptr[c + 1];
  const i64 items = (j1 - j0) * h;
  for (i64 it = lane; it < items; it += kWave) {
    const i64 j = j0 + it / h, k = it % h;
    const i64 e = eid[j];
    const T s = gv2w_score<T, EDGE>(xl + (r * h + k) * d, xr + (indices[j] * h + k) * d,
                                    EDGE ? xe + (e * h + k) * d : nullptr, att + k * d, d, slope);
    a[e * h + k] = gatw_weight(s, stats[(r * h + k) * 2], stats[(r * h + k) * 2 + 1]);
  }
}

}  // namespace graphop
