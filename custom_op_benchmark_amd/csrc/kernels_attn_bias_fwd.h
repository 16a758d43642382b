// Fused attention FORWARD with a per-edge score bias, chunk-driver form (graphop_attention_bias_forward, DESIGN.md
// 4.5k):  o_i = sum_e softmax_e(<Q_i, K_j> + b[e]) m_e V_j  without s or a in memory.  A lane group walks
// chunks_per_group consecutive chunks of a plan with sorted rows (a row's chunks are consecutive), gathers K_j and V_j
// straight from the caller's tables (no pack pass), keeps Q_i and the running (m, l, o) of the row it is in in
// registers -- the online softmax of kernels_attn_walk.h:  mn = max(m, s); o = o * exp(m - mn) + exp(s - mn) * mult * V_j,
// l likewise without mult: (m, l) are those of the undropped scores -- and reduces the dot products slot by slot in the
// order k_attn_bwd_rows_f32 uses, so the backward recomputes the same s.
// At a row change a row that lies wholly inside the group's run is normalised and stored (o, stats = (max(m, -1e9),
// 1 / l)).  A row shared with a neighbouring group (at most the group's first and its last row; a group whose whole run
// lies inside one hub row has one) leaves as a PIECE record (row | first-piece flag, m, l, o) in slot 2 * group + {0: the
// row continues from the group before, 1: it continues into the group after}; exactly one piece of a shared row carries
// the flag, the one of the group that holds the row's first chunk.  A shared row's piece is written even when the group
// saw no slot of it (m = "no score yet", l = 0): the flagged piece is what finishes the row.  The pieces are merged by
// k_attn_piece_max and the <L, NV> forms of the walk's other two merge kernels below.
#pragma once
#include "kernels_attn_bias.h"
#include "kernels_attn_walk.h"

namespace graphop {

struct AttnBiasFwdArgs {
  const float* Q;       // [n_q][F]   own rows
  const float* K;       // [n_k][F]   gathered
  const float* V;       // [n_k][F]   gathered
  const float* b;       // [n_edges]  by edge id
  float* o;             // [n_q][F]   zero-filled by the caller (pieces are added)
  float* stats;         // [n_q][2]   (m, 1 / l); rows without slots keep the caller's (0, 0)
  int* p_row;           // [2 * groups] row | first-piece flag, -1 = none (pre-filled)
  float* p_ml;          // [2 * groups][2]
  float* p_o;           // [2 * groups][F]
};

template <int L, int NV, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_attn_bias_fwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnBiasFwdArgs a, i64 n_chunks, int chunks_per_group, AttnDropIf<DROP> dr) {
  constexpr int SB = AttnCfg<L, NV>::SB;
  constexpr i64 F4 = (i64)L * NV;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * GroupCfg<L>::kGroupsPerBlock + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  const i64 row_before = c0 > 0 ? row[c0 - 1] : -1;
  const i64 row_after = c1 < n_chunks ? row[c1] : -1;
  float4 q[NV], o_c[NV];
  float m_c = kAttnNegBig, l_c = 0.f;
  auto finish = [&](i64 r) {
    if (r == row_before || r == row_after) {
      const i64 pi = gid * 2 + (r == row_before ? 0 : 1);
#pragma unroll
      for (int v = 0; v < NV; ++v) reinterpret_cast<float4*>(a.p_o)[pi * F4 + v * L + l] = o_c[v];
      if (l == 0) {
        a.p_row[pi] = (int)r | (r != row_before ? kWalkFirstPiece : 0);
        reinterpret_cast<float2*>(a.p_ml)[pi] = make_float2(m_c, l_c);
      }
    } else if (l_c > 0.f) {
      const float mf = fmaxf(m_c, -1e9f);
      const float e = attn_exp(m_c - mf);
      const float lsum = l_c * e;
      const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
      const float f = e * linv;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        float4 o = o_c[v];
        o.x *= f; o.y *= f; o.z *= f; o.w *= f;
        reinterpret_cast<float4*>(a.o)[r * F4 + v * L + l] = o;
      }
      if (l == 0 && lsum > 0.f) reinterpret_cast<float2*>(a.stats)[r] = make_float2(mf, linv);
    }
  };
  i64 cur_row = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      if (cur_row >= 0) finish(cur_row);
      cur_row = r;
      m_c = kAttnNegBig;
      l_c = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        q[v] = ld4(a.Q, r * F4 + v * L + l);
        o_c[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // slots past the end re-read the batch's last neighbour and are not folded in
      i64 my_src = 0;
      if (l < SB) my_src = indices[jb + (l < nb ? l : nb - 1)];
      float4 x0[SB][NV], x1[SB][NV];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const i64 src = __shfl(my_src, u, L);
        const float4* kp = reinterpret_cast<const float4*>(a.K) + src * F4 + l;
        const float4* vp = reinterpret_cast<const float4*>(a.V) + src * F4 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      }
      // the slot's bias (issued behind the row requests) and keep decision: lane u < nb holds slot u's ids
      float my_b = 0.f, mult = 1.f;
      if (l < nb) {
        const i64 e = eid ? eid[jb + l] : jb + l;   // kernel-uniform branch
        my_b = a.b[e];
        if constexpr (DROP) mult = attn_drop_mult((unsigned)cur_row, (unsigned)my_src, dr);
      }
      float my_s = 0.f;
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        float p = dot4(q[0], x0[u][0]);
#pragma unroll
        for (int v = 1; v < NV; ++v) p += dot4(q[v], x0[u][v]);
        p = group_sum<L>(p);
        if (l == u) my_s = p;
      }
      my_s += my_b;
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        if (u < nb) {   // group-uniform
          const float su = __shfl(my_s, u, L);
          const float mx = fmaxf(m_c, su);
          const float sc = attn_exp(m_c - mx);
          const float p = attn_exp(su - mx);
          l_c = fmaf(l_c, sc, p);
          float pm = p;
          if constexpr (DROP) pm *= __shfl(mult, u, L);
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            o_c[v].x = fmaf(o_c[v].x, sc, pm * x1[u][v].x); o_c[v].y = fmaf(o_c[v].y, sc, pm * x1[u][v].y);
            o_c[v].z = fmaf(o_c[v].z, sc, pm * x1[u][v].z); o_c[v].w = fmaf(o_c[v].w, sc, pm * x1[u][v].w);
          }
          m_c = mx;
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// k_attn_piece_add / _fin of kernels_attn_walk.h for rows of NV float4 slots per lane (those two keep their <L> form:
// the walk's launches stay as they are)
template <int L, int NV>
__global__ __launch_bounds__(kFastBlock) void k_attn_bias_piece_add(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                                                    const float* __restrict__ p_o, const float* __restrict__ Mtmp,
                                                                    float* __restrict__ Ltmp, float* __restrict__ o, i64 n) {
  constexpr i64 F4 = (i64)L * NV;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  const int rec = p_row[i];
  if (rec < 0) return;
  const i64 row = rec & kWalkRowMask;
  const float sc = attn_exp(p_ml[i * 2] - Mtmp[row]);
  float4 v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    v[k] = reinterpret_cast<const float4*>(p_o)[i * F4 + k * L + l];
    v[k].x *= sc; v[k].y *= sc; v[k].z *= sc; v[k].w *= sc;
  }
  atomic_flush_dense<L, NV>(o, row, v, l);
  if (l == 0) atomicAdd(Ltmp + row, p_ml[i * 2 + 1] * sc);
}
template <int L, int NV>
__global__ __launch_bounds__(kFastBlock) void k_attn_bias_piece_fin(const int* __restrict__ p_row, const float* __restrict__ Mtmp,
                                                                    const float* __restrict__ Ltmp, float* __restrict__ o,
                                                                    float* __restrict__ stats, i64 n) {
  constexpr i64 F4 = (i64)L * NV;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  const int rec = p_row[i];
  if (rec < 0 || !(rec & kWalkFirstPiece)) return;       // one piece per shared row finishes it
  const i64 row = rec & kWalkRowMask;
  const float m = Mtmp[row];
  const float mf = fmaxf(m, -1e9f);
  const float e = attn_exp(m - mf);
  const float lsum = Ltmp[row] * e;
  const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
  const float f = e * linv;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float4 v = reinterpret_cast<float4*>(o)[row * F4 + k * L + l];
    v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    reinterpret_cast<float4*>(o)[row * F4 + k * L + l] = v;
  }
  if (l == 0 && lsum > 0.f) reinterpret_cast<float2*>(stats)[row] = make_float2(mf, linv);
}

}  // namespace graphop
