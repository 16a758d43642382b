// Fused dot-product attention with edge features (graphop_attention_edge_*): the edge row xe[e], indexed
// by edge id, is added to the key AND the value of edge e = (i, j):
//   kx_e  = K_j + xe[e]          vx_e = V_j + xe[e]             (each formed once per piece, in this order, in every pass)
//   s_ek  = <Q_ik, kx_ek>        a_ek = exp(s_ek - m_ik) / l_ik,   o_ik = sum_e a_ek mult_ek vx_ek
//   ds_ek = a_ek (mult_ek <dO_ik, vx_ek> - D_ik)
//   dQ_i  = sum_e ds_e kx_e      dK_j = sum_e ds_e Q_i             dV_j = sum_e a_e mult_e dO_i
//   dxe[e] = ds_e Q_i + a_e mult_e dO_i
// The fast kernels are the chunk-driver passes of the several-head kernels (kernels_attn_heads.h) in
// their layout -- a lane group of 16 lanes holds all heads of a row, piece p = v * L + l, a head's score is dot4 +
// group_sum<DQ> and stays in the lanes of the head -- with the edge row of 4.5i streamed per slot: xe[e * F4 + p] is one
// float4 per (lane, slot, piece), read once with a non-temporal load and added into the gathered K and V pieces where
// they are consumed; the row pass stores dxe[e * F4 + p] with one plain float4 per lane and real slot.  H = 1 (1 x 64)
// is an instantiation like the others.  The generic kernels at the end (one wave per chunk, fp32 / fp64, any h and d,
// any chunk layout) cover every other valid call.  That header cannot be included here (it defines a kernel that is no
// template), so its configuration and keep bits are restated.
#pragma once
#include "kernels_attn.h"
#include "kernels_gat_attn.h"

namespace graphop {

constexpr float kAttnEdgeNegBig = -3.0e38f;   // "no score yet" (finite: differences of two of them are 0, not NaN)
__device__ __forceinline__ float attn_edge_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }   // x <= 0

__device__ __forceinline__ float4 attn_edge_add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ void attn_edge_fma4(float4& acc, float w, const float4& x) {
  acc.x = fmaf(w, x.x, acc.x); acc.y = fmaf(w, x.y, acc.y); acc.z = fmaf(w, x.z, acc.z); acc.w = fmaf(w, x.w, acc.w);
}

// AttnHeadsCfg<H, D> with H = 1 admitted.  SB is that configuration's 8 / NV: the two gathered rows of a batch are 16
// float4 pieces in flight per lane, and the edge piece is a temporary that dies into them, so no instantiation needs a
// smaller batch to stay out of scratch (at most 228 VGPRs).
template <int H, int D>
struct AttnEdgeCfg {
  using G = GatAttnCfg<H, D>;
  static constexpr int L = G::L, F4 = G::F4, NV = G::NV, DQ = G::DQ;
  static constexpr int SB = 8 / NV;
};

// the dropout decision of the call's heads: global head of local head k is head0 + k
struct AttnEdgeDrop {
  DropArgs<float> d;
  int head0;
};
template <bool DROP>
using AttnEdgeDropIf = std::conditional_t<DROP, AttnEdgeDrop, NoDrop>;

// attn_heads_keep_bits restated: lane l works for slot l % SB and runs Philox for the blocks l / SB, l / SB + L / SB, ...
// of the blocks the global heads head0 .. head0 + H - 1 fall into; the lanes of a slot OR their bits together.  Returns,
// in every lane with l % SB == u, slot u's bits (bit k = local head k is kept).  (i, j) as in edge_dropout_mask.
template <int H, int SB>
__device__ __forceinline__ int attn_edge_keep_bits(int l, unsigned i, unsigned j, const AttnEdgeDrop& dr) {
  constexpr int L = 16;
  const int b0 = dr.head0 >> 2;
  const int nblk = ((dr.head0 + H + 3) >> 2) - b0;
  int bits = 0;
  for (int t = l / SB; t < nblk; t += L / SB) {
    const int k4 = drop_keep4<float>(i, j, (unsigned)(b0 + t), dr.d);
    const int sh = (b0 + t) * 4 - dr.head0;   // local head of the block's first decision
    bits |= sh >= 0 ? (k4 << sh) : (k4 >> -sh);
  }
#pragma unroll
  for (int s = SB; s < L; s <<= 1) bits |= __shfl_xor(bits, s, L);
  return bits & ((1 << H) - 1);
}

// ---- forward ------------------------------------------------------------------------------------------------------
struct AttnEdgeFwdArgs {
  const float* Q;       // [n_q][H][D]   own rows
  const float* K;       // [n_k][H][D]   gathered
  const float* V;       // [n_k][H][D]   gathered
  const float* xe;      // [n_edges][H][D]  by edge id, streamed
  float* o;             // [n_q][H][D]   zero-filled by the caller (pieces are added)
  float* stats;         // [n_q][H][2]   (m, 1 / l); rows without slots keep the caller's (-1e9, 0)
  int* p_row;           // [2 * groups]  row | first-piece flag, -1 = none (pre-filled)
  float* p_ml;          // [2 * groups][H][2]
  float* p_o;           // [2 * groups][H][D]
};

// The walk, the per-batch online softmax and the piece protocol of k_attn_heads_fwd_rows_f32.  eid == NULL: the plan
// says eid[slot] == slot.
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_attn_edge_fwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnEdgeFwdArgs a, i64 n_chunks, int chunks_per_group, AttnEdgeDropIf<DROP> dr) {
  using C = AttnEdgeCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  const i64 row_before = c0 > 0 ? row[c0 - 1] : -1;
  const i64 row_after = c1 < n_chunks ? row[c1] : -1;
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 q[NV], o_c[NV];
  float m_c[NV], l_c[NV];   // of the piece's head
  auto finish = [&](i64 r) {
    if (r == row_before || r == row_after) {
      const i64 pi = gid * 2 + (r == row_before ? 0 : 1);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        reinterpret_cast<float4*>(a.p_o)[pi * F4 + v * L + l] = o_c[v];
        if (l % DQ == 0) reinterpret_cast<float2*>(a.p_ml)[pi * H + kv[v]] = make_float2(m_c[v], l_c[v]);
      }
      if (l == 0) a.p_row[pi] = (int)r | (r != row_before ? kWalkFirstPiece : 0);
    } else {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (l_c[v] > 0.f) {   // (the same for every head: a row has slots or has none)
          const float mf = fmaxf(m_c[v], -1e9f);
          const float e = attn_edge_exp(m_c[v] - mf);
          const float lsum = l_c[v] * e;
          const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
          const float f = e * linv;
          float4 o = o_c[v];
          o.x *= f; o.y *= f; o.z *= f; o.w *= f;
          reinterpret_cast<float4*>(a.o)[r * F4 + v * L + l] = o;
          if (l % DQ == 0 && lsum > 0.f) reinterpret_cast<float2*>(a.stats)[r * H + kv[v]] = make_float2(mf, linv);
        }
      }
    }
  };
  i64 cur_row = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      if (cur_row >= 0) finish(cur_row);
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        q[v] = ld4(a.Q, r * F4 + v * L + l);
        o_c[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        m_c[v] = kAttnEdgeNegBig;
        l_c[v] = 0.f;
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the ids of slot l % SB; slots past the end re-read the batch's last slot and are not folded in
      const int t = l % SB;
      const i64 j = jb + (t < nb ? t : nb - 1);
      const int my_src = (int)indices[j];
      const int my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      float4 x0[SB][NV], x1[SB][NV];
      i64 eo[SB];   // the slots' edge rows: e * F4 is 64-bit
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        eo[u] = (i64)group_bcast<L, u>(my_e) * F4;
        const float4* kp = reinterpret_cast<const float4*>(a.K) + src * F4 + l;
        const float4* vp = reinterpret_cast<const float4*>(a.V) + src * F4 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = attn_edge_keep_bits<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        float s[SB];
        float mx = m_c[v];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          // the edge piece goes into the gathered pieces here: kx in place of K_j, vx in place of V_j
          const float4 xe4 = ld4_nt(a.xe, eo[u] + v * L + l);
          x0[u][v] = attn_edge_add4(x0[u][v], xe4);
          x1[u][v] = attn_edge_add4(x1[u][v], xe4);
          s[u] = group_sum<DQ>(dot4(q[v], x0[u][v]));
          if (u < nb) mx = fmaxf(mx, s[u]);   // group-uniform
        }
        const float sc = attn_edge_exp(m_c[v] - mx);
        l_c[v] *= sc;
        o_c[v].x *= sc; o_c[v].y *= sc; o_c[v].z *= sc; o_c[v].w *= sc;
        m_c[v] = mx;
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          if (u < nb) {
            const float p = attn_edge_exp(s[u] - mx);
            l_c[v] += p;
            float pm = p;
            if constexpr (DROP) pm = (keep[u] >> kv[v]) & 1 ? p * dr.d.scale : 0.f;
            attn_edge_fma4(o_c[v], pm, x1[u][v]);
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- merge of the shared rows' pieces: k_attn_heads_piece_max / _add / _fin under this op's names ---------------------
// Mtmp[row, k] starts at kAttnEdgeNegBig, Ltmp[row, k] at 0, o is zero where pieces will be added.
__global__ void k_attn_edge_piece_max(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                      float* __restrict__ Mtmp, i64 n, int h) {   // n = pieces * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int rec = p_row[i / h];
  if (rec < 0) return;
  atomic_max_float(Mtmp + (i64)(rec & kWalkRowMask) * h + i % h, p_ml[i * 2]);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_edge_piece_add(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                                                    const float* __restrict__ p_o, const float* __restrict__ Mtmp,
                                                                    float* __restrict__ Ltmp, float* __restrict__ o, i64 n) {
  using C = AttnEdgeCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  const int rec = p_row[i];
  if (rec < 0) return;
  const i64 row = rec & kWalkRowMask;
  float4 v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int hd = gat_attn_head<H, D>(k, l);
    const float sc = attn_edge_exp(p_ml[(i * H + hd) * 2] - Mtmp[row * H + hd]);
    v[k] = reinterpret_cast<const float4*>(p_o)[i * F4 + k * L + l];
    v[k].x *= sc; v[k].y *= sc; v[k].z *= sc; v[k].w *= sc;
    if (l % DQ == 0) atomicAdd(Ltmp + row * H + hd, p_ml[(i * H + hd) * 2 + 1] * sc);
  }
  atomic_flush_dense<L, NV>(o, row, v, l);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_edge_piece_fin(const int* __restrict__ p_row, const float* __restrict__ Mtmp,
                                                                    const float* __restrict__ Ltmp, float* __restrict__ o,
                                                                    float* __restrict__ stats, i64 n) {
  using C = AttnEdgeCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  const int rec = p_row[i];
  if (rec < 0 || !(rec & kWalkFirstPiece)) return;       // one piece per shared row finishes it
  const i64 row = rec & kWalkRowMask;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int hd = gat_attn_head<H, D>(k, l);
    const float m = Mtmp[row * H + hd];
    const float mf = fmaxf(m, -1e9f);
    const float e = attn_edge_exp(m - mf);
    const float lsum = Ltmp[row * H + hd] * e;
    const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
    const float f = e * linv;
    float4 v = reinterpret_cast<float4*>(o)[row * F4 + k * L + l];
    v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    reinterpret_cast<float4*>(o)[row * F4 + k * L + l] = v;
    if (l % DQ == 0 && lsum > 0.f) reinterpret_cast<float2*>(stats)[row * H + hd] = make_float2(mf, linv);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// (A_r | B_r) -> out[r][2F]; with STATS also st4[r, k] = (m_rk, linv_rk, <B_rk, O_rk>, 0) per head
template <int H, int D, bool STATS>
__global__ __launch_bounds__(kFastBlock) void k_attn_edge_pack(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out, i64 n,
    const float* __restrict__ O, const float* __restrict__ stats2, float4* __restrict__ st4) {
  using C = AttnEdgeCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 r = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (r >= n) return;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float4 a = ld4(A, r * F4 + v * L + l);
    const float4 b = ld4(B, r * F4 + v * L + l);
    reinterpret_cast<float4*>(out)[r * 2 * F4 + v * L + l] = a;
    reinterpret_cast<float4*>(out)[r * 2 * F4 + F4 + v * L + l] = b;
    if constexpr (STATS) {
      const float dsum = group_sum<DQ>(dot4(b, ld4(O, r * F4 + v * L + l)));
      if (l % DQ == 0) {
        const i64 k = r * H + gat_attn_head<H, D>(v, l);
        st4[k] = make_float4(stats2[k * 2], stats2[k * 2 + 1], dsum, 0.f);
      }
    }
  }
}

//   COL = false: OWN = (Q | dO) packed [n_q][2F], XT = (K | V) packed, out0 = dQ; dxe (may be NULL) is written; eid may
//                be NULL (identity plan)
//   COL = true : OWN = (K | V) packed [n_k][2F], XT = (Q | dO) packed, out0 = dK, out1 = dV; dxe is not touched; the
//                edge row xe[eid[slot]] is a random row read of 4 h d bytes per slot, inherent to an operand indexed by
//                edge id
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.
template <int H, int D, bool COL, bool OWNED, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_attn_edge_bwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ OWN, const float* __restrict__ XT,
    const float4* __restrict__ stats4, const float* __restrict__ xe, float* __restrict__ out0, float* __restrict__ out1,
    float* __restrict__ dxe, i64 n_chunks, int chunks_per_group, AttnEdgeDropIf<DROP> dr) {
  using C = AttnEdgeCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  i64 row_before = -1, row_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0) row_before = row[c0 - 1];
    if (c1 < n_chunks) row_after = row[c1];
  }
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = gat_attn_head<H, D>(v, l);
  float4 y0[NV], y1[NV], acc0[NV], acc1[COL ? NV : 1];
  float4 own_st[COL ? 1 : NV];   // ROW: (m, 1 / l, D) of the piece's head
  auto zero_acc = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc0[v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int v = 0; v < (COL ? NV : 1); ++v) acc1[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto flush = [&](i64 r) {
    if (OWNED && r != row_before && r != row_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        reinterpret_cast<float4*>(out0)[r * F4 + v * L + l] = acc0[v];
        if constexpr (COL) reinterpret_cast<float4*>(out1)[r * F4 + v * L + l] = acc1[v];
      }
    } else {
      atomic_flush<L, NV>(out0, r, acc0, l);
      if constexpr (COL) atomic_flush<L, NV>(out1, r, acc1, l);
    }
  };
  zero_acc();
  i64 cur_row = -1;
  bool dirty = false;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      if (dirty) { flush(cur_row); zero_acc(); dirty = false; }
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        y0[v] = ld4(OWN, r * 2 * F4 + v * L + l);
        y1[v] = ld4(OWN, r * 2 * F4 + F4 + v * L + l);
        if constexpr (!COL) own_st[v] = stats4[r * H + kv[v]];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    if (j1 > j0) dirty = true;
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the ids of slot l % SB; slots past the end re-read the batch's last slot with weights 0
      const int t = l % SB;
      const i64 j = jb + (t < nb ? t : nb - 1);
      const int my_src = (int)indices[j];
      const int my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      float4 x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
      i64 eo[SB];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        eo[u] = (i64)group_bcast<L, u>(my_e) * F4;
        const float4* rowp = reinterpret_cast<const float4*>(XT) + src * (2 * F4) + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = rowp[v * L]; x1[u][v] = rowp[F4 + v * L]; }
        if constexpr (COL) {
#pragma unroll
          for (int v = 0; v < NV; ++v) stg[u][v] = stats4[src * H + kv[v]];
        }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = COL ? attn_edge_keep_bits<H, SB>(l, (unsigned)my_src, (unsigned)cur_row, dr)
                             : attn_edge_keep_bits<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float4 xe4 = ld4_nt(xe, eo[u] + v * L + l);
          float4 kx, vx;   // K_j + xe[e], V_j + xe[e]: of the gathered row in the row pass, of the own row in the column pass
          float s, da;
          if constexpr (COL) {
            kx = attn_edge_add4(y0[v], xe4);
            vx = attn_edge_add4(y1[v], xe4);
            s = group_sum<DQ>(dot4(x0[u][v], kx));
            da = group_sum<DQ>(dot4(x1[u][v], vx));
          } else {
            kx = attn_edge_add4(x0[u][v], xe4);
            vx = attn_edge_add4(x1[u][v], xe4);
            s = group_sum<DQ>(dot4(y0[v], kx));
            da = group_sum<DQ>(dot4(y1[v], vx));
          }
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          float mult = 1.f;
          if constexpr (DROP) mult = (keep[u] >> kv[v]) & 1 ? dr.d.scale : 0.f;
          if constexpr (DROP) da *= mult;
          const float ds = av * (da - st.z);
          if constexpr (DROP) av *= mult;   // from here on av weights dO only: a_e mult_e
          if constexpr (COL) {
            attn_edge_fma4(acc0[v], ds, x0[u][v]);   // dK += ds Q_i
            attn_edge_fma4(acc1[v], av, x1[u][v]);   // dV += a mult dO_i
          } else {
            attn_edge_fma4(acc0[v], ds, kx);         // dQ += ds kx
            // kernel-uniform check: the gradient of xe is wanted; one plain float4 per lane and real slot
            if (dxe != nullptr && u < nb) {
              float4 g = make_float4(ds * y0[v].x, ds * y0[v].y, ds * y0[v].z, ds * y0[v].w);
              attn_edge_fma4(g, av, y1[v]);
              reinterpret_cast<float4*>(dxe)[eo[u] + v * L + l] = g;
            }
          }
        }
      }
    }
  }
  if (dirty) flush(cur_row);
}

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
