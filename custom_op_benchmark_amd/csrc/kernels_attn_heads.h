// Several-head forms of the fused dot-product attention kernels (graphop_attention_*, _dropout_*, _bias_*; DESIGN.md
// 4.5l): the chunk-driver forward (k_attn_bias_fwd_rows_f32) and backward (k_attn_bias_bwd_rows_f32) restated for a row
// of F = H * D floats in the layout of the fused GAT layer (GatAttnCfg<H, D>, kernels_gat_attn.h): a lane group of
// L = 16 lanes holds the row's F4 = H * D / 4 float4 pieces, piece p = v * L + l, so the DQ = D / 4 pieces of one head
// sit in DQ adjacent lanes and a per-head dot product is a group_sum<DQ> that leaves the head's score in every lane of
// the head.  Each lane therefore carries the softmax of ITS pieces' heads itself -- (m, l) in the forward, (m, 1 / l, D)
// and a, ds in the backward are per (lane, piece) values -- and no value crosses heads:
//   s_ek  = <Q_ik, K_jk> (+ b[e, k])           e = (i, j), b (E, H) by edge id
//   a_ek  = exp(s_ek - m_ik) / l_ik,   o_ik = sum_e a_ek mult_ek V_jk      (mult: dropout multiplier of global head head0 + k)
//   ds_ek = a_ek (mult_ek <dO_ik, V_jk> - D_ik),   db[e, k] = ds_ek,   dQ, dK from ds, dV from a * mult
// Forward and backward reduce a head's dot product by the same dot4 + group_sum<DQ>, so the backward recomputes the
// forward's s bit for bit.  The one-head kernels keep their text; nothing is shared with them but the helpers.
#pragma once
#include "kernels_attn.h"
#include "kernels_gat_attn.h"

namespace graphop {

// kAttnNegBig and attn_exp of kernels_attn_walk.h, restated: that header defines a kernel that is no template, so only
// one translation unit may include it
constexpr float kAttnHeadsNegBig = -3.0e38f;   // "no score yet" (finite: differences of two of them are 0, not NaN)
__device__ __forceinline__ float attn_heads_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }   // x <= 0

template <int H, int D>
struct AttnHeadsCfg {
  using G = GatAttnCfg<H, D>;
  static constexpr int L = G::L, F4 = G::F4, NV = G::NV, DQ = G::DQ;
  // slots per batch: both kernels gather two rows per slot (K | V, or the packed pair), 16 float4 pieces in flight per
  // lane as in AttnCfg (64 VGPRs); GatAttnCfg::SB_FWD would put 128 in flight
  static constexpr int SB = 8 / NV;
};

// the dropout decision of the call's heads: global head of local head k is head0 + k
struct AttnHeadsDrop {
  DropArgs<float> d;
  int head0;
};
template <bool DROP>
using AttnHeadsDropIf = std::conditional_t<DROP, AttnHeadsDrop, NoDrop>;

// Keep bits of a batch's slots.  Lane l works for slot l % SB: it runs Philox for the blocks l / SB, l / SB + L / SB, ...
// of the blocks the global heads head0 .. head0 + H - 1 fall into (one to three), moves the four decisions of a block to
// the local heads' bit positions, and the lanes of a slot OR their bits together.  Returns, in every lane with
// l % SB == u, slot u's bits (bit k = local head k is kept).  (i, j) = (row-major row, neighbour) as in edge_dropout_mask.
template <int H, int SB>
__device__ __forceinline__ int attn_heads_keep_bits(int l, unsigned i, unsigned j, const AttnHeadsDrop& dr) {
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
struct AttnHeadsFwdArgs {
  const float* Q;       // [n_q][H][D]   own rows
  const float* K;       // [n_k][H][D]   gathered
  const float* V;       // [n_k][H][D]   gathered
  const float* b;       // [n_edges][H]  by edge id (BIAS)
  float* o;             // [n_q][H][D]   zero-filled by the caller (pieces are added)
  float* stats;         // [n_q][H][2]   (m, 1 / l); rows without slots keep the caller's (0, 0)
  int* p_row;           // [2 * groups]  row | first-piece flag, -1 = none (pre-filled)
  float* p_ml;          // [2 * groups][H][2]
  float* p_o;           // [2 * groups][H][D]
};

// The walk of k_attn_bias_fwd_rows_f32 (a lane group takes chunks_per_group consecutive chunks of a rows_sorted plan;
// rows inside the run are normalised and stored, rows shared with a neighbouring group leave as piece records in slot
// 2 * group + {0: continues from the group before, 1: continues into the group after}).  The online softmax is taken
// batch by batch: the heads' maxima over the batch first, one rescale of (l, o) per batch, then one exp per slot.
template <int H, int D, bool DROP, bool BIAS>
__global__ __launch_bounds__(kFastBlock) void k_attn_heads_fwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnHeadsFwdArgs a, i64 n_chunks, int chunks_per_group, AttnHeadsDropIf<DROP> dr) {
  using C = AttnHeadsCfg<H, D>;
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
          const float e = attn_heads_exp(m_c[v] - mf);
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
        m_c[v] = kAttnHeadsNegBig;
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
      int my_e = 0;
      if constexpr (BIAS) my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      float4 x0[SB][NV], x1[SB][NV];
      float bb[BIAS ? SB : 1][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const float4* kp = reinterpret_cast<const float4*>(a.K) + src * F4 + l;
        const float4* vp = reinterpret_cast<const float4*>(a.V) + src * F4 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
      if constexpr (BIAS) {   // the slots' H bias values, behind the row requests
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const i64 e = group_bcast<L, u>(my_e);
#pragma unroll
          for (int v = 0; v < NV; ++v) bb[u][v] = a.b[e * H + kv[v]];
        });
      }
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = attn_heads_keep_bits<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
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
          s[u] = group_sum<DQ>(dot4(q[v], x0[u][v]));
          if constexpr (BIAS) s[u] += bb[u][v];
          if (u < nb) mx = fmaxf(mx, s[u]);   // group-uniform
        }
        const float sc = attn_heads_exp(m_c[v] - mx);
        l_c[v] *= sc;
        o_c[v].x *= sc; o_c[v].y *= sc; o_c[v].z *= sc; o_c[v].w *= sc;
        m_c[v] = mx;
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          if (u < nb) {
            const float p = attn_heads_exp(s[u] - mx);
            l_c[v] += p;
            float pm = p;
            if constexpr (DROP) pm = (keep[u] >> kv[v]) & 1 ? p * dr.d.scale : 0.f;
            o_c[v].x = fmaf(pm, x1[u][v].x, o_c[v].x); o_c[v].y = fmaf(pm, x1[u][v].y, o_c[v].y);
            o_c[v].z = fmaf(pm, x1[u][v].z, o_c[v].z); o_c[v].w = fmaf(pm, x1[u][v].w, o_c[v].w);
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- merge of the shared rows' pieces: the walk's three kernels with (m, l) per (piece, head) -----------------------
// Mtmp[row, k] starts at kAttnHeadsNegBig, Ltmp[row, k] at 0, o is zero where pieces will be added.
__global__ void k_attn_heads_piece_max(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                       float* __restrict__ Mtmp, i64 n, int h) {   // n = pieces * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int rec = p_row[i / h];
  if (rec < 0) return;
  atomic_max_float(Mtmp + (i64)(rec & kWalkRowMask) * h + i % h, p_ml[i * 2]);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_heads_piece_add(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                                                     const float* __restrict__ p_o, const float* __restrict__ Mtmp,
                                                                     float* __restrict__ Ltmp, float* __restrict__ o, i64 n) {
  using C = AttnHeadsCfg<H, D>;
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
    const float sc = attn_heads_exp(p_ml[(i * H + hd) * 2] - Mtmp[row * H + hd]);
    v[k] = reinterpret_cast<const float4*>(p_o)[i * F4 + k * L + l];
    v[k].x *= sc; v[k].y *= sc; v[k].z *= sc; v[k].w *= sc;
    if (l % DQ == 0) atomicAdd(Ltmp + row * H + hd, p_ml[(i * H + hd) * 2 + 1] * sc);
  }
  atomic_flush_dense<L, NV>(o, row, v, l);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_heads_piece_fin(const int* __restrict__ p_row, const float* __restrict__ Mtmp,
                                                                     const float* __restrict__ Ltmp, float* __restrict__ o,
                                                                     float* __restrict__ stats, i64 n) {
  using C = AttnHeadsCfg<H, D>;
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
    const float e = attn_heads_exp(m - mf);
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
__global__ __launch_bounds__(kFastBlock) void k_attn_heads_pack(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out, i64 n,
    const float* __restrict__ O, const float* __restrict__ stats2, float4* __restrict__ st4) {
  using C = AttnHeadsCfg<H, D>;
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

//   COL = false: OWN = (Q | dO) packed [n_q][2F], XT = (K | V) packed, out0 = dQ; db (may be NULL) is written
//   COL = true : OWN = (K | V) packed [n_k][2F], XT = (Q | dO) packed, out0 = dK, out1 = dV; db is not touched
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.
template <int H, int D, bool COL, bool OWNED, bool DROP, bool BIAS>
__global__ __launch_bounds__(kFastBlock) void k_attn_heads_bwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ OWN, const float* __restrict__ XT,
    const float4* __restrict__ stats4, const float* __restrict__ b, float* __restrict__ out0, float* __restrict__ out1,
    float* __restrict__ db, i64 n_chunks, int chunks_per_group, AttnHeadsDropIf<DROP> dr) {
  using C = AttnHeadsCfg<H, D>;
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
      int my_e = 0;
      if constexpr (BIAS) my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      float4 x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
      float bb[BIAS ? SB : 1][NV];
      int ed[BIAS ? SB : 1];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const float4* rowp = reinterpret_cast<const float4*>(XT) + src * (2 * F4) + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = rowp[v * L]; x1[u][v] = rowp[F4 + v * L]; }
        if constexpr (COL) {
#pragma unroll
          for (int v = 0; v < NV; ++v) stg[u][v] = stats4[src * H + kv[v]];
        }
      });
      if constexpr (BIAS) {   // the slots' H bias values, behind the row requests
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          ed[u] = group_bcast<L, u>(my_e);
#pragma unroll
          for (int v = 0; v < NV; ++v) bb[u][v] = b[(i64)ed[u] * H + kv[v]];
        });
      }
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = COL ? attn_heads_keep_bits<H, SB>(l, (unsigned)my_src, (unsigned)cur_row, dr)
                             : attn_heads_keep_bits<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          float s = group_sum<DQ>(dot4(y0[v], x0[u][v]));
          float da = group_sum<DQ>(dot4(y1[v], x1[u][v]));
          if constexpr (BIAS) s += bb[u][v];
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          float mult = 1.f;
          if constexpr (DROP) mult = (keep[u] >> kv[v]) & 1 ? dr.d.scale : 0.f;
          if constexpr (DROP) da *= mult;
          const float ds = av * (da - st.z);
          if constexpr (DROP && COL) av *= mult;   // from here on av only weights dV
          if constexpr (BIAS && !COL) {
            // kernel-uniform check: the gradient of b is wanted; the head's first lane stores it, real slots only
            if (db != nullptr && u < nb && l % DQ == 0) db[(i64)ed[u] * H + kv[v]] = ds;
          }
          acc0[v].x = fmaf(ds, x0[u][v].x, acc0[v].x); acc0[v].y = fmaf(ds, x0[u][v].y, acc0[v].y);
          acc0[v].z = fmaf(ds, x0[u][v].z, acc0[v].z); acc0[v].w = fmaf(ds, x0[u][v].w, acc0[v].w);
          if constexpr (COL) {
            acc1[v].x = fmaf(av, x1[u][v].x, acc1[v].x); acc1[v].y = fmaf(av, x1[u][v].y, acc1[v].y);
            acc1[v].z = fmaf(av, x1[u][v].z, acc1[v].z); acc1[v].w = fmaf(av, x1[u][v].w, acc1[v].w);
          }
        }
      }
    }
  }
  if (dirty) flush(cur_row);
}

}  // namespace graphop
