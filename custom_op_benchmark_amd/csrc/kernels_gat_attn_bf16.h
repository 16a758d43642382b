// The fused GAT attention layer on bfloat16 tables (gat_attention_bf16.hip has the host side): el, er, V,
// o, dO, del, der, dV are bf16, stats (n_src, H, 2) = (m, 1 / l) stay fp32, every sum is fp32 and every bf16 result is
// rounded once, to nearest even.  The formulas are those of kernels_gat_attn.h (and kernels_dropout.h for the keep
// decision); the score is z = float(el_i) + float(er_j), one fp32 add of exactly widened values, then LeakyReLU in fp32.
//
// Layout, accumulators, the dot chain and the record scheme are kernels_attn_bf16.h's: a row of F = H * D elements is
// F8 = F / 8 pieces of 16 B, a lane group of L = min(16, F8) lanes holds NV = F8 / L of them, piece p = v * L + l, a head
// is DQ = D / 8 adjacent lanes.  A slot gathers ONE row here (V_j, or dO_i in the column pass), so the forward takes
// SB = min(16 / NV, L) slots per batch -- up to 16 pieces of 16 B in flight per lane -- and the backward passes, which
// also gather er_j or the 16-byte P item per piece, 8 / NV.  SB <= L in every pass: lane l holds the id of slot l % SB
// and runs that slot's Philox call, the keep bits travel round the group like the id (GatBf16DropCfg).
//
// Matrix instructions do not fit: a weight pairs one own row with one gathered row, so there is no second dimension of
// rows to tile over; the per-head dot of the backward is a v_dot2c_f32_bf16 chain and a group_sum<DQ>.
//
// No float atomic on any output.  A lane group takes chunks_per_group consecutive chunks of a row_owned plan; rows wholly
// inside its run it rounds and stores; the at most two rows it shares with its neighbours leave as fp32 records in slot
// 2 * group + {0, 1} (row word with first / last flags, kBf16RecNone = no record) that a merge kernel sums in record
// order -- plain sums, the statistics are final before the forward starts -- rounds and stores once.
// Passes:
//   widen  : el, er -> fp32 tables for k_gat_attn_stats_f32, which runs unchanged: stats are bit for bit those of the
//            fp32 op on the widened inputs
//   fwd    : el_i, (m, 1 / l) and the fp32 output row in registers; gathers er_j (2 B per piece's head) and V_j
//   pack   : P[i, k] = (el, m, 1 / l, D) fp32, D = <dO_i, o_i> from the bf16 o as given
//   bwd_row: dO_i packed and P[i] in registers; gathers er_j and V_j -> del (records of H floats)
//   bwd_col: V_j packed and er_j in registers; gathers P[i] and dO_i -> der, dV (records of H + F floats)
// da = group_sum<DQ>(attn_bf16_dot(dO piece, V piece)) with the dO-side word first in both backward passes, so the two
// agree on every dz bit for bit.
#pragma once
#include "kernels_attn_bf16.h"
#include "kernels_bf16_drop.h"
#include "kernels_dropout.h"
#include "kernels_gat.h"

namespace graphop {

typedef unsigned short bf16_t;   // one bfloat16 as its bits

template <int H, int D>
struct GatBf16Cfg : AttnBf16Cfg<H, D> {
  using B = AttnBf16Cfg<H, D>;
  static constexpr int SB_FWD = 16 / B::NV < B::L ? 16 / B::NV : B::L;   // one gathered row per slot
  static constexpr int SB_BWD = B::SB;                                   // 8 / NV: er / P ride along per piece
  static_assert(SB_FWD <= B::L && SB_BWD <= B::L, "a lane holds at most one slot id");
};

__device__ __forceinline__ float bf16_widen(bf16_t x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ bf16_t bf16_round1(float x) { return (bf16_t)(bf16_pack2(x, 0.f) & 0xffffu); }

// ---- widen: k_gat_attn_bf16_widen, no template, is defined in gat_attention_bf16.hip alone (kernels_gatv2_attn_bf16.h includes this file)

// ---- forward ----------------------------------------------------------------------------------------------------------------
struct GatBf16FwdArgs {
  const bf16_t* el;       // [n_l][H]
  const bf16_t* er;       // [n_r][H]   gathered
  const float2* stats;    // [n_l][H]   (m, 1 / l), final
  const uint4* V;         // [n_r][F8]  gathered
  uint4* o;               // [n_l][F8]  zero-filled by the caller: rows without chunks are not written
  unsigned* p_row;        // [2 * groups]  row words, kBf16RecNone-filled
  float* p_o;             // [2 * groups][F]
};

template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_bf16_fwd(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices, GatBf16FwdArgs a,
    i64 n_chunks, int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  using C = GatBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, SB = C::SB_FWD;
  constexpr i64 F8 = C::F8;
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
  for (int v = 0; v < NV; ++v) kv[v] = attn_bf16_head<H, D>(v, l);
  Bf16Acc acc[NV];
  float a_el[NV], a_m[NV], a_il[NV];
  auto flush = [&](i64 r) {
    if (r != row_before && r != row_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) a.o[r * F8 + v * L + l] = attn_bf16_round(acc[v]);
    } else {
      const i64 pi = attn_bf16_rec_slot(gid, r, row_before);
#pragma unroll
      for (int v = 0; v < NV; ++v) attn_bf16_rec_store(a.p_o, pi * F8 + v * L + l, acc[v]);
      if (l == 0) a.p_row[pi] = attn_bf16_rec_word(r, row_before, row_after);
    }
  };
  i64 cur = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur) {
      if (cur >= 0) flush(cur);
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        attn_bf16_zero(acc[v]);
        a_el[v] = bf16_widen(a.el[r * H + kv[v]]);
        const float2 st = a.stats[r * H + kv[v]];
        a_m[v] = st.x;
        a_il[v] = st.y;
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot with weight 0
      const int t = l % SB;
      const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      uint4 x[SB][NV];
      bf16_t e[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* vp = a.V + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          x[u][v] = vp[v * L];
          e[u][v] = a.er[src * H + kv[v]];
        }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = gat_bf16_lane_bits<H, SB, L, false>(l, r, my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = gat_bf16_slot_bits<H, SB, L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float z = gat_lrelu(a_el[v] + bf16_widen(e[u][v]), slope);
          float w = u < nb ? exp_nonpos(z - a_m[v]) * a_il[v] : 0.f;
          if constexpr (DROP) w = (keep[u] >> kv[v]) & 1 ? w * dr.scale : 0.f;
          attn_bf16_fma(acc[v], w, x[u][v]);
        }
      }
    }
  }
  if (cur >= 0) flush(cur);
}

// One lane group per first record: plain sums over the row's records in record order, then the row once.
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_bf16_fwd_merge(GatBf16FwdArgs a, i64 n) {
  using C = GatBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  unsigned w = a.p_row[i];
  if (w == kBf16RecNone || !(w & kBf16RecFirst)) return;
  const unsigned r = w & kBf16RecRow;
  Bf16Acc acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) attn_bf16_zero(acc[v]);
  for (i64 j = i; j >= 0; j = attn_bf16_rec_next(a.p_row, j, n, r, w)) {
#pragma unroll
    for (int v = 0; v < NV; ++v) attn_bf16_add(acc[v], attn_bf16_rec_load(a.p_o, j * F8 + v * L + l));
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) a.o[(i64)r * F8 + v * L + l] = attn_bf16_round(acc[v]);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// P[i, k] = (el, m, 1 / l, <dO_ik, o_ik>): the dO-side word first, fp32 sums
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_bf16_pack(
    const bf16_t* __restrict__ el, const float2* __restrict__ stats, const uint4* __restrict__ dO,
    const uint4* __restrict__ o, float4* __restrict__ P, i64 n) {
  using C = GatBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;   // group-uniform
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float dsum = group_sum<DQ>(attn_bf16_dot(dO[i * F8 + v * L + l], o[i * F8 + v * L + l]));
    if (l % DQ == 0) {
      const i64 k = i * H + attn_bf16_head<H, D>(v, l);
      const float2 st = stats[k];
      P[k] = make_float4(bf16_widen(el[k]), st.x, st.y, dsum);
    }
  }
}

// the records of a backward pass: row words, H floats (del or der) and, in the column pass, F floats (dV) per record
struct GatBf16BwdRec {
  unsigned* p_row;      // [2 * groups], kBf16RecNone-filled
  float* p_h;           // [2 * groups][H]
  float* p_v;           // [2 * groups][F]   COL only
};

//   COL = false: own = dO_i (packed) and P[i]; gathers er_j and V_j; out_h = del
//   COL = true : own = V_j (packed) and er_j; gathers P[i] and dO_i; out_h = der, out_v = dV
// out_h / out_v are zero-filled by the caller: rows without chunks are not written.
// DROP: da_ij = m_ij <dO_i, V_j> and dV_j sums a_ij m_ij dO_i; D_i in P is <dO_i, o_i> of the dropped o.
template <int H, int D, bool COL, bool DROP>
__device__ __forceinline__ void gat_attn_bf16_bwd_walk(
    const i64* __restrict__ seg, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const bf16_t* __restrict__ er, const uint4* __restrict__ V, const float4* __restrict__ P,
    const uint4* __restrict__ dO, bf16_t* __restrict__ out_h, uint4* __restrict__ out_v, const GatBf16BwdRec& rec,
    i64 n_chunks, int chunks_per_group, float slope, const DropArgsIf<DROP, float>& dr) {
  using C = GatBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_BWD;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  const i64 row_before = c0 > 0 ? seg[c0 - 1] : -1;
  const i64 row_after = c1 < n_chunks ? seg[c1] : -1;
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = attn_bf16_head<H, D>(v, l);
  uint4 y[NV];                 // ROW: dO_i   COL: V_j
  float4 p_own[COL ? 1 : NV];  // ROW: P[i, k_v]
  float e_own[COL ? NV : 1];   // COL: er[j, k_v]
  float acc[NV];               // dz sums of the piece's head
  Bf16Acc accv[COL ? NV : 1];  // COL: dV_j
  auto zero_acc = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.f;
#pragma unroll
    for (int v = 0; v < (COL ? NV : 1); ++v) attn_bf16_zero(accv[v]);
  };
  auto flush = [&](i64 r) {
    if (r != row_before && r != row_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (l % DQ == 0) out_h[r * H + kv[v]] = bf16_round1(acc[v]);
        if constexpr (COL) out_v[r * F8 + v * L + l] = attn_bf16_round(accv[v]);
      }
    } else {
      const i64 pi = attn_bf16_rec_slot(gid, r, row_before);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (l % DQ == 0) rec.p_h[pi * H + kv[v]] = acc[v];
        if constexpr (COL) attn_bf16_rec_store(rec.p_v, pi * F8 + v * L + l, accv[v]);
      }
      if (l == 0) rec.p_row[pi] = attn_bf16_rec_word(r, row_before, row_after);
    }
  };
  i64 cur = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = seg[c];
    if (r != cur) {
      if (cur >= 0) flush(cur);
      zero_acc();
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        y[v] = (COL ? V : dO)[r * F8 + v * L + l];
        if constexpr (COL) e_own[v] = bf16_widen(er[r * H + kv[v]]);
        else p_own[v] = P[r * H + kv[v]];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot with weight 0
      const int t = l % SB;
      const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      uint4 x[SB][NV];                  // ROW: V_j   COL: dO_i
      float4 pg[COL ? SB : 1][NV];      // COL: P[i, k_v]
      bf16_t eg[COL ? 1 : SB][NV];      // ROW: er[j, k_v]
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* xp = (COL ? dO : V) + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          x[u][v] = xp[v * L];
          if constexpr (COL) pg[u][v] = P[src * H + kv[v]];
          else eg[u][v] = er[src * H + kv[v]];
        }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = gat_bf16_lane_bits<H, SB, L, COL>(l, r, my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = gat_bf16_slot_bits<H, SB, L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          // the dO-side words first in both passes
          float da = group_sum<DQ>(COL ? attn_bf16_dot(x[u][v], y[v]) : attn_bf16_dot(y[v], x[u][v]));
          float4 p;
          float z;
          if constexpr (COL) { p = pg[u][v]; z = p.x + e_own[v]; }
          else { p = p_own[v]; z = p.x + bf16_widen(eg[u][v]); }
          const float av = u < nb ? exp_nonpos(gat_lrelu(z, slope) - p.y) * p.z : 0.f;
          float am = av;   // a_ij m_ij
          if constexpr (DROP) {
            const float m = (keep[u] >> kv[v]) & 1 ? dr.scale : 0.f;
            da *= m;
            am *= m;
          }
          const float ds = av * (da - p.w);
          acc[v] += z > 0.f ? ds : ds * slope;
          if constexpr (COL) attn_bf16_fma(accv[v], am, x[u][v]);
        }
      }
    }
  }
  if (cur >= 0) flush(cur);
}

template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_bf16_bwd_row(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const bf16_t* __restrict__ er, const uint4* __restrict__ V, const float4* __restrict__ P,
    const uint4* __restrict__ dO, bf16_t* __restrict__ del, GatBf16BwdRec rec, i64 n_chunks, int chunks_per_group,
    float slope, DropArgsIf<DROP, float> dr) {
  gat_attn_bf16_bwd_walk<H, D, false, DROP>(row, indptr, indices, er, V, P, dO, del, nullptr, rec, n_chunks,
                                            chunks_per_group, slope, dr);
}

template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_bf16_bwd_col(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const bf16_t* __restrict__ er, const uint4* __restrict__ V, const float4* __restrict__ P,
    const uint4* __restrict__ dO, bf16_t* __restrict__ der, uint4* __restrict__ dV, GatBf16BwdRec rec, i64 n_chunks,
    int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  gat_attn_bf16_bwd_walk<H, D, true, DROP>(col, indptr, indices, er, V, P, dO, der, dV, rec, n_chunks, chunks_per_group,
                                           slope, dr);
}

// One lane group per first record: plain sums over the row's records in record order, then the row once.  COL says what
// a record holds: H floats, or H floats and a row of F.  Lane k < H sums head k.
template <int H, int D, bool COL>
__global__ __launch_bounds__(kFastBlock) void k_gat_attn_bf16_bwd_merge(GatBf16BwdRec rec, bf16_t* __restrict__ out_h,
                                                                        uint4* __restrict__ out_v, i64 n) {
  using C = GatBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV;
  constexpr i64 F8 = C::F8;
  static_assert(H <= L, "a lane per head");
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  unsigned w = rec.p_row[i];
  if (w == kBf16RecNone || !(w & kBf16RecFirst)) return;
  const unsigned r = w & kBf16RecRow;
  float acc = 0.f;
  Bf16Acc accv[COL ? NV : 1];
#pragma unroll
  for (int v = 0; v < (COL ? NV : 1); ++v) attn_bf16_zero(accv[v]);
  for (i64 j = i; j >= 0; j = attn_bf16_rec_next(rec.p_row, j, n, r, w)) {
    if (l < H) acc += rec.p_h[j * H + l];
    if constexpr (COL) {
#pragma unroll
      for (int v = 0; v < NV; ++v) attn_bf16_add(accv[v], attn_bf16_rec_load(rec.p_v, j * F8 + v * L + l));
    }
  }
  if (l < H) out_h[(i64)r * H + l] = bf16_round1(acc);
  if constexpr (COL) {
#pragma unroll
    for (int v = 0; v < NV; ++v) out_v[(i64)r * F8 + v * L + l] = attn_bf16_round(accv[v]);
  }
}

}  // namespace graphop
