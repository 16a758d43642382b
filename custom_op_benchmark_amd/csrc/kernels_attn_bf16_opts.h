// The bfloat16 fused attention step with attention dropout, a per-edge score bias, or both (DESIGN.md 4.5w;
// attention_bf16_opts.hip has the host side).  Tables, layout, record scheme and arithmetic are those of
// kernels_attn_bf16.h: AttnBf16Cfg<H, D>, 16-byte pieces, lane groups of L = min(16, F8) lanes, SB = 8 / NV slots per
// batch, rows shared between lane groups leave as fp32 records.  The pack kernel and the three merge kernels are that
// header's, unchanged: the records hold the same things.  These two kernels are text of their own, so that
// k_attn_bf16_fwd_rows / _bwd_rows stay what their own text compiles to.
//
// What the options add to a batch:
//   edge ids   the lane that holds a slot's neighbour id also loads eid[slot] (BIAS alone; a NULL eid says eid[slot] ==
//              slot, a kernel-uniform branch) and hands it round the group like the neighbour id; the column pass is given
//              the column-major eid, so b is addressed by edge id in both orientations
//   b          bf16 (n_edges, H): every lane reads the 2-byte values of its pieces' heads behind the row requests -- the
//              DQ lanes of a head read one address, which the memory pipeline serves once -- and widens them exactly.
//              s = group_sum<DQ>(dot chain) + b: ONE fp32 add after the reduction, the same expression in the forward, the
//              row pass and the column pass, so the backward's s is the forward's bit for bit
//   keep bits  bf16_keep_bits<H, SB, L> (kernels_bf16_drop.h): Philox in the lanes of the slot, one to three blocks for
//              the global heads head0 .. head0 + H - 1; the multiplier is 1 / (1 - p) in fp32.  l sums the UNDROPPED exp:
//              stats are those of the biased, undropped scores, and a row whose edges are all dropped has o = 0, dQ = 0
//   db         the row pass with DB: the head's first lane (l % DQ == 0) stores bf16(ds), rounded once, for the real slots
//              u < nb; each edge id a row-major slot names is written exactly once.  Without DB neither the store nor its
//              address arithmetic exists.
// No float atomic on any output, db included; every sum has one fixed order.
#pragma once
#include "kernels_attn_bf16.h"
#include "kernels_bf16_drop.h"

namespace graphop {

// the dropout decision of the call's heads: global head of local head k is head0 + k
struct AttnBf16Drop {
  DropArgs<float> d;
  int head0;
};
template <bool DROP>
using AttnBf16DropIf = std::conditional_t<DROP, AttnBf16Drop, NoDrop>;

typedef unsigned short bf16_bits_t;   // one bf16 value of b / db as it lies in memory

__device__ __forceinline__ float attn_bf16_widen(bf16_bits_t x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ bf16_bits_t attn_bf16_round1(float x) { return (bf16_bits_t)(bf16_pack2(x, 0.f) & 0xffffu); }

// ---- forward: k_attn_bf16_fwd_rows' walk and online softmax with the options ---------------------------------------------
template <int H, int D, bool DROP, bool BIAS>
__global__ __launch_bounds__(kFastBlock) void k_attnopt_bf16_fwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnBf16FwdArgs a, const bf16_bits_t* __restrict__ b, i64 n_chunks,
    int chunks_per_group, AttnBf16DropIf<DROP> dr) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
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
  uint4 q[NV];
  Bf16Acc o_c[NV];
  float m_c[NV], l_c[NV];   // of the piece's head; l of the undropped exp
  auto finish = [&](i64 r) {
    if (r == row_before || r == row_after) {
      const i64 pi = attn_bf16_rec_slot(gid, r, row_before);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        attn_bf16_rec_store(a.p_o, pi * F8 + v * L + l, o_c[v]);
        if (l % DQ == 0) reinterpret_cast<float2*>(a.p_ml)[pi * H + kv[v]] = make_float2(m_c[v], l_c[v]);
      }
      if (l == 0) a.p_row[pi] = attn_bf16_rec_word(r, row_before, row_after);
    } else {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (l_c[v] > 0.f) {   // (the same for every head: a row has slots or has none)
          float f;
          const float2 st = attn_bf16_stats(m_c[v], l_c[v], f);
          attn_bf16_scale(o_c[v], f);
          a.o[r * F8 + v * L + l] = attn_bf16_round(o_c[v]);
          if (l % DQ == 0 && st.y > 0.f) reinterpret_cast<float2*>(a.stats)[r * H + kv[v]] = st;
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
        q[v] = a.Q[r * F8 + v * L + l];
        attn_bf16_zero(o_c[v]);
        m_c[v] = kAttnNegBig;
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
      uint4 x0[SB][NV], x1[SB][NV];
      float bb[BIAS ? SB : 1][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* kp = a.K + src * F8 + l;
        const uint4* vp = a.V + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
      if constexpr (BIAS) {   // the slots' bias values of this lane's heads, behind the row requests
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const i64 e = group_bcast<L, u>(my_e);
#pragma unroll
          for (int v = 0; v < NV; ++v) bb[u][v] = attn_bf16_widen(b[e * H + kv[v]]);
        });
      }
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = bf16_keep_bits<H, SB, L>(l, (unsigned)cur_row, (unsigned)my_src, dr.d, dr.head0);
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
          s[u] = group_sum<DQ>(attn_bf16_dot(q[v], x0[u][v]));
          if constexpr (BIAS) s[u] += bb[u][v];
          if (u < nb) mx = fmaxf(mx, s[u]);   // group-uniform
        }
        const float sc = attn_rows_exp(m_c[v] - mx);
        l_c[v] *= sc;
        attn_bf16_scale(o_c[v], sc);
        m_c[v] = mx;
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          if (u < nb) {
            const float p = attn_rows_exp(s[u] - mx);
            l_c[v] += p;
            float pm = p;
            if constexpr (DROP) pm = (keep[u] >> kv[v]) & 1 ? p * dr.d.scale : 0.f;
            attn_bf16_fma(o_c[v], pm, x1[u][v]);
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- backward: k_attn_bf16_bwd_rows' walk with the options -----------------------------------------------------------------
//   COL = false: OWN = (Q | dO) packed [n_q][2 F8], XT = (K | V) packed, out0 = dQ; with DB, db[eid[slot], k] = bf16(ds)
//   COL = true : OWN = (K | V) packed [n_k][2 F8], XT = (Q | dO) packed, out0 = dK, out1 = dV; eid is the column-major
//                one and db is not touched (DB is false)
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.  a = exp(s - m) / l,
// da = mult <dO_i, V_j>, ds = a (da - D); dQ / dK take ds, dV takes a mult.  The keep decision's (i, j) is (row-major row,
// neighbour) in both passes: (own, gathered) in the row pass, (gathered, own) in the column pass.
template <int H, int D, bool COL, bool DROP, bool BIAS, bool DB>
__global__ __launch_bounds__(kFastBlock) void k_attnopt_bf16_bwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const uint4* __restrict__ OWN, const uint4* __restrict__ XT,
    const float4* __restrict__ stats4, const bf16_bits_t* __restrict__ b, uint4* __restrict__ out0,
    uint4* __restrict__ out1, bf16_bits_t* __restrict__ db, AttnBf16BwdRec rec, i64 n_chunks, int chunks_per_group,
    AttnBf16DropIf<DROP> dr) {
  static_assert(!DB || (BIAS && !COL), "db is the row pass's, and only with a bias");
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB, NOUT = COL ? 2 : 1;
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
  uint4 y0[NV], y1[NV];
  Bf16Acc acc0[NV], acc1[COL ? NV : 1];
  float4 own_st[COL ? 1 : NV];   // ROW: (m, 1 / l, D) of the piece's head
  auto zero_acc = [&]() {
#pragma unroll
    for (int v = 0; v < NV; ++v) attn_bf16_zero(acc0[v]);
#pragma unroll
    for (int v = 0; v < (COL ? NV : 1); ++v) attn_bf16_zero(acc1[v]);
  };
  auto flush = [&](i64 r) {
    if (r != row_before && r != row_after) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        out0[r * F8 + v * L + l] = attn_bf16_round(acc0[v]);
        if constexpr (COL) out1[r * F8 + v * L + l] = attn_bf16_round(acc1[v]);
      }
    } else {
      const i64 pi = attn_bf16_rec_slot(gid, r, row_before);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        attn_bf16_rec_store(rec.p_acc, pi * NOUT * F8 + v * L + l, acc0[v]);
        if constexpr (COL) attn_bf16_rec_store(rec.p_acc, pi * NOUT * F8 + F8 + v * L + l, acc1[v]);
      }
      if (l == 0) rec.p_row[pi] = attn_bf16_rec_word(r, row_before, row_after);
    }
  };
  i64 cur_row = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = row[c];
    if (r != cur_row) {
      if (cur_row >= 0) flush(cur_row);
      zero_acc();
      cur_row = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        y0[v] = OWN[r * 2 * F8 + v * L + l];
        y1[v] = OWN[r * 2 * F8 + F8 + v * L + l];
        if constexpr (!COL) own_st[v] = stats4[r * H + kv[v]];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the ids of slot l % SB; slots past the end re-read the batch's last slot with weights 0
      const int t = l % SB;
      const i64 j = jb + (t < nb ? t : nb - 1);
      const int my_src = (int)indices[j];
      int my_e = 0;
      if constexpr (BIAS) my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      uint4 x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
      float bb[BIAS ? SB : 1][NV];
      int ed[DB ? SB : 1];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* rowp = XT + src * (2 * F8) + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = rowp[v * L]; x1[u][v] = rowp[F8 + v * L]; }
        if constexpr (COL) {
#pragma unroll
          for (int v = 0; v < NV; ++v) stg[u][v] = stats4[src * H + kv[v]];
        }
      });
      if constexpr (BIAS) {   // the slots' bias values of this lane's heads, behind the row requests
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const int e = group_bcast<L, u>(my_e);
          if constexpr (DB) ed[u] = e;
#pragma unroll
          for (int v = 0; v < NV; ++v) bb[u][v] = attn_bf16_widen(b[(i64)e * H + kv[v]]);
        });
      }
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = COL ? bf16_keep_bits<H, SB, L>(l, (unsigned)my_src, (unsigned)cur_row, dr.d, dr.head0)
                             : bf16_keep_bits<H, SB, L>(l, (unsigned)cur_row, (unsigned)my_src, dr.d, dr.head0);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          // the Q-side words first in both passes: the forward's chain, then the forward's one add
          float s = group_sum<DQ>(COL ? attn_bf16_dot(x0[u][v], y0[v]) : attn_bf16_dot(y0[v], x0[u][v]));
          float da = group_sum<DQ>(COL ? attn_bf16_dot(x1[u][v], y1[v]) : attn_bf16_dot(y1[v], x1[u][v]));
          if constexpr (BIAS) s += bb[u][v];
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          float mult = 1.f;
          if constexpr (DROP) mult = (keep[u] >> kv[v]) & 1 ? dr.d.scale : 0.f;
          if constexpr (DROP) da *= mult;
          const float ds = av * (da - st.z);
          if constexpr (DROP) av *= mult;   // from here on av weights dO only: a_e mult_e
          if constexpr (DB) {   // the head's first lane, real slots only
            if (u < nb && l % DQ == 0) db[(i64)ed[u] * H + kv[v]] = attn_bf16_round1(ds);
          }
          attn_bf16_fma(acc0[v], ds, x0[u][v]);                       // dQ += ds K_j, or dK += ds Q_i
          if constexpr (COL) attn_bf16_fma(acc1[v], av, x1[u][v]);    // dV += a mult dO_i
        }
      }
    }
  }
  if (cur_row >= 0) flush(cur_row);
}

}  // namespace graphop
