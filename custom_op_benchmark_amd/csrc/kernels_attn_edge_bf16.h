// The bfloat16 fused attention step with edge features, s_e = <Q_i, K_j + xe[e]>, o_i = sum_e a_e mult_e (V_j + xe[e]),
// and attention dropout as an option (attention_edge_bf16.hip has the host side).  The semantics are
// graphop_attention_edge_*'s (4.5m); tables, layout, record scheme and arithmetic are those of kernels_attn_bf16.h /
// kernels_attn_bf16_opts.h: AttnBf16Cfg<H, D>, 16-byte pieces, lane groups of L = min(16, F8) lanes, rows shared between
// lane groups leave as fp32 records.  The pack kernel and the merge kernels are kernels_attn_bf16.h's, unchanged: the
// records hold the same things.  The kernels here are text of their own, so that no existing kernel changes.
//
// What the edge row adds to a pass:
//   no kx, no vx  K_j + xe[e] as a packed bf16 value would be rounded a second time.  A head's score is ONE chain of
//              v_dot2 (edge_bf16_chain), the Q-side word always first: over the four words of K_j's piece and then, with
//              the running sum as the accumulator, over the four words of xe[e]'s piece; group_sum<DQ> follows.  That is
//              exact in its inputs, fp32 throughout, and the same expression in the same order in the forward, the row
//              pass and the column pass, so the backward's s is the forward's bit for bit.  da is the same chain with dO_i
//              on the Q side over V_j and then xe[e].  The value side and dQ take two attn_bf16_fma per piece -- the weight
//              times V_j (K_j), then times xe[e] -- both unpacked where they are consumed.
//   three pieces  a slot brings three pieces per lane and piece index, not two: EdgeBf16Cfg<H, D>::SB slots per batch are
//              chosen per NV from the compiler's register report (4.5y has the table).  xe's words stay a third array
//              beside x0 / x1 and are never merged into the gathered pieces: they are consumed exactly twice, by the score
//              and by the value (the row pass: score, da and dQ).
//   load order    xe[e] comes from HBM, each row once per pass: non-temporal 16-byte loads at the 64-bit offset e * F8,
//              issued for the whole batch BEFORE the gathers of K_j / V_j, which mostly hit L2.  The lane that holds a
//              slot's neighbour id also loads its edge id (a NULL eid says eid[slot] == slot, a kernel-uniform branch; the
//              column pass is given the column-major eid) and hands it round the group like the neighbour id.
//   dxe           the row pass alone: the row-major orientation visits each slot once, so per lane, piece and real slot
//              (u < nb) there is one plain non-temporal 16-byte store of attn_bf16_round(ds Q_i + a mult dO_i), rounded once.
//              dxe == NULL is a kernel-uniform run-time check, as in 4.5m: nothing edge-sized is then written.  The
//              column pass reads xe[eid_c[slot]], a random 2 H D-byte row per slot -- inherent, 4.5m -- and writes dK, dV
//              and nothing edge-sized.
//   dropout       bf16_keep_bits<H, SB, L> (kernels_bf16_drop.h) as in kernels_attn_bf16_opts.h; stats are those of the
//              UNDROPPED scores.
// No float atomic anywhere; every sum has one fixed order, so two runs agree bit for bit, dxe included.
// Matrix instructions do not fit, for 4.5s's reason: a slot's score is one row against one row.
#pragma once
#include "kernels_attn_bf16_opts.h"

namespace graphop {

// Slots per batch of the edge passes.  A slot holds three pieces per piece index in flight, so AttnBf16Cfg's SB = 8 / NV
// would be 24 pieces per lane: that fits at NV = 1 and NV = 2 (at most 206 and 231 VGPRs) and not at NV = 4 (up to 299),
// where SB = 2 is also the plain step's batch.  NV = 4 therefore takes one slot per batch: 12 pieces, at most 247 VGPRs.
template <int H, int D>
struct EdgeBf16Cfg {
  static constexpr int NV = AttnBf16Cfg<H, D>::NV;
  static constexpr int SB = NV == 4 ? 1 : 8 / NV;
};

typedef unsigned edge_bf16_u4 __attribute__((ext_vector_type(4)));

// one piece of an edge row, streamed once: kept out of the caches
__device__ __forceinline__ uint4 edge_bf16_ld_nt(const uint4* p) {
  const edge_bf16_u4 v = __builtin_nontemporal_load(reinterpret_cast<const edge_bf16_u4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void edge_bf16_st_nt(uint4* p, const uint4& x) {
  const edge_bf16_u4 v = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(v, reinterpret_cast<edge_bf16_u4*>(p));
}

// the lane's share of <qside, kside + xside>: qside's words first, over kside's four words and then, the running sum as
// the accumulator, over xside's four (one order everywhere, see above)
__device__ __forceinline__ float edge_bf16_chain(const uint4& qside, const uint4& kside, const uint4& xside) {
  float s = attn_bf16_dot(qside, kside);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.x), __builtin_bit_cast(bf16x2_t, xside.x), s, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.y), __builtin_bit_cast(bf16x2_t, xside.y), s, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.z), __builtin_bit_cast(bf16x2_t, xside.z), s, false);
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.w), __builtin_bit_cast(bf16x2_t, xside.w), s, false);
}

// ---- forward: k_attnopt_bf16_fwd_rows' walk and online softmax with the edge row ------------------------------------------
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_edge_bf16_fwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnBf16FwdArgs a, const uint4* __restrict__ xe, i64 n_chunks, int chunks_per_group,
    AttnBf16DropIf<DROP> dr) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = EdgeBf16Cfg<H, D>::SB;
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
      const int my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      uint4 xr[SB][NV], x0[SB][NV], x1[SB][NV];
      static_for<SB>([&](auto uc) {   // the edge rows first: they come from HBM
        constexpr int u = decltype(uc)::value;
        const uint4* ep = xe + (i64)group_bcast<L, u>(my_e) * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) xr[u][v] = edge_bf16_ld_nt(ep + v * L);
      });
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* kp = a.K + src * F8 + l;
        const uint4* vp = a.V + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
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
          s[u] = group_sum<DQ>(edge_bf16_chain(q[v], x0[u][v], xr[u][v]));
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
            attn_bf16_fma(o_c[v], pm, x1[u][v]);   // o += a mult V_j ...
            attn_bf16_fma(o_c[v], pm, xr[u][v]);   // ... + a mult xe[e]
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- backward: k_attnopt_bf16_bwd_rows' walk with the edge row -------------------------------------------------------------
//   COL = false: OWN = (Q | dO) packed [n_q][2 F8], XT = (K | V) packed, out0 = dQ; eid is the row-major one and, with
//                dxe != NULL, dxe[eid[slot]] = bf16(ds Q_i + a mult dO_i) for the real slots
//   COL = true : OWN = (K | V) packed [n_k][2 F8], XT = (Q | dO) packed, out0 = dK, out1 = dV; eid is the column-major
//                one and dxe is not touched
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.  a = exp(s - m) / l,
// da = mult <dO_i, V_j + xe[e]>, ds = a (da - D); dQ takes ds (K_j + xe[e]), dK takes ds Q_i, dV takes a mult dO_i.  The
// keep decision's (i, j) is (row-major row, neighbour) in both passes.
template <int H, int D, bool COL, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_edge_bf16_bwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const uint4* __restrict__ OWN, const uint4* __restrict__ XT,
    const float4* __restrict__ stats4, const uint4* __restrict__ xe, uint4* __restrict__ out0, uint4* __restrict__ out1,
    uint4* __restrict__ dxe, AttnBf16BwdRec rec, i64 n_chunks, int chunks_per_group, AttnBf16DropIf<DROP> dr) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = EdgeBf16Cfg<H, D>::SB, NOUT = COL ? 2 : 1;
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
      const int my_e = eid ? (int)eid[j] : (int)j;   // kernel-uniform branch
      uint4 xr[SB][NV], x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
      i64 ed[COL ? 1 : SB];           // ROW: the slots' piece offsets in dxe
      static_for<SB>([&](auto uc) {   // the edge rows first: they come from HBM
        constexpr int u = decltype(uc)::value;
        const i64 eo = (i64)group_bcast<L, u>(my_e) * F8 + l;
        if constexpr (!COL) ed[u] = eo;
#pragma unroll
        for (int v = 0; v < NV; ++v) xr[u][v] = edge_bf16_ld_nt(xe + eo + v * L);
      });
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
          // the Q-side words first in both passes: the forward's chain
          const float s = group_sum<DQ>(COL ? edge_bf16_chain(x0[u][v], y0[v], xr[u][v]) : edge_bf16_chain(y0[v], x0[u][v], xr[u][v]));
          float da = group_sum<DQ>(COL ? edge_bf16_chain(x1[u][v], y1[v], xr[u][v]) : edge_bf16_chain(y1[v], x1[u][v], xr[u][v]));
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          float mult = 1.f;
          if constexpr (DROP) mult = (keep[u] >> kv[v]) & 1 ? dr.d.scale : 0.f;
          if constexpr (DROP) da *= mult;
          const float ds = av * (da - st.z);
          if constexpr (DROP) av *= mult;   // from here on av weights dO only: a_e mult_e
          attn_bf16_fma(acc0[v], ds, x0[u][v]);   // dQ += ds K_j, or dK += ds Q_i
          if constexpr (COL) {
            attn_bf16_fma(acc1[v], av, x1[u][v]);   // dV += a mult dO_i
          } else {
            attn_bf16_fma(acc0[v], ds, xr[u][v]);   // dQ += ds xe[e]
            if (dxe != nullptr && u < nb) {         // (kernel-uniform, then group-uniform) each real slot once
              Bf16Acc g;
              attn_bf16_zero(g);
              attn_bf16_fma(g, ds, y0[v]);   // ds Q_i
              attn_bf16_fma(g, av, y1[v]);   // + a mult dO_i
              edge_bf16_st_nt(dxe + ed[u] + v * L, attn_bf16_round(g));
            }
          }
        }
      }
    }
  }
  if (cur_row >= 0) flush(cur_row);
}

}  // namespace graphop
