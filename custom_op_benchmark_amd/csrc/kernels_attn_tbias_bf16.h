// The bfloat16 fused attention step with an edge-type score bias, s_e = <Q_i, K_j> + B[t_e, k], and attention dropout as
// an option (attention_tbias_bf16.hip has the host side).  The semantics are graphop_attention_tbias_*'s
// (4.5p); tables, layout, record scheme and arithmetic are those of kernels_attn_bf16.h / kernels_attn_bf16_opts.h:
// AttnBf16Cfg<H, D>, 16-byte pieces, lane groups of L = min(16, F8) lanes, SB = 8 / NV slots per batch, rows shared between
// lane groups leave as fp32 records.  The pack kernel and the merge kernels are kernels_attn_bf16.h's, unchanged.  The
// kernels here are text of their own, so that no existing kernel changes.
//
// What the table adds to a pass:
//   B in LDS   every workgroup copies B (bf16, W = n_types * H words) into dynamic LDS once, widened exactly to fp32; a
//              slot's bias is then an LDS read of word t * H + k.  Nothing edge-sized is read but the 4-byte type.
//   types      the lane that holds a slot's neighbour id also loads the edge id (a NULL eid says eid[slot] == slot, a
//              kernel-uniform branch; the column pass is given the column-major eid) and then etype[e]; it clamps the type,
//              t = min((unsigned) etype[e], tmax), BEFORE any address is formed from it, and hands t round the group.
//   s          group_sum<DQ>(dot chain) + Bs[t * H + k]: ONE fp32 add after the reduction, the same expression in the
//              forward, the row pass and the column pass, so the backward's s is the forward's bit for bit.
//   dropout    bf16_keep_bits<H, SB, L> (kernels_bf16_drop.h) as in kernels_attn_bf16_opts.h; stats are those of the
//              biased, UNDROPPED scores.
//   dB         the row pass with DB.  Each lane group owns a private fp32 table of W words in LDS, zeroed at the start.
//              Word (t, k) of a group's table has one owner lane -- the head's first lane (l % DQ == 0) of the piece whose
//              head is k -- which does a plain read-add-write of ds for the real slots u < nb, in slot order: a group's
//              table is a sum in one fixed order.  After a barrier the workgroup sums its groups' tables word by word in
//              group order and writes one full partial table of Wp = up256(4 W) / 4 words into the workspace, row
//              blockIdx.x.  k_tbias_bf16_db_reduce then sums the partial tables in a tree of fixed shape (a function of the
//              number of workgroups alone), rounds once and writes EVERY element of dB; types no edge carries get exactly 0.
// Every thread meets the barriers: lane groups past the last chunk walk no chunk, they do not return early.
// No float atomic anywhere; every sum has one fixed order, so two runs agree bit for bit, dB included.
// Matrix instructions do not fit, for 4.5s's reason: a slot's score is one row against one row.
//
// LDS: 4 W bytes for B, plus, in the row pass with DB, (kFastBlock / L) * 4 W for the groups' tables: at the bound
// W = kTbiasBf16MaxWords = 512 and L = 8 that is 2 KiB + 32 * 2 KiB = 66 KiB, above the 64 KiB a kernel gets by default, so
// the host raises the kernel's maximum dynamic LDS once per instantiation.  Two such workgroups fit the CU's 160 KiB.
// Workspace: the plain bf16 step's, plus, last in the backward's, n_workgroups * up256(4 W) bytes of partial tables (not
// touched without dB).  That grows with the number of chunks: about 28 MB at the Reddit shape (14 K workgroups of the row
// pass) at the bound.
#pragma once
#include "kernels_attn_bf16_opts.h"

namespace graphop {

constexpr i64 kTbiasBf16MaxWords = 512;   // n_types * h at most
constexpr int kTbiasBf16Fan = 64;         // segments of the reduce tree's first level at most

// the table and the types as the kernels take them
struct TbiasBf16Tab {
  const bf16_bits_t* B;   // [tmax + 1][H]
  const int* etype;       // [n_edges], by edge id
  unsigned tmax;          // n_types - 1
  int words;              // (tmax + 1) * H
};

// B -> LDS, widened; `extra` further words behind it are zeroed (the groups' tables of dB).  Ends in the barrier.
__device__ __forceinline__ void tbias_bf16_stage(float* lds, const TbiasBf16Tab& tb, int extra) {
  for (int i = threadIdx.x; i < tb.words; i += kFastBlock) lds[i] = attn_bf16_widen(tb.B[i]);
  for (int i = threadIdx.x; i < extra; i += kFastBlock) lds[tb.words + i] = 0.f;
  __syncthreads();
}

// the clamped type of slot j, read behind the edge id by the lane that holds the slot's neighbour id
__device__ __forceinline__ int tbias_bf16_type(const i64* __restrict__ eid, i64 j, const TbiasBf16Tab& tb) {
  const i64 e = eid ? eid[j] : j;   // kernel-uniform branch
  const unsigned t = (unsigned)tb.etype[e];
  return (int)(t < tb.tmax ? t : tb.tmax);
}

// ---- forward: k_attnopt_bf16_fwd_rows' walk and online softmax with the bias read from LDS ----------------------------------
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_tbias_bf16_fwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnBf16FwdArgs a, TbiasBf16Tab tb, i64 n_chunks, int chunks_per_group,
    AttnBf16DropIf<DROP> dr) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
  constexpr i64 F8 = C::F8;
  extern __shared__ float tbias_lds[];
  const float* Bs = tbias_lds;
  tbias_bf16_stage(tbias_lds, tb, 0);
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;   // (behind the only barrier)
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
      const int my_t = tbias_bf16_type(eid, j, tb);
      uint4 x0[SB][NV], x1[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* kp = a.K + src * F8 + l;
        const uint4* vp = a.V + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
      float bb[SB][NV];   // the slots' bias values of this lane's heads, from LDS behind the row requests
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const int ty = group_bcast<L, u>(my_t);
#pragma unroll
        for (int v = 0; v < NV; ++v) bb[u][v] = Bs[ty * H + kv[v]];
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
          s[u] = group_sum<DQ>(attn_bf16_dot(q[v], x0[u][v])) + bb[u][v];
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

// ---- backward: k_attnopt_bf16_bwd_rows' walk with the bias read from LDS ---------------------------------------------------
//   COL = false: OWN = (Q | dO) packed [n_q][2 F8], XT = (K | V) packed, out0 = dQ; with DB the workgroup's partial table
//                of dB goes to partial[blockIdx.x][wp]
//   COL = true : OWN = (K | V) packed [n_k][2 F8], XT = (Q | dO) packed, out0 = dK, out1 = dV; eid is the column-major
//                one and no table of dB exists (DB is false)
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.  a = exp(s - m) / l,
// da = mult <dO_i, V_j>, ds = a (da - D); dQ / dK take ds, dV takes a mult.
template <int H, int D, bool COL, bool DROP, bool DB>
__global__ __launch_bounds__(kFastBlock) void k_tbias_bf16_bwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const uint4* __restrict__ OWN, const uint4* __restrict__ XT,
    const float4* __restrict__ stats4, TbiasBf16Tab tb, uint4* __restrict__ out0, uint4* __restrict__ out1,
    float* __restrict__ partial, int wp, AttnBf16BwdRec rec, i64 n_chunks, int chunks_per_group,
    AttnBf16DropIf<DROP> dr) {
  static_assert(!DB || !COL, "dB is the row pass's");
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB, NOUT = COL ? 2 : 1, G = kFastBlock / L;
  constexpr i64 F8 = C::F8;
  extern __shared__ float tbias_lds[];
  const float* Bs = tbias_lds;
  const int W = tb.words;
  tbias_bf16_stage(tbias_lds, tb, DB ? G * W : 0);
  const int l = threadIdx.x % L;
  float* tab = tbias_lds + W + (threadIdx.x / L) * W;   // DB: this lane group's table of dB
  const i64 gid = (i64)blockIdx.x * G + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  const bool live = c0 < c1;   // a group past the last chunk walks no chunk and meets the barrier below
  if constexpr (!DB) {
    if (!live) return;   // (behind the only barrier)
  }
  const i64 row_before = live && c0 > 0 ? row[c0 - 1] : -1;
  const i64 row_after = live && c1 < n_chunks ? row[c1] : -1;
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
      const int my_t = tbias_bf16_type(eid, j, tb);
      uint4 x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
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
      float bb[SB][NV];   // the slots' bias values of this lane's heads, from LDS behind the row requests
      int ty[DB ? SB : 1];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const int tu = group_bcast<L, u>(my_t);
        if constexpr (DB) ty[u] = tu * H;
#pragma unroll
        for (int v = 0; v < NV; ++v) bb[u][v] = Bs[tu * H + kv[v]];
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
          // the Q-side words first in both passes: the forward's chain, then the forward's one add
          const float s = group_sum<DQ>(COL ? attn_bf16_dot(x0[u][v], y0[v]) : attn_bf16_dot(y0[v], x0[u][v])) + bb[u][v];
          float da = group_sum<DQ>(COL ? attn_bf16_dot(x1[u][v], y1[v]) : attn_bf16_dot(y1[v], x1[u][v]));
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          float mult = 1.f;
          if constexpr (DROP) mult = (keep[u] >> kv[v]) & 1 ? dr.d.scale : 0.f;
          if constexpr (DROP) da *= mult;
          const float ds = av * (da - st.z);
          if constexpr (DROP) av *= mult;   // from here on av weights dO only: a_e mult_e
          if constexpr (DB) {   // the word's one owner, real slots only, in slot order
            if (u < nb && l % DQ == 0) tab[ty[u] + kv[v]] += ds;
          }
          attn_bf16_fma(acc0[v], ds, x0[u][v]);                       // dQ += ds K_j, or dK += ds Q_i
          if constexpr (COL) attn_bf16_fma(acc1[v], av, x1[u][v]);    // dV += a mult dO_i
        }
      }
    }
  }
  if (cur_row >= 0) flush(cur_row);
  if constexpr (DB) {
    __syncthreads();
    const float* tabs = tbias_lds + W;
    for (int w = threadIdx.x; w < W; w += kFastBlock) {
      float sum = 0.f;
      for (int g = 0; g < G; ++g) sum += tabs[g * W + w];   // group order
      partial[(i64)blockIdx.x * wp + w] = sum;
    }
  }
}

// One level of the tree over the partial tables.  Table i lies at in[i * stride] (W words of it count); segment
// blockIdx.y covers tables [blockIdx.y * per, min(n, (blockIdx.y + 1) * per)) and a workgroup 64 consecutive words:
// wave q of the workgroup sums the segment's tables q, q + 4, ... in that order, and the four sums are added in wave
// order.  dB == NULL: the segment's sum replaces its own first table (fp32, in place: no other workgroup reads or writes
// those words); else it is rounded once into dB[w] (the last level: one segment).
__global__ __launch_bounds__(256) void k_tbias_bf16_db_reduce(float* __restrict__ in, i64 n, i64 stride, i64 per,
                                                              bf16_bits_t* __restrict__ dB, int W) {
  __shared__ float part[4][64];
  const int wl = threadIdx.x % 64, q = threadIdx.x / 64;
  const int w = blockIdx.x * 64 + wl;
  const i64 i0 = (i64)blockIdx.y * per;
  i64 i1 = i0 + per;
  if (i1 > n) i1 = n;
  float sum = 0.f;
  if (w < W)
    for (i64 i = i0 + q; i < i1; i += 4) sum += in[i * stride + w];
  part[q][wl] = sum;
  __syncthreads();
  if (q == 0 && w < W) {
    const float total = ((part[0][wl] + part[1][wl]) + part[2][wl]) + part[3][wl];
    if (dB) dB[w] = attn_bf16_round1(total);
    else in[i0 * stride + w] = total;
  }
}

}  // namespace graphop
