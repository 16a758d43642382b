// The bfloat16 fused attention step with edge-type embeddings, s_e = <Q_i, K_j + R[t_e]>, o_i = sum_e a_e mult_e (V_j + R[t_e]),
// and attention dropout as an option (attention_etype_bf16.hip has the host side).  The semantics are
// graphop_attention_etype_*'s (4.5o); tables, layout, record scheme and arithmetic are those of the bf16 edge step
// (kernels_attn_edge_bf16.h, 4.5y) with xe[e] := R[t_e]: AttnBf16Cfg<H, D>, 16-byte pieces, lane groups of L = min(16, F8)
// lanes, EdgeBf16Cfg<H, D>::SB slots per batch, three pieces per slot, the score ONE fp32 edge_bf16_chain over K_j's words
// and then R[t_e]'s, two attn_bf16_fma per piece on the value side and in dQ.  The pack kernel and the merge kernels are
// kernels_attn_bf16.h's, unchanged: the records hold the same things.  The kernels here are text of their own, so that no
// existing kernel changes.
//
// What the table adds to a pass:
//   R in LDS   every workgroup copies R (bf16, 2 T F bytes, F = H D) into dynamic LDS once and keeps it PACKED: a slot's
//              third piece is one 16-byte LDS read at piece index t * F8 + v * L + l, where the edge step has a
//              non-temporal global load.  Nothing edge-sized is read but the 4-byte type (and the edge id).
//   types      the lane that holds a slot's neighbour id also loads the edge id (a NULL eid says eid[slot] == slot, a
//              kernel-uniform branch; the column pass is given the column-major eid) and then etype[e]; it clamps the type,
//              t = min((unsigned) etype[e], tmax), BEFORE any address is formed from it, and hands t round the group.
//   dR         the row pass with DR.  dR is T F words of vector sums, so a table per lane group (4.5x's scheme for dB)
//              would take (256 / L) 4 T F bytes: 128 KiB at T F = 1024.  Instead each of the workgroup's four WAVES owns
//              one fp32 table of T F words in LDS, zeroed at the start, and the wave's 64 / L lane groups TAKE TURNS in
//              group order: in its turn a group's lanes do a plain read-add-write of their eight words of
//              ds Q_i + a mult dO_i per piece, for the real slots u < nb, in slot order.  A wave's table is therefore one
//              sum in one order that the code and the graph fix.  The turns are kept apart by a wavefront-scope fence and
//              a wave barrier: each thread does one read-add-write per round of turns, and without them the compiler could
//              fold the turns into one concurrent access, in which two groups that hold the same type would lose an add.
//   partials   a workgroup with DR keeps its tables across a run of the VIRTUAL workgroups the plain launch would have:
//              the grid is min(kEtypeBf16Parts, virtual workgroups), workgroup b walks the virtual workgroups
//              [b n / grid, (b + 1) n / grid), and the virtual gid drives attn_bf16_rec_slot, so records and merge are
//              the plain launch's.  At its end, behind a barrier, the workgroup adds its four tables word by word in wave
//              order and writes ONE partial table, row blockIdx.x of the workspace's last part.  k_etype_bf16_dr_reduce
//              sums the partial tables in a tree whose shape follows from their number alone, rounds once and writes EVERY
//              element of dR; types no edge carries get exactly 0.
// Every thread meets every barrier: lane groups past the last chunk walk no chunk, they do not return early.
// No float atomic anywhere, in LDS or in global memory; two runs agree bit for bit, dR included.
// Matrix instructions do not fit, for 4.5s's reason: a slot's score is one row against one row, and a slot's share of dR
// is a rank-one update of ONE table row that the slot's type picks.
//
// LDS: 2 T F bytes for R, plus, in the row pass with DR, 4 * 4 T F for the waves' tables: at the bound
// T F = kEtypeBf16MaxWords = 4096 that is 8 KiB + 64 KiB = 72 KiB, above the 64 KiB a kernel gets by default, so the host
// raises the kernel's maximum dynamic LDS once per instantiation.  Two such workgroups fit the CU's 160 KiB.
// Workspace: the plain bf16 step's, plus, last in the backward's, parts * up256(4 T F) bytes of partial tables (not
// touched without dR), parts = min(kEtypeBf16Parts, the row pass's virtual workgroups): at most 16 MiB.
#pragma once
#include "kernels_attn_edge_bf16.h"

namespace graphop {

constexpr i64 kEtypeBf16MaxWords = 4096;   // n_types * h * d at most (the fp32 op's kAttnEtypeTableBytes / 4)
constexpr int kEtypeBf16Parts = 1024;      // workgroups of the row pass with dR at most, each leaving one partial table
constexpr int kEtypeBf16Fan = 64;          // segments of the reduce tree's first level at most

// the table and the types as the kernels take them
struct EtypeBf16Tab {
  const uint4* R;      // [tmax + 1][F8] pieces
  const int* etype;    // [n_edges], by edge id
  unsigned tmax;       // n_types - 1
  int pieces;          // (tmax + 1) * F8
};

// R -> LDS, packed as it is; `extra` fp32 words behind it are zeroed (the waves' tables of dR).  Ends in the barrier.
__device__ __forceinline__ void etype_bf16_stage(uint4* lds, const EtypeBf16Tab& tb, int extra) {
  for (int i = threadIdx.x; i < tb.pieces; i += kFastBlock) lds[i] = tb.R[i];
  float* z = reinterpret_cast<float*>(lds + tb.pieces);
  for (int i = threadIdx.x; i < extra; i += kFastBlock) z[i] = 0.f;
  __syncthreads();
}

// the clamped type of slot j, read behind the edge id by the lane that holds the slot's neighbour id
__device__ __forceinline__ int etype_bf16_type(const i64* __restrict__ eid, i64 j, const EtypeBf16Tab& tb) {
  const i64 e = eid ? eid[j] : j;   // kernel-uniform branch
  const unsigned t = (unsigned)tb.etype[e];
  return (int)(t < tb.tmax ? t : tb.tmax);
}

// ---- forward: k_edge_bf16_fwd_rows' walk and online softmax with the edge piece read from LDS -----------------------------
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_etype_bf16_fwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnBf16FwdArgs a, EtypeBf16Tab tb, i64 n_chunks, int chunks_per_group,
    AttnBf16DropIf<DROP> dr) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = EdgeBf16Cfg<H, D>::SB;
  constexpr i64 F8 = C::F8;
  extern __shared__ uint4 etype_bf16_lds[];
  const uint4* Rs = etype_bf16_lds;
  etype_bf16_stage(etype_bf16_lds, tb, 0);
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
      const int my_t = etype_bf16_type(eid, j, tb);
      uint4 xr[SB][NV], x0[SB][NV], x1[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* kp = a.K + src * F8 + l;
        const uint4* vp = a.V + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
      static_for<SB>([&](auto uc) {   // the table rows from LDS, behind the row requests
        constexpr int u = decltype(uc)::value;
        const uint4* rp = Rs + group_bcast<L, u>(my_t) * (int)F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) xr[u][v] = rp[v * L];
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
            attn_bf16_fma(o_c[v], pm, xr[u][v]);   // ... + a mult R[t_e]
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- backward: k_edge_bf16_bwd_rows' walk with the edge piece read from LDS ------------------------------------------------
//   COL = false: OWN = (Q | dO) packed [n_q][2 F8], XT = (K | V) packed, out0 = dQ; eid is the row-major one; with DR the
//                workgroup's partial table of dR goes to partial[blockIdx.x][wp]
//   COL = true : OWN = (K | V) packed [n_k][2 F8], XT = (Q | dO) packed, out0 = dK, out1 = dV; eid is the column-major
//                one and no table of dR exists (DR is false)
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.  a = exp(s - m) / l,
// da = mult <dO_i, V_j + R[t_e]>, ds = a (da - D); dQ takes ds (K_j + R[t_e]), dK takes ds Q_i, dV takes a mult dO_i.  The
// keep decision's (i, j) is (row-major row, neighbour) in both passes.
// The workgroup walks the virtual workgroups [blockIdx.x n_vblocks / gridDim.x, (blockIdx.x + 1) n_vblocks / gridDim.x):
// exactly its own where the grid is n_vblocks (every launch without DR).
template <int H, int D, bool COL, bool DROP, bool DR>
__global__ __launch_bounds__(kFastBlock) void k_etype_bf16_bwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const uint4* __restrict__ OWN, const uint4* __restrict__ XT,
    const float4* __restrict__ stats4, EtypeBf16Tab tb, uint4* __restrict__ out0, uint4* __restrict__ out1,
    float* __restrict__ partial, int wp, AttnBf16BwdRec rec, i64 n_chunks, int chunks_per_group, i64 n_vblocks,
    AttnBf16DropIf<DROP> dr) {
  static_assert(!DR || !COL, "dR is the row pass's");
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = EdgeBf16Cfg<H, D>::SB, NOUT = COL ? 2 : 1, G = kFastBlock / L;
  constexpr int NG = 64 / L;   // lane groups of a wave: the turns
  constexpr i64 F8 = C::F8;
  constexpr int F = H * D;
  extern __shared__ uint4 etype_bf16_lds[];
  const uint4* Rs = etype_bf16_lds;
  const int W = tb.pieces * 8;   // words of a table of dR
  etype_bf16_stage(etype_bf16_lds, tb, DR ? 4 * W : 0);
  float* tabs = reinterpret_cast<float*>(etype_bf16_lds + tb.pieces);
  float* tab = tabs + (threadIdx.x / 64) * W;   // DR: this wave's table
  const int l = threadIdx.x % L;
  const int turn = (threadIdx.x % 64) / L;      // DR: this lane group's turn within its wave
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) kv[v] = attn_bf16_head<H, D>(v, l);
  auto walk = [&](const i64 gid) {   // one virtual lane group
    const i64 c0 = gid * chunks_per_group;
    i64 c1 = c0 + chunks_per_group;
    if (c1 > n_chunks) c1 = n_chunks;
    if (c0 >= c1) return;   // (walks no chunk; the kernel's barriers are outside)
    const i64 row_before = c0 > 0 ? row[c0 - 1] : -1;
    const i64 row_after = c1 < n_chunks ? row[c1] : -1;
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
        const int my_t = etype_bf16_type(eid, j, tb);
        uint4 xr[SB][NV], x0[SB][NV], x1[SB][NV];
        float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
        int ty[DR ? SB : 1];            // DR: the slots' word offsets in a table of dR
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
        static_for<SB>([&](auto uc) {   // the table rows from LDS, behind the row requests
          constexpr int u = decltype(uc)::value;
          const int tu = group_bcast<L, u>(my_t);
          if constexpr (DR) ty[u] = tu * F;
          const uint4* rp = Rs + tu * (int)F8 + l;
#pragma unroll
          for (int v = 0; v < NV; ++v) xr[u][v] = rp[v * L];
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
              attn_bf16_fma(acc0[v], ds, xr[u][v]);   // dQ += ds R[t_e]
            }
            if constexpr (DR) {
              Bf16Acc g;
              attn_bf16_zero(g);
              attn_bf16_fma(g, ds, y0[v]);   // ds Q_i
              attn_bf16_fma(g, av, y1[v]);   // + a mult dO_i
              float4* w = reinterpret_cast<float4*>(tab + ty[u] + (v * L + l) * 8);
              // the wave's lane groups in turn, real slots only: two groups may hold the same type, so the same words
#pragma unroll
              for (int k = 0; k < NG; ++k) {
                if (k == turn && u < nb) {
                  float4 w0 = w[0], w1 = w[1];
                  w0.x += g.a[0]; w0.y += g.a[1]; w0.z += g.a[2]; w0.w += g.a[3];
                  w1.x += g.a[4]; w1.y += g.a[5]; w1.z += g.a[6]; w1.w += g.a[7];
                  w[0] = w0; w[1] = w1;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
              }
            }
          }
        }
      }
    }
    if (cur_row >= 0) flush(cur_row);
  };
  const i64 vb0 = (i64)blockIdx.x * n_vblocks / gridDim.x, vb1 = ((i64)blockIdx.x + 1) * n_vblocks / gridDim.x;
  for (i64 vb = vb0; vb < vb1; ++vb) walk(vb * G + threadIdx.x / L);
  if constexpr (DR) {
    __syncthreads();
    for (int w = threadIdx.x; w < W; w += kFastBlock)   // wave order
      partial[(i64)blockIdx.x * wp + w] = ((tabs[w] + tabs[W + w]) + tabs[2 * W + w]) + tabs[3 * W + w];
  }
}

// One level of the tree over the partial tables.  Table i lies at in[i * stride] (W words of it count); segment
// blockIdx.y covers tables [blockIdx.y * per, min(n, (blockIdx.y + 1) * per)) and a workgroup 64 consecutive words:
// wave q of the workgroup sums the segment's tables q, q + 4, ... in that order, and the four sums are added in wave
// order.  dR == NULL: the segment's sum replaces its own first table (fp32, in place: no other workgroup reads or writes
// those words); else it is rounded once into dR[w] (the last level: one segment).
__global__ __launch_bounds__(256) void k_etype_bf16_dr_reduce(float* __restrict__ in, i64 n, i64 stride, i64 per,
                                                              bf16_bits_t* __restrict__ dR, int W) {
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
    if (dR) dR[w] = attn_bf16_round1(total);
    else in[i0 * stride + w] = total;
  }
}

}  // namespace graphop
