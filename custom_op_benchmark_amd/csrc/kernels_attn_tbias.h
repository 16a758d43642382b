// Fused dot-product attention with an edge-type score bias (graphop_attention_tbias_*): edge e = (i, j)
// carries a category t_e = etype[e] (by edge id) and the table holds one scalar per (category, head), added to the score:
//   s_e   = <Q_i, K_j> + B[t_e, k]      one add, after the dot product's reduction (as kernels_attn_bias.h)
//   everything else as the several-head passes with a per-edge bias (kernels_attn_rows_passes.inc, first inclusion) with
//   b[e, k] := B[t_e, k]
//   dB[t, k] = sum_{e : t_e = t} ds_e
// Nothing edge-sized exists but the int32 per edge.  Every kernel clamps the type into [0, n_types - 1] (one min on the
// unsigned value) before it forms an address: an out-of-range type gives an undefined value and touches no memory
// outside B / dB.
// The fast kernels are a text of their own, not a fourth inclusion of kernels_attn_rows_passes.inc: the bias here is no
// template parameter, the type is loaded where that text loads nothing, and the row pass keeps an LDS table of another
// shape than 4.5o's, so a shared text would have needed a macro at nearly every spot the three inclusions already vary
// in.  The layout, the walk, the piece records, the merge kernels and the pack kernels are those of that file
// (AttnRowsCfg<H, D>: a lane group of 16 lanes holds the row's F4 float4 pieces, piece p = v * L + l).
//   forward : the lane that holds a slot's ids loads t = etype[e] behind the edge id (e = eid[slot], or slot under an
//             identity plan), clamps it and broadcasts it; the slot's H bias values are cached loads of B[t * H + k_v]
//             issued behind the row requests (the table is 4 T h bytes)
//   column  : the same read of etype[eid_c[slot]] -- one random 4-byte read per slot, inherent to an operand indexed by
//             edge id -- writes dK, dV and nothing else
//   row     : writes dQ; with dB != NULL (kernel-uniform) the first lane of each head adds ds of the real slots into a
//             workgroup-wide dynamic LDS table tab[t * H + k] (4 T h bytes, given at the launch only when dB is wanted)
//             and at its end the workgroup adds the table's nonzero words into replica blockIdx.x % nrep of dB.  Groups
//             past the last chunk walk no chunk instead of leaving, so that every thread meets the barriers.
//             k_attn_tbias_db_reduce sums the replicas and writes every element of dB.
// The generic kernels (one wave per chunk, fp32 / fp64, any h and d, any chunk layout, any n_types) cover every other
// valid call: one score function (attn_tbias_score) and one place that reads and clamps a type (attn_tbias_of).
// This header emits kernels under fixed names, two of them (k_attn_tbias_piece_max, k_attn_tbias_db_reduce) no template,
// so it belongs to exactly one translation unit (attention_tbias.hip).
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

// The fast row pass holds 4 T h bytes of LDS when dB is wanted; beyond this many bytes that pass alone is the generic one.
constexpr i64 kAttnTbiasTableBytes = 16384;
constexpr i64 kAttnTbiasMaxWords = kAttnTbiasTableBytes / 4;   // n_types * h at most
// Replicas of dB the row pass's workgroups add into (blockIdx.x % kAttnTbiasReplicas): at most 1 MiB of workspace.
constexpr int kAttnTbiasReplicas = 64;

// the dropout decision of the call's heads: global head of local head k is head0 + k
struct AttnTbiasDrop {
  DropArgs<float> d;
  int head0;
};
template <bool DROP>
using AttnTbiasDropIf = std::conditional_t<DROP, AttnTbiasDrop, NoDrop>;

// Keep bits of a batch's slots, as the several-head passes take them: lane l works for slot l % SB, runs Philox for the
// blocks l / SB, l / SB + L / SB, ... of the blocks the global heads head0 .. head0 + H - 1 fall into, moves a block's
// four decisions to the local heads' bit positions, and the lanes of a slot OR their bits together.  Returns, in every
// lane with l % SB == u, slot u's bits (bit k = local head k is kept).  (i, j) = (row-major row, neighbour).
template <int H, int SB>
__device__ __forceinline__ int attn_tbias_keep_bits(int l, unsigned i, unsigned j, const AttnTbiasDrop& dr) {
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
struct AttnTbiasFwdArgs {
  const float* Q;       // [n_q][H][D]   own rows
  const float* K;       // [n_k][H][D]   gathered
  const float* V;       // [n_k][H][D]   gathered
  const float* B;       // [tmax + 1][H]
  const int* etype;     // [n_edges]     by edge id
  unsigned tmax;        // n_types - 1
  float* o;             // [n_q][H][D]   zero-filled by the caller (pieces are added)
  float* stats;         // [n_q][H][2]   (m, 1 / l); rows without slots keep the caller's fill (-1e9, 0)
  int* p_row;           // [2 * groups]  row | first-piece flag, -1 = none (pre-filled)
  float* p_ml;          // [2 * groups][H][2]
  float* p_o;           // [2 * groups][H][D]
};

// A lane group takes chunks_per_group consecutive chunks of a rows_sorted plan; rows inside the run are normalised and
// stored, rows shared with a neighbouring group leave as piece records in slot 2 * group + {0: continues from the group
// before, 1: continues into the group after}.  The online softmax is taken batch by batch: the heads' maxima over the
// batch first, one rescale of (l, o) per batch, then one exp per slot.
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_attn_tbias_fwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, AttnTbiasFwdArgs a, i64 n_chunks, int chunks_per_group, AttnTbiasDropIf<DROP> dr) {
  using C = AttnRowsCfg<H, D>;
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
          const float e = attn_rows_exp(m_c[v] - mf);
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
      const i64 my_e = eid ? eid[j] : j;   // kernel-uniform branch
      const int my_t = (int)min((unsigned)a.etype[my_e], a.tmax);   // the slot's type, clamped
      float4 x0[SB][NV], x1[SB][NV];
      float bb[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const float4* kp = reinterpret_cast<const float4*>(a.K) + src * F4 + l;
        const float4* vp = reinterpret_cast<const float4*>(a.V) + src * F4 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
      static_for<SB>([&](auto uc) {   // the slots' H bias values, behind the row requests
        constexpr int u = decltype(uc)::value;
        const int tu = group_bcast<L, u>(my_t);
#pragma unroll
        for (int v = 0; v < NV; ++v) bb[u][v] = a.B[tu * H + kv[v]];
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = attn_tbias_keep_bits<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
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
          s[u] = group_sum<DQ>(dot4(q[v], x0[u][v])) + bb[u][v];
          if (u < nb) mx = fmaxf(mx, s[u]);   // group-uniform
        }
        const float sc = attn_rows_exp(m_c[v] - mx);
        l_c[v] *= sc;
        o_c[v].x *= sc; o_c[v].y *= sc; o_c[v].z *= sc; o_c[v].w *= sc;
        m_c[v] = mx;
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          if (u < nb) {
            const float p = attn_rows_exp(s[u] - mx);
            l_c[v] += p;
            float pm = p;
            if constexpr (DROP) pm = (keep[u] >> kv[v]) & 1 ? p * dr.d.scale : 0.f;
            attn_rows_fma4(o_c[v], pm, x1[u][v]);
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// ---- merge of the shared rows' pieces: (m, l) per (piece, head) -----------------------------------------------------
// Mtmp[row, k] starts at kAttnNegBig, Ltmp[row, k] at 0, o is zero where pieces will be added.
__global__ void k_attn_tbias_piece_max(const int* __restrict__ p_row, const float* __restrict__ p_ml,
                                       float* __restrict__ Mtmp, i64 n, int h) {   // n = pieces * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int rec = p_row[i / h];
  if (rec < 0) return;
  atomic_max_float(Mtmp + (i64)(rec & kWalkRowMask) * h + i % h, p_ml[i * 2]);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_tbias_piece_add(
    const int* __restrict__ p_row, const float* __restrict__ p_ml, const float* __restrict__ p_o,
    const float* __restrict__ Mtmp, float* __restrict__ Ltmp, float* __restrict__ o, i64 n) {
  using C = AttnRowsCfg<H, D>;
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
    const float sc = attn_rows_exp(p_ml[(i * H + hd) * 2] - Mtmp[row * H + hd]);
    v[k] = reinterpret_cast<const float4*>(p_o)[i * F4 + k * L + l];
    v[k].x *= sc; v[k].y *= sc; v[k].z *= sc; v[k].w *= sc;
    if (l % DQ == 0) atomicAdd(Ltmp + row * H + hd, p_ml[(i * H + hd) * 2 + 1] * sc);
  }
  atomic_flush_dense<L, NV>(o, row, v, l);
}
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_tbias_piece_fin(
    const int* __restrict__ p_row, const float* __restrict__ Mtmp, const float* __restrict__ Ltmp,
    float* __restrict__ o, float* __restrict__ stats, i64 n) {
  using C = AttnRowsCfg<H, D>;
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
    const float e = attn_rows_exp(m - mf);
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
__global__ __launch_bounds__(kFastBlock) void k_attn_tbias_pack(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out, i64 n,
    const float* __restrict__ O, const float* __restrict__ stats2, float4* __restrict__ st4) {
  using C = AttnRowsCfg<H, D>;
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

//   COL = false: OWN = (Q | dO) packed [n_q][2F], XT = (K | V) packed, out0 = dQ; rep (may be NULL) is the replicas of dB
//   COL = true : OWN = (K | V) packed [n_k][2F], XT = (Q | dO) packed, out0 = dK, out1 = dV; rep is not touched
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.  The dynamic LDS table is
// [tmax + 1][H] words in the row pass with rep alone; the launch gives no byte otherwise.
template <int H, int D, bool COL, bool OWNED, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_attn_tbias_bwd_rows_f32(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const float* __restrict__ OWN, const float* __restrict__ XT,
    const float4* __restrict__ stats4, const float* __restrict__ B, const int* __restrict__ etype, unsigned tmax,
    int nrep, float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ rep, i64 n_chunks,
    int chunks_per_group, AttnTbiasDropIf<DROP> dr) {
  using C = AttnRowsCfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB;
  constexpr i64 F4 = C::F4;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = min(gid * chunks_per_group, n_chunks);   // groups past the last chunk walk none
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  extern __shared__ float tab[];
  const int n_tab = COL || rep == nullptr ? 0 : (int)(tmax + 1) * H;   // kernel-uniform
  for (int i = threadIdx.x; i < n_tab; i += kFastBlock) tab[i] = 0.f;
  if (n_tab) __syncthreads();
  i64 row_before = -1, row_after = -1;
  if constexpr (OWNED) {
    if (c0 > 0 && c0 < c1) row_before = row[c0 - 1];
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
      const i64 my_e = eid ? eid[j] : j;   // kernel-uniform branch
      const int my_t = (int)min((unsigned)etype[my_e], tmax);   // the slot's type, clamped
      float4 x0[SB][NV], x1[SB][NV];
      float4 stg[COL ? SB : 1][NV];   // COL: the gathered row's statistics
      float bb[SB][NV];
      int tt[SB];                     // the slots' table rows: t * H
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
      static_for<SB>([&](auto uc) {   // the slots' H bias values, behind the row requests
        constexpr int u = decltype(uc)::value;
        tt[u] = group_bcast<L, u>(my_t) * H;
#pragma unroll
        for (int v = 0; v < NV; ++v) bb[u][v] = B[tt[u] + kv[v]];
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = COL ? attn_tbias_keep_bits<H, SB>(l, (unsigned)my_src, (unsigned)cur_row, dr)
                             : attn_tbias_keep_bits<H, SB>(l, (unsigned)cur_row, (unsigned)my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = group_bcast<L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float s = group_sum<DQ>(dot4(y0[v], x0[u][v])) + bb[u][v];
          float da = group_sum<DQ>(dot4(y1[v], x1[u][v]));
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
            attn_rows_fma4(acc0[v], ds, x0[u][v]);   // dK += ds Q_i
            attn_rows_fma4(acc1[v], av, x1[u][v]);   // dV += a mult dO_i
          } else {
            // kernel-uniform check: dB is wanted.  The head's first lane adds, real slots only; lane groups may meet in
            // a word of the table
            if (rep != nullptr && u < nb && l % DQ == 0) atomicAdd(tab + tt[u] + kv[v], ds);
            attn_rows_fma4(acc0[v], ds, x0[u][v]);   // dQ += ds K_j
          }
        }
      }
    }
  }
  if (dirty) flush(cur_row);
  if (n_tab) {   // the table has dB's layout
    __syncthreads();
    float* mine = rep + (i64)(blockIdx.x % nrep) * n_tab;
    for (int i = threadIdx.x; i < n_tab; i += kFastBlock) {
      const float g = tab[i];
      if (g != 0.f) atomicAdd(mine + i, g);   // a (type, head) this workgroup met in no slot adds nothing
    }
  }
}

// dB[i] = sum over the replicas of rep[r][i]; every element of dB is written
__global__ void k_attn_tbias_db_reduce(const float* __restrict__ rep, float* __restrict__ dB, int n, int nrep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int r = 0; r < nrep; ++r) acc += rep[(i64)r * n + i];
  dB[i] = acc;
}

// ---- generic kernels: fp32 / fp64, any h and d, any chunk layout, any n_types; one wave per chunk --------------------
// the type of edge id e, clamped: the one place a generic pass reads etype
__device__ __forceinline__ i64 attn_tbias_of(const int* __restrict__ etype, i64 e, unsigned tmax) {
  return (i64)min((unsigned)etype[e], tmax);
}

// s of one (slot, head): q = Q[i, k, :], kj = K[j, k, :], bias = B[t, k].  Every generic pass evaluates it by this
// function, so a recomputed score is bitwise the one the statistics were taken from.
template <typename T>
__device__ __forceinline__ T attn_tbias_score(const T* __restrict__ q, const T* __restrict__ kj, T bias, i64 d) {
  T s = 0;
  for (i64 c = 0; c < d; ++c) s += q[c] * kj[c];
  return s + bias;
}

// stats[i, k] = (-1e9, 0): the floor of the maxima, the start of the sums, and what rows without slots keep
template <typename T>
__global__ void k_attn_tbias_stats_init_generic(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { stats[i * 2] = (T)-1e9; stats[i * 2 + 1] = (T)0; }
}
// the sums become 1 / l
template <typename T>
__global__ void k_attn_tbias_stats_fin_generic(T* __restrict__ stats, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const T s = stats[i * 2 + 1]; stats[i * 2 + 1] = s > (T)0 ? (T)1 / s : (T)0; }
}

// lanes over the chunk's slots, one head at a time; SUM = false: the maxima, true: the sums of exp(s - m)
template <typename T, bool SUM>
__global__ __launch_bounds__(kGenericBlock) void k_attn_tbias_stats_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ B,
    const int* __restrict__ etype, unsigned tmax, T* __restrict__ stats, i64 n_chunks, i64 h, i64 d) {
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
      const i64 t = attn_tbias_of(etype, eid[j], tmax);
      const T s = attn_tbias_score<T>(Q + (r * h + k) * d, K + (indices[j] * h + k) * d, B[t * h + k], d);
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
__global__ __launch_bounds__(kGenericBlock) void k_attn_tbias_fwd_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ B, const int* __restrict__ etype, unsigned tmax, const T* __restrict__ stats,
    T* __restrict__ o, i64 n_chunks, i64 h, i64 d, i64 head0, DropArgsIf<DROP, T> dr) {
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
      const i64 src = indices[j], t = attn_tbias_of(etype, eid[j], tmax);
      const T s = attn_tbias_score<T>(Q + (r * h + k) * d, K + (src * h + k) * d, B[t * h + k], d);
      T w = exp_t(s - m) * il;
      if constexpr (DROP) w *= drop_mult<T>(r, src, head0 + k, dr);
      acc += w * V[src * f + it];
    }
    atomicAdd(o + r * f + it, acc);
  }
}

// P[i, k] = (m, 1 / l, D = <dO_ik, o_ik>, 0)
template <typename T>
__global__ void k_attn_tbias_pack_generic(const T* __restrict__ stats, const T* __restrict__ dO, const T* __restrict__ o,
                                          T* __restrict__ P, i64 n, i64 d) {   // n = n_q * h
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T dsum = 0;
  for (i64 c = 0; c < d; ++c) dsum += dO[i * d + c] * o[i * d + c];
  P[i * 4] = stats[i * 2]; P[i * 4 + 1] = stats[i * 2 + 1]; P[i * 4 + 2] = dsum; P[i * 4 + 3] = 0;
}

// ds of one (slot, head): p = P[i, k] holds (m, 1 / l, D); *a_out = a_e; mult = the slot's dropout multiplier
template <typename T>
__device__ __forceinline__ T attn_tbias_ds(const T* __restrict__ q, const T* __restrict__ kj, const T* __restrict__ vj,
                                           T bias, const T* __restrict__ p, const T* __restrict__ dO_ik, i64 d, T mult,
                                           T* a_out) {
  const T s = attn_tbias_score<T>(q, kj, bias, d);
  const T a = exp_t(s - p[0]) * p[1];
  T da = 0;
  for (i64 t = 0; t < d; ++t) da += dO_ik[t] * vj[t];
  *a_out = a;
  return a * (mult * da - p[2]);
}

// dB (may be NULL; zero-filled by the caller) is added into with global atomics by the lane that holds a head's first
// element, one per (run of slots of one type, head): a lane sums what consecutive slots of one type give before it adds.
// The slow path, not tuned.
template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_tbias_bwd_row_generic(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ B, const int* __restrict__ etype, unsigned tmax, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dQ, T* __restrict__ dB, i64 n_chunks, i64 h, i64 d, i64 head0,
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
    const bool adds = dB != nullptr && it == k * d;   // the head's first element
    T acc = 0, aij, run = 0;
    i64 t_run = attn_tbias_of(etype, eid[j0], tmax);
    for (i64 j = j0; j < j1; ++j) {
      const i64 src = indices[j], t = attn_tbias_of(etype, eid[j], tmax);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(r, src, head0 + k, dr);
      const T ds = attn_tbias_ds<T>(Q + (r * h + k) * d, K + (src * h + k) * d, V + (src * h + k) * d, B[t * h + k],
                                    P + (r * h + k) * 4, dO + (r * h + k) * d, d, mult, &aij);
      acc += ds * K[src * f + it];
      if (adds) {
        if (t != t_run) { atomicAdd(dB + t_run * h + k, run); run = 0; t_run = t; }
        run += ds;
      }
    }
    atomicAdd(dQ + r * f + it, acc);
    if (adds) atomicAdd(dB + t_run * h + k, run);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(kGenericBlock) void k_attn_tbias_bwd_col_generic(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V,
    const T* __restrict__ B, const int* __restrict__ etype, unsigned tmax, const T* __restrict__ P,
    const T* __restrict__ dO, T* __restrict__ dK, T* __restrict__ dV, i64 n_chunks, i64 h, i64 d, i64 head0,
    DropArgsIf<DROP, T> dr) {
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
      const i64 i = indices[j], t = attn_tbias_of(etype, eid[j], tmax);
      T mult = 1;
      if constexpr (DROP) mult = drop_mult<T>(i, jc, head0 + k, dr);
      const T ds = attn_tbias_ds<T>(Q + (i * h + k) * d, K + (jc * h + k) * d, V + (jc * h + k) * d, B[t * h + k],
                                    P + (i * h + k) * 4, dO + (i * h + k) * d, d, mult, &aij);
      acc_k += ds * Q[i * f + it];
      acc_v += aij * mult * dO[i * f + it];
    }
    atomicAdd(dK + jc * f + it, acc_k);
    atomicAdd(dV + jc * f + it, acc_v);
  }
}

}  // namespace graphop
