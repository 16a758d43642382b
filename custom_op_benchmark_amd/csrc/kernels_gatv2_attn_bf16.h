// The fused GATv2 attention layer on bfloat16 tables (gatv2_attention_bf16.hip has the host side): xl, xr,
// att, o, dO, dxl, dxr, datt are bf16, stats (n_src, H, 2) = (m, 1 / l) stay fp32, every sum is fp32 and every bf16 result
// is rounded once, to nearest even.  The formulas are those of kernels_gatv2_attn.h (and kernels_dropout.h for the keep
// decision): z_c = float(xl[i, k, c]) + float(xr[j, k, c]), one fp32 add of exactly widened values, LeakyReLU in fp32 as
// max(z, 0) + slope * min(z, 0), s = sum_c float(att[k, c]) LeakyReLU(z_c).
//
// Layout, accumulators, the dot chain and the record scheme are kernels_attn_bf16.h's: a row of F = H * D elements is
// F8 = F / 8 pieces of 16 B, a lane group of L = min(16, F8) lanes holds NV = F8 / L of them, piece p = v * L + l, a head
// is DQ = D / 8 adjacent lanes.  The lane's share of a score is gatv2_bf16_score: ONE expression, the piece's element 0
// first, used by the forward and by both backward passes, then group_sum<DQ>; a recomputed s is bitwise the forward's
// (the add of z commutes, so the column pass, whose own row is xr, forms the same z).  Gathered rows stay packed until
// they are consumed: two elements per word by a shift and a mask.  att is widened once per lane and kept as fp32.
//
// Slots per batch (Gatv2Bf16Cfg) follow from the register counts of the gfx950 code objects.  The forward gathers one row
// per slot: 8 / NV slots = 8 pieces = 32 registers in flight beside att, the fp32 accumulator row and the packed own row:
// 119 - 164 VGPRs.  The row pass keeps att, the sums, the datt partials (8 NV floats each), two packed own rows and P, and
// the compiler keeps a batch's z_c alive from the score to the sums across the group_sum: at 8 / NV slots it needs 238 -
// 299 registers (AGPR copies from 256 on), at 4 / NV 162 - 219, so 4 / NV it is.  The column pass gathers xl_i, dO_i and
// the 16-byte P item per piece: 4 / NV slots = 48 registers in flight, 132 - 174 VGPRs.  SB <= L in every pass: lane l
// holds the id of slot l % SB and runs that slot's Philox call, the keep bits travel round the group like the id
// (GatBf16DropCfg).  Arithmetic is scalar fp32 (the object is built without packed fp32 operations, like the other bf16
// ones).
//
// Matrix instructions do not fit: LeakyReLU stands between the add and the contraction with att, so the score is no
// product of two tables, and a weight pairs one own row with one gathered row, so there is no second dimension of rows to
// tile over; da of the backward is a v_dot2c_f32_bf16 chain and a group_sum<DQ>.
//
// No float atomic on any output.  The forward is a segment driver: one lane group per row segment of a row_owned plan
// (segments above kLongSegment slots: one workgroup each, its groups merging (m, l, acc) through LDS in group order), an
// online softmax in fp32, a row is never split, o_i = acc / l rounded once; no records.  The backward passes are chunk
// drivers: a lane group takes chunks_per_group consecutive chunks; rows wholly inside its run it rounds and stores; the at
// most two rows it shares with its neighbours leave as fp32 records of F floats in slot 2 * group + {0, 1} (row word with
// first / last flags, kBf16RecNone = no record) that a merge kernel sums in record order, rounds and stores once.
// Passes:
//   fwd     : xl_i packed, att, the fp32 accumulator row and (m, l) per head in registers; gathers xr_j
//   pack    : P[i, k] = (m, 1 / l, D, 0) fp32, D = <dO_i, o_i> from the bf16 o as given
//   bwd_row : xl_i, dO_i packed and P[i] in registers; gathers xr_j -> dxl = att * sum_j ds t (multiplied when the row
//             leaves) and the workgroup's row of fp32 datt partials, kept in registers over the group's run
//   bwd_col : xr_j packed and att in registers; gathers xl_i, dO_i and P[i] -> dxr
//   merge   : the records of either backward pass -> dxl / dxr
//   datt_fin: the row pass's partial rows summed in a fixed order and rounded once
// da = group_sum<DQ>(attn_bf16_dot(dO piece, xr piece)) with the dO-side word first in both backward passes, so the two
// agree on every ds bit for bit.
#pragma once
#include "kernels_attn_bf16.h"
#include "kernels_bf16_drop.h"
#include "kernels_dropout.h"

namespace graphop {

constexpr float kGatv2Bf16Floor = -1e9f;   // the library's softmax floor (m = max(-1e9, max_j s_ij))

template <int H, int D>
struct Gatv2Bf16Cfg : AttnBf16Cfg<H, D> {
  using B = AttnBf16Cfg<H, D>;
  static constexpr int SB_FWD = 8 / B::NV;   // one gathered row per slot
  static constexpr int SB_ROW = 4 / B::NV;
  static constexpr int SB_COL = 4 / B::NV;   // two gathered rows and a P item per slot
  static_assert(SB_FWD <= B::L && SB_COL >= 1, "a lane holds at most one slot id");
};

__device__ __forceinline__ Bf16Acc gatv2_bf16_unpack(const uint4& x) {
  return Bf16Acc{{bf16_lo(x.x), bf16_hi(x.x), bf16_lo(x.y), bf16_hi(x.y), bf16_lo(x.z), bf16_hi(x.z), bf16_lo(x.w),
                  bf16_hi(x.w)}};
}

// max(z, 0) + s * min(z, 0): one of the two terms is 0, so the fused form rounds as the unfused one; z == 0 takes the slope
__device__ __forceinline__ float gatv2_bf16_lrelu(float z, float s) { return fmaf(s, fminf(z, 0.f), fmaxf(z, 0.f)); }

// The lane's share of a score over one piece: sum_e w_e LeakyReLU(xl_e + xr_e), element 0 first.  The one text every
// pass evaluates a score by.
__device__ __forceinline__ float gatv2_bf16_score(const Bf16Acc& w, const uint4& xl, const uint4& xr, float slope) {
  const Bf16Acc a = gatv2_bf16_unpack(xl), b = gatv2_bf16_unpack(xr);
  float s = w.a[0] * gatv2_bf16_lrelu(a.a[0] + b.a[0], slope);
#pragma unroll
  for (int e = 1; e < 8; ++e) s = fmaf(w.a[e], gatv2_bf16_lrelu(a.a[e] + b.a[e], slope), s);
  return s;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
struct Gatv2Bf16FwdArgs {
  const uint4* xl;      // [n_l][F8]  own rows
  const uint4* xr;      // [n_r][F8]  gathered
  const uint4* att;     // [F8]
  uint4* o;             // [n_l][F8]  zero-filled by the caller: rows without segments are not written
  float2* stats;        // [n_l][H]   (-1e9, 0)-filled by the caller likewise
};

// Blocks [0, nb_short): lane groups of L, one row segment each (segments above long_len slots are skipped); block
// nb_short + b: the whole workgroup on segment long_segs[b], its groups taking batches strided and merging through LDS.
// Per batch the running maximum is raised once and (l, acc) rescaled once.  DROP: l sums the undropped exp(s - m), acc
// the terms exp(s - m) m_ijk xr_j, so stats come from the same expressions in the same order as without dropout.
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_gv2bf16_fwd(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const i64* __restrict__ seg_chunk, Gatv2Bf16FwdArgs a, i64 n_seg, unsigned nb_short, i64 long_len,
    const int* __restrict__ long_segs, float slope, DropArgsIf<DROP, float> dr) {
  using C = Gatv2Bf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_FWD, F8 = C::F8;
  constexpr int NG = kFastBlock / L;   // lane groups of a workgroup
  // Static LDS of EVERY workgroup although only the long-segment ones use it: 17 KB at h * d = 256, nine workgroups a CU,
  // while the kernel's 119 - 164 VGPRs allow three or four.  A register cut below 56 would run into it.
  __shared__ Bf16Acc red_acc[NG][F8];
  __shared__ float2 red_ml[NG][H];
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const bool longp = blockIdx.x >= nb_short;   // workgroup-uniform
  const i64 s = longp ? (i64)long_segs[blockIdx.x - nb_short] : (i64)blockIdx.x * NG + g;
  const bool have = s < n_seg;
  i64 r = 0, j0 = 0, j1 = 0;
  if (have) {
    const i64 c0 = seg_chunk[s];
    r = row[c0];
    j0 = indptr[c0];
    j1 = indptr[seg_chunk[s + 1]];
  }
  const bool work = have && (longp || j1 - j0 <= long_len);   // group-uniform
  int kv[NV];
  uint4 q[NV];
  Bf16Acc w[NV], acc[NV];
  float m[NV], ls[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = attn_bf16_head<H, D>(v, l);
    attn_bf16_zero(acc[v]);
    m[v] = kGatv2Bf16Floor;
    ls[v] = 0.f;
  }
  if (work) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      w[v] = gatv2_bf16_unpack(a.att[v * L + l]);
      q[v] = a.xl[r * F8 + v * L + l];
    }
    const i64 step = longp ? (i64)NG * SB : (i64)SB;
    for (i64 jb = longp ? j0 + (i64)g * SB : j0; jb < j1; jb += step) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot with weight 0
      const int t = l % SB;
      const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      uint4 x[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* xp = a.xr + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) x[u][v] = xp[v * L];
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
      for (int v = 0; v < NV; ++v) {
        float sc[SB];
        float mn = m[v];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          sc[u] = group_sum<DQ>(gatv2_bf16_score(w[v], q[v], x[u][v], slope));
          mn = u < nb ? fmaxf(mn, sc[u]) : mn;
        }
        const float f = exp_nonpos(m[v] - mn);
        m[v] = mn;
        ls[v] *= f;
        attn_bf16_scale(acc[v], f);
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const float p = u < nb ? exp_nonpos(sc[u] - mn) : 0.f;
          ls[v] += p;
          if constexpr (DROP) attn_bf16_fma(acc[v], (keep[u] >> kv[v]) & 1 ? p * dr.scale : 0.f, x[u][v]);
          else attn_bf16_fma(acc[v], p, x[u][v]);
        }
      }
    }
  }
  if (!longp) {
    if (work) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float il = ls[v] > 0.f ? 1.f / ls[v] : 0.f;
        attn_bf16_scale(acc[v], il);
        a.o[r * F8 + v * L + l] = attn_bf16_round(acc[v]);
        if (l % DQ == 0) a.stats[r * H + kv[v]] = make_float2(m[v], il);
      }
    }
    return;
  }
  // long segment (workgroup-uniform branch): every group publishes (m, l) per head and acc per piece (16 KB + 1 KB of
  // LDS at h * d = 256); thread p < F8 merges piece p over the groups in group order
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    red_acc[g][v * L + l] = acc[v];
    if (l % DQ == 0) red_ml[g][kv[v]] = make_float2(m[v], ls[v]);
  }
  __syncthreads();
  if (have && threadIdx.x < F8) {
    const int p = threadIdx.x, k = p / DQ;
    float mm = kGatv2Bf16Floor;
#pragma unroll
    for (int q2 = 0; q2 < NG; ++q2) mm = fmaxf(mm, red_ml[q2][k].x);
    float lsum = 0.f;
    Bf16Acc t;
    attn_bf16_zero(t);
    for (int q2 = 0; q2 < NG; ++q2) {
      const float2 ml = red_ml[q2][k];
      const float f = exp_nonpos(ml.x - mm);
      lsum = fmaf(ml.y, f, lsum);
      const Bf16Acc x = red_acc[q2][p];
#pragma unroll
      for (int e = 0; e < 8; ++e) t.a[e] = fmaf(f, x.a[e], t.a[e]);
    }
    const float il = lsum > 0.f ? 1.f / lsum : 0.f;
    attn_bf16_scale(t, il);
    a.o[r * F8 + p] = attn_bf16_round(t);
    if (p % DQ == 0) a.stats[r * H + k] = make_float2(mm, il);
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// P[i, k] = (m, 1 / l, <dO_ik, o_ik>, 0): the dO-side word first, fp32 sums
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gv2bf16_pack(
    const float2* __restrict__ stats, const uint4* __restrict__ dO, const uint4* __restrict__ o, float4* __restrict__ P,
    i64 n) {
  using C = Gatv2Bf16Cfg<H, D>;
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
      P[k] = make_float4(st.x, st.y, dsum, 0.f);
    }
  }
}

// the records of a backward pass: row words and one row of F floats per record
struct Gatv2Bf16Rec {
  unsigned* p_row;      // [2 * groups], kBf16RecNone-filled
  float* p_acc;         // [2 * groups][F]
};

// a finished row leaves the group: rounded and stored where the group owns it, else as a record
template <int L, int NV>
__device__ __forceinline__ void gatv2_bf16_flush(const Bf16Acc (&acc)[NV], uint4* __restrict__ out, const Gatv2Bf16Rec& rec,
                                                 i64 gid, i64 r, i64 row_before, i64 row_after, int l) {
  constexpr i64 F8 = (i64)L * NV;
  if (r != row_before && r != row_after) {
#pragma unroll
    for (int v = 0; v < NV; ++v) out[r * F8 + v * L + l] = attn_bf16_round(acc[v]);
  } else {
    const i64 pi = attn_bf16_rec_slot(gid, r, row_before);
#pragma unroll
    for (int v = 0; v < NV; ++v) attn_bf16_rec_store(rec.p_acc, pi * F8 + v * L + l, acc[v]);
    if (l == 0) rec.p_row[pi] = attn_bf16_rec_word(r, row_before, row_after);
  }
}

// row pass: own = xl_i, dO_i (packed), P[i]; gathered = xr_j.  The row sum is kept as sum_j ds t and multiplied by att when
// the row leaves.  The lane's pieces of datt are summed over the group's whole run, reduced over the workgroup (shuffles
// inside a wave, LDS across waves, both in a fixed order) and written as row blockIdx.x of datt_part (gridDim.x, F):
// every workgroup writes its row, groups without chunks add zeros.  dxl is zero-filled by the caller: rows without chunks
// are not written.  DROP: da_ij = m_ij <dO_i, xr_j>; D_i in P is <dO_i, o_i> of the dropped o.
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_gv2bf16_bwd_row(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const uint4* __restrict__ xl, const uint4* __restrict__ xr, const uint4* __restrict__ att,
    const float4* __restrict__ P, const uint4* __restrict__ dO, uint4* __restrict__ dxl, Gatv2Bf16Rec rec,
    float* __restrict__ datt_part, i64 n_chunks, int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  using C = Gatv2Bf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_ROW, F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  int kv[NV];
  Bf16Acc w[NV], acc[NV], dw[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = attn_bf16_head<H, D>(v, l);
    w[v] = gatv2_bf16_unpack(att[v * L + l]);
    attn_bf16_zero(dw[v]);
  }
  if (c0 < c1) {   // group-uniform
    const i64 row_before = c0 > 0 ? row[c0 - 1] : -1;
    const i64 row_after = c1 < n_chunks ? row[c1] : -1;
    uint4 a[NV], g[NV];   // xl_i, dO_i
    float pm[NV], pil[NV], pd[NV];
    auto flush = [&](i64 r) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[v].a[e] *= w[v].a[e];
      }
      gatv2_bf16_flush<L, NV>(acc, dxl, rec, gid, r, row_before, row_after, l);
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
          a[v] = xl[r * F8 + v * L + l];
          g[v] = dO[r * F8 + v * L + l];
          const float4 p = P[r * H + kv[v]];
          pm[v] = p.x; pil[v] = p.y; pd[v] = p.z;
        }
      }
      const i64 j0 = indptr[c], j1 = indptr[c + 1];
      for (i64 jb = j0; jb < j1; jb += SB) {
        const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
        // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot with weight 0
        const int t = l % SB;
        const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
        uint4 x[SB][NV];
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const i64 src = group_bcast<L, u>(my_src);
          const uint4* xp = xr + src * F8 + l;
#pragma unroll
          for (int v = 0; v < NV; ++v) x[u][v] = xp[v * L];
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
            const float s = group_sum<DQ>(gatv2_bf16_score(w[v], a[v], x[u][v], slope));
            float da = group_sum<DQ>(attn_bf16_dot(g[v], x[u][v]));   // the dO-side words first in both passes
            if constexpr (DROP) da *= (keep[u] >> kv[v]) & 1 ? dr.scale : 0.f;
            const float aij = u < nb ? exp_nonpos(s - pm[v]) * pil[v] : 0.f;
            const float ds = aij * (da - pd[v]), dss = ds * slope;
            const Bf16Acc ya = gatv2_bf16_unpack(a[v]), yx = gatv2_bf16_unpack(x[u][v]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float z = ya.a[e] + yx.a[e];
              acc[v].a[e] += z > 0.f ? ds : dss;
              dw[v].a[e] = fmaf(ds, gatv2_bf16_lrelu(z, slope), dw[v].a[e]);
            }
          }
        }
      }
    }
    if (cur >= 0) flush(cur);
  }
  // every thread of the workgroup arrives here
  static_assert(F8 <= kWave, "one thread per piece in the last step");
  __shared__ Bf16Acc red[kFastBlock / kWave][F8];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    Bf16Acc t = dw[v];
#pragma unroll
    for (int o = L; o < kWave; o <<= 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) t.a[e] += __shfl_xor(t.a[e], o);
    }
    if (lane < L) red[wv][v * L + lane] = t;
  }
  __syncthreads();
  if (threadIdx.x < F8) {
    Bf16Acc t = red[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < kFastBlock / kWave; ++q) attn_bf16_add(t, red[q][threadIdx.x]);
    attn_bf16_rec_store(datt_part, (i64)blockIdx.x * F8 + threadIdx.x, t);
  }
}

// column pass: own = xr_j (packed); gathered = xl_i, dO_i and P[i]; dxr[j] = sum_i (ds att t + a dO_i), one fp32 register
// row per column.  dxr is zero-filled by the caller.  DROP: the decision's counter stays (i, j) = (gathered id, own
// column); da_ij = m_ij <dO_i, xr_j> and the second term is a_ij m_ij dO_i.
template <int H, int D, bool DROP>
__global__ __launch_bounds__(kFastBlock) void k_gv2bf16_bwd_col(
    const i64* __restrict__ col, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const uint4* __restrict__ xl, const uint4* __restrict__ xr, const uint4* __restrict__ att,
    const float4* __restrict__ P, const uint4* __restrict__ dO, uint4* __restrict__ dxr, Gatv2Bf16Rec rec, i64 n_chunks,
    int chunks_per_group, float slope, DropArgsIf<DROP, float> dr) {
  using C = Gatv2Bf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ, SB = C::SB_COL, F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 gid = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  const i64 c0 = gid * chunks_per_group;
  i64 c1 = c0 + chunks_per_group;
  if (c1 > n_chunks) c1 = n_chunks;
  if (c0 >= c1) return;
  const i64 col_before = c0 > 0 ? col[c0 - 1] : -1;
  const i64 col_after = c1 < n_chunks ? col[c1] : -1;
  int kv[NV];
  uint4 b[NV];   // xr_j
  Bf16Acc w[NV], acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = attn_bf16_head<H, D>(v, l);
    w[v] = gatv2_bf16_unpack(att[v * L + l]);
  }
  i64 cur = -1;
  for (i64 c = c0; c < c1; ++c) {
    const i64 r = col[c];
    if (r != cur) {
      if (cur >= 0) gatv2_bf16_flush<L, NV>(acc, dxr, rec, gid, cur, col_before, col_after, l);
      cur = r;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        attn_bf16_zero(acc[v]);
        b[v] = xr[r * F8 + v * L + l];
      }
    }
    const i64 j0 = indptr[c], j1 = indptr[c + 1];
    for (i64 jb = j0; jb < j1; jb += SB) {
      const int nb = (j1 - jb) < SB ? (int)(j1 - jb) : SB;
      // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot with weight 0
      const int t = l % SB;
      const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      uint4 x[SB][NV], y[SB][NV];   // xl_i, dO_i
      float4 p[SB][NV];             // P[i, k_v]
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          x[u][v] = xl[src * F8 + v * L + l];
          y[u][v] = dO[src * F8 + v * L + l];
          p[u][v] = P[src * H + kv[v]];
        }
      });
      int keep[DROP ? SB : 1];
      if constexpr (DROP) {
        const int mine = gat_bf16_lane_bits<H, SB, L, true>(l, r, my_src, dr);
        static_for<SB>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          keep[u] = gat_bf16_slot_bits<H, SB, L, u>(mine);
        });
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float s = group_sum<DQ>(gatv2_bf16_score(w[v], x[u][v], b[v], slope));
          float da = group_sum<DQ>(attn_bf16_dot(y[u][v], b[v]));   // the dO-side words first in both passes
          const float aij = u < nb ? exp_nonpos(s - p[u][v].x) * p[u][v].y : 0.f;
          float am = aij;   // a_ij m_ij
          if constexpr (DROP) {
            const float mk = (keep[u] >> kv[v]) & 1 ? dr.scale : 0.f;
            da *= mk;
            am *= mk;
          }
          const float ds = aij * (da - p[u][v].z), dss = ds * slope;
          const Bf16Acc yx = gatv2_bf16_unpack(x[u][v]), yb = gatv2_bf16_unpack(b[v]), yg = gatv2_bf16_unpack(y[u][v]);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float z = yx.a[e] + yb.a[e];
            acc[v].a[e] = fmaf(z > 0.f ? ds : dss, w[v].a[e], fmaf(am, yg.a[e], acc[v].a[e]));
          }
        }
      }
    }
  }
  if (cur >= 0) gatv2_bf16_flush<L, NV>(acc, dxr, rec, gid, cur, col_before, col_after, l);
}

// One lane group per first record: plain sums over the row's records in record order, then the row once (dxl or dxr).
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_gv2bf16_bwd_merge(Gatv2Bf16Rec rec, uint4* __restrict__ out,
                                                                          i64 n) {
  using C = Gatv2Bf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  unsigned w = rec.p_row[i];
  if (w == kBf16RecNone || !(w & kBf16RecFirst)) return;
  const unsigned r = w & kBf16RecRow;
  Bf16Acc acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) attn_bf16_zero(acc[v]);
  for (i64 j = i; j >= 0; j = attn_bf16_rec_next(rec.p_row, j, n, r, w)) {
#pragma unroll
    for (int v = 0; v < NV; ++v) attn_bf16_add(acc[v], attn_bf16_rec_load(rec.p_acc, j * F8 + v * L + l));
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) out[(i64)r * F8 + v * L + l] = attn_bf16_round(acc[v]);
}

// k_gv2bf16_stats_init and k_gv2bf16_datt_fin are no templates: they are defined in gatv2_attention_bf16.hip alone.

}  // namespace graphop
