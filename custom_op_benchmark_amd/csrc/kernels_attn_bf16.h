// The fused dot-product attention step on bfloat16 rows (attention_bf16.hip has the host side): Q, K, V,
// o, dO, dQ, dK, dV are bf16 [n][H][D], everything summed is fp32, stats (n_q, H, 2) = (m, 1 / l) stay fp32.
//
// Layout (AttnBf16Cfg<H, D>): a piece is 16 B = 8 bf16 in four packed words (element 2 w in the low half of word w).  A
// row of F = H * D elements is F8 = F / 8 pieces; a lane group of L = min(16, F8) lanes holds NV = F8 / L of them, piece
// p = v * L + l, so a head is DQ = D / 8 adjacent lanes and a head's score is a group_sum<DQ> (DQ = 1 at D = 8: no
// cross-lane step).  Slots per batch keep AttnRowsCfg's budget, 16 pieces of 16 B in flight per lane at two rows per slot:
// SB = 8 / NV, and the same registers cover twice the elements.
//
// Arithmetic: Q (the own rows of the backward) stays packed; a score is a chain of v_dot2c_f32_bf16 over the four words
// of the own and the gathered piece, always with the Q-side word first, then group_sum<DQ>.  Forward and both backward
// passes reduce a score by that chain over the same words, so the backward's s is the forward's bit for bit.  V, dO and
// whatever else is multiplied by a weight is unpacked by a shift and a mask where it is consumed.  Results are rounded
// once, to nearest even, by v_cvt_pk_bf16_f32.
//
// No float atomic on any output.  A lane group takes chunks_per_group consecutive chunks of a row_owned plan; the rows
// that lie wholly inside its run it rounds and stores itself.  The at most two rows it shares with its neighbours leave
// as fp32 RECORDS in the workspace, slot 2 * group + {0: shared with the group before, 1: with the group after}: a row
// word (row | kBf16RecFirst on the row's first record | kBf16RecLast on its last; kBf16RecNone = the fill: no record),
// and the group's partial result.  Sorted rows make one row's records a run of record slots, so a merge kernel gives one
// lane group to every record that carries the first flag; it walks forward to the last flag, skipping empty slots,
// combines in registers in record order, rounds and stores the row once.  Every sum therefore has one fixed order: the
// op is bitwise reproducible from run to run.
#pragma once
#include "kernels_attn_rows.h"

namespace graphop {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

constexpr unsigned kBf16RecFirst = 1u << 31, kBf16RecLast = 1u << 30, kBf16RecNone = ~0u;   // (first & last: never a record)
constexpr unsigned kBf16RecRow = kBf16RecLast - 1;

template <int H, int D>
struct AttnBf16Cfg {
  static constexpr int F8 = H * D / 8;            // pieces of a row
  static constexpr int L = F8 < 16 ? F8 : 16;     // lanes per group (8 or 16)
  static constexpr int NV = F8 / L;               // pieces per lane (1, 2, 4)
  static constexpr int DQ = D / 8;                // lanes holding one head's pieces (1 .. 16)
  static constexpr int SB = 8 / NV;               // slots per batch
  static_assert(D % 8 == 0 && NV * L == F8 && DQ <= L && L % DQ == 0 && NV <= 4, "unsupported (H, D)");
};

// head of lane l's piece v
template <int H, int D>
__device__ __forceinline__ int attn_bf16_head(int v, int l) {
  using C = AttnBf16Cfg<H, D>;
  return (v * C::L + l) / C::DQ;
}

// the lane's share of a dot product of two pieces: qside's words first (one order everywhere, see above)
__device__ __forceinline__ float attn_bf16_dot(const uint4& qside, const uint4& kside) {
  float s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.x), __builtin_bit_cast(bf16x2_t, kside.x), 0.f, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.y), __builtin_bit_cast(bf16x2_t, kside.y), s, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.z), __builtin_bit_cast(bf16x2_t, kside.z), s, false);
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, qside.w), __builtin_bit_cast(bf16x2_t, kside.w), s, false);
}

// eight fp32 accumulators of one piece: element e of the piece is a[e]
struct Bf16Acc {
  float a[8];
};
__device__ __forceinline__ void attn_bf16_zero(Bf16Acc& c) {
#pragma unroll
  for (int e = 0; e < 8; ++e) c.a[e] = 0.f;
}
__device__ __forceinline__ void attn_bf16_scale(Bf16Acc& c, float f) {
#pragma unroll
  for (int e = 0; e < 8; ++e) c.a[e] *= f;
}
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
// c += w * x, x unpacked here
__device__ __forceinline__ void attn_bf16_fma(Bf16Acc& c, float w, const uint4& x) {
  c.a[0] = fmaf(w, bf16_lo(x.x), c.a[0]); c.a[1] = fmaf(w, bf16_hi(x.x), c.a[1]);
  c.a[2] = fmaf(w, bf16_lo(x.y), c.a[2]); c.a[3] = fmaf(w, bf16_hi(x.y), c.a[3]);
  c.a[4] = fmaf(w, bf16_lo(x.z), c.a[4]); c.a[5] = fmaf(w, bf16_hi(x.z), c.a[5]);
  c.a[6] = fmaf(w, bf16_lo(x.w), c.a[6]); c.a[7] = fmaf(w, bf16_hi(x.w), c.a[7]);
}
__device__ __forceinline__ void attn_bf16_add(Bf16Acc& c, const Bf16Acc& x) {
#pragma unroll
  for (int e = 0; e < 8; ++e) c.a[e] += x.a[e];
}
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) {   // round to nearest even
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ uint4 attn_bf16_round(const Bf16Acc& c) {
  return make_uint4(bf16_pack2(c.a[0], c.a[1]), bf16_pack2(c.a[2], c.a[3]), bf16_pack2(c.a[4], c.a[5]), bf16_pack2(c.a[6], c.a[7]));
}
// a record's fp32 copy of one piece: two float4 at piece index i of a float table
__device__ __forceinline__ void attn_bf16_rec_store(float* __restrict__ tab, i64 i, const Bf16Acc& c) {
  float4* p = reinterpret_cast<float4*>(tab) + i * 2;
  p[0] = make_float4(c.a[0], c.a[1], c.a[2], c.a[3]);
  p[1] = make_float4(c.a[4], c.a[5], c.a[6], c.a[7]);
}
__device__ __forceinline__ Bf16Acc attn_bf16_rec_load(const float* __restrict__ tab, i64 i) {
  const float4* p = reinterpret_cast<const float4*>(tab) + i * 2;
  const float4 x = p[0], y = p[1];
  return Bf16Acc{{x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w}};
}
// the row word of group `gid`'s record of row r, and its slot
__device__ __forceinline__ i64 attn_bf16_rec_slot(i64 gid, i64 r, i64 row_before) { return gid * 2 + (r == row_before ? 0 : 1); }
__device__ __forceinline__ unsigned attn_bf16_rec_word(i64 r, i64 row_before, i64 row_after) {
  return (unsigned)r | (r != row_before ? kBf16RecFirst : 0u) | (r != row_after ? kBf16RecLast : 0u);
}
// The next record of `row` behind slot j (empty slots skipped), or -1 when the record at j was the row's last.  `w` is
// the word at j on entry and the word of the returned slot on exit.
__device__ __forceinline__ i64 attn_bf16_rec_next(const unsigned* __restrict__ p_row, i64 j, i64 n, unsigned row, unsigned& w) {
  if (w & kBf16RecLast) return -1;
  for (++j; j < n; ++j) {
    w = p_row[j];
    if (w == kBf16RecNone) continue;
    return (w & kBf16RecRow) == row ? j : -1;
  }
  return -1;
}

// the final (m, 1 / l) of a row's head from its running (m, l): the library's floor on m, 0 for a row without slots
__device__ __forceinline__ float2 attn_bf16_stats(float m, float l, float& scale_o) {
  const float mf = fmaxf(m, -1e9f);
  const float e = attn_rows_exp(m - mf);
  const float lsum = l * e;
  const float linv = lsum > 0.f ? 1.f / lsum : 0.f;
  scale_o = e * linv;
  return make_float2(mf, linv);
}

// ---- forward --------------------------------------------------------------------------------------------------------
struct AttnBf16FwdArgs {
  const uint4* Q;       // [n_q][F8]  own rows
  const uint4* K;       // [n_k][F8]  gathered
  const uint4* V;       // [n_k][F8]  gathered
  uint4* o;             // [n_q][F8]  zero-filled by the caller: rows without slots are not written
  float* stats;         // [n_q][H][2] fp32, zero-filled by the caller likewise
  unsigned* p_row;      // [2 * groups]  row words, kBf16RecNone-filled
  float* p_ml;          // [2 * groups][H][2]
  float* p_o;           // [2 * groups][F]
};

// Online softmax batch by batch as in the fp32 several-head pass: the heads' maxima over the batch first, one rescale of
// (l, o) per batch, then one exp2 per slot.
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_bf16_fwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices, AttnBf16FwdArgs a,
    i64 n_chunks, int chunks_per_group) {
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
  float m_c[NV], l_c[NV];   // of the piece's head
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
      // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot and are not folded in
      const int t = l % SB;
      const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
      uint4 x0[SB][NV], x1[SB][NV];
      static_for<SB>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        const i64 src = group_bcast<L, u>(my_src);
        const uint4* kp = a.K + src * F8 + l;
        const uint4* vp = a.V + src * F8 + l;
#pragma unroll
        for (int v = 0; v < NV; ++v) { x0[u][v] = kp[v * L]; x1[u][v] = vp[v * L]; }
      });
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        float s[SB];
        float mx = m_c[v];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          s[u] = group_sum<DQ>(attn_bf16_dot(q[v], x0[u][v]));
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
            attn_bf16_fma(o_c[v], p, x1[u][v]);
          }
        }
      }
    }
  }
  if (cur_row >= 0) finish(cur_row);
}

// One lane group per first record: the online softmax over the row's records in record order, then o and stats once.
template <int H, int D>
__global__ __launch_bounds__(kFastBlock) void k_attn_bf16_fwd_merge(AttnBf16FwdArgs a, i64 n) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  unsigned w = a.p_row[i];
  if (w == kBf16RecNone || !(w & kBf16RecFirst)) return;
  const unsigned r = w & kBf16RecRow;
  Bf16Acc o_c[NV];
  float m_c[NV], l_c[NV];
  int kv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    kv[v] = attn_bf16_head<H, D>(v, l);
    attn_bf16_zero(o_c[v]);
    m_c[v] = kAttnNegBig;
    l_c[v] = 0.f;
  }
  for (i64 j = i; j >= 0; j = attn_bf16_rec_next(a.p_row, j, n, r, w)) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float2 ml = reinterpret_cast<const float2*>(a.p_ml)[j * H + kv[v]];
      const float mx = fmaxf(m_c[v], ml.x);
      const float sc = attn_rows_exp(m_c[v] - mx), sp = attn_rows_exp(ml.x - mx);
      l_c[v] = fmaf(ml.y, sp, l_c[v] * sc);
      attn_bf16_scale(o_c[v], sc);
      const Bf16Acc x = attn_bf16_rec_load(a.p_o, j * F8 + v * L + l);
#pragma unroll
      for (int e = 0; e < 8; ++e) o_c[v].a[e] = fmaf(sp, x.a[e], o_c[v].a[e]);
      m_c[v] = mx;
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    float f;
    const float2 st = attn_bf16_stats(m_c[v], l_c[v], f);
    attn_bf16_scale(o_c[v], f);
    a.o[(i64)r * F8 + v * L + l] = attn_bf16_round(o_c[v]);
    if (l % DQ == 0 && st.y > 0.f) reinterpret_cast<float2*>(a.stats)[(i64)r * H + kv[v]] = st;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// (A_r | B_r) -> out[r][2 F8]: one contiguous request per gathered slot; with STATS also st4[r, k] = (m, 1 / l, <B_rk,
// O_rk>, 0) per head in fp32, O as given (bf16)
template <int H, int D, bool STATS>
__global__ __launch_bounds__(kFastBlock) void k_attn_bf16_pack(
    const uint4* __restrict__ A, const uint4* __restrict__ B, uint4* __restrict__ out, i64 n, const uint4* __restrict__ O,
    const float* __restrict__ stats2, float4* __restrict__ st4) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, DQ = C::DQ;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 r = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (r >= n) return;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const uint4 x = A[r * F8 + v * L + l];
    const uint4 y = B[r * F8 + v * L + l];
    out[r * 2 * F8 + v * L + l] = x;
    out[r * 2 * F8 + F8 + v * L + l] = y;
    if constexpr (STATS) {
      const float dsum = group_sum<DQ>(attn_bf16_dot(y, O[r * F8 + v * L + l]));
      if (l % DQ == 0) {
        const i64 k = r * H + attn_bf16_head<H, D>(v, l);
        st4[k] = make_float4(stats2[k * 2], stats2[k * 2 + 1], dsum, 0.f);
      }
    }
  }
}

// the records of a backward pass: row words and NOUT accumulator rows of F floats per record
struct AttnBf16BwdRec {
  unsigned* p_row;      // [2 * groups], kBf16RecNone-filled
  float* p_acc;         // [2 * groups][NOUT][F]
};

//   COL = false: OWN = (Q | dO) packed [n_q][2 F8], XT = (K | V) packed, out0 = dQ
//   COL = true : OWN = (K | V) packed [n_k][2 F8], XT = (Q | dO) packed, out0 = dK, out1 = dV
// stats4[i, k] = (m, 1 / l, D, -) per ROW i of the attention matrix and head in both passes.  a = exp(s - m) / l,
// ds = a (da - D).  out0 / out1 are zero-filled by the caller: rows without chunks are not written.
template <int H, int D, bool COL>
__global__ __launch_bounds__(kFastBlock) void k_attn_bf16_bwd_rows(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ indices,
    const uint4* __restrict__ OWN, const uint4* __restrict__ XT, const float4* __restrict__ stats4,
    uint4* __restrict__ out0, uint4* __restrict__ out1, AttnBf16BwdRec rec, i64 n_chunks, int chunks_per_group) {
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
      // lane l holds the id of slot l % SB; slots past the end re-read the batch's last slot with weights 0
      const int t = l % SB;
      const int my_src = (int)indices[jb + (t < nb ? t : nb - 1)];
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
#pragma unroll
      for (int u = 0; u < SB; ++u) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          // the Q-side words first in both passes: the forward's chain
          const float s = group_sum<DQ>(COL ? attn_bf16_dot(x0[u][v], y0[v]) : attn_bf16_dot(y0[v], x0[u][v]));
          const float da = group_sum<DQ>(COL ? attn_bf16_dot(x1[u][v], y1[v]) : attn_bf16_dot(y1[v], x1[u][v]));
          float4 st;
          if constexpr (COL) st = stg[u][v];
          else st = own_st[v];
          const float av = u < nb ? expf(s - st.x) * st.y : 0.f;
          const float ds = av * (da - st.z);
          attn_bf16_fma(acc0[v], ds, x0[u][v]);                       // dQ += ds K_j, or dK += ds Q_i
          if constexpr (COL) attn_bf16_fma(acc1[v], av, x1[u][v]);    // dV += a dO_i
        }
      }
    }
  }
  if (cur_row >= 0) flush(cur_row);
}

// One lane group per first record: plain sums over the row's records in record order, then the row(s) once.
template <int H, int D, bool COL>
__global__ __launch_bounds__(kFastBlock) void k_attn_bf16_bwd_merge(AttnBf16BwdRec rec, uint4* __restrict__ out0,
                                                                    uint4* __restrict__ out1, i64 n) {
  using C = AttnBf16Cfg<H, D>;
  constexpr int L = C::L, NV = C::NV, NOUT = COL ? 2 : 1;
  constexpr i64 F8 = C::F8;
  const int l = threadIdx.x % L;
  const i64 i = (i64)blockIdx.x * (kFastBlock / L) + threadIdx.x / L;
  if (i >= n) return;
  unsigned w = rec.p_row[i];
  if (w == kBf16RecNone || !(w & kBf16RecFirst)) return;
  const unsigned r = w & kBf16RecRow;
  Bf16Acc acc[NOUT][NV];
#pragma unroll
  for (int k = 0; k < NOUT; ++k)
#pragma unroll
    for (int v = 0; v < NV; ++v) attn_bf16_zero(acc[k][v]);
  for (i64 j = i; j >= 0; j = attn_bf16_rec_next(rec.p_row, j, n, r, w)) {
#pragma unroll
    for (int k = 0; k < NOUT; ++k)
#pragma unroll
      for (int v = 0; v < NV; ++v) attn_bf16_add(acc[k][v], attn_bf16_rec_load(rec.p_acc, (j * NOUT + k) * F8 + v * L + l));
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    out0[(i64)r * F8 + v * L + l] = attn_bf16_round(acc[0][v]);
    if constexpr (COL) out1[(i64)r * F8 + v * L + l] = attn_bf16_round(acc[NOUT - 1][v]);
  }
}

}  // namespace graphop
