// Edge dropout without an edge-sized mask (extra op).  The keep decision of edge (i, j) and head k is
// a pure function of (i, j, k, seed, offset, p), so every pass that holds both node ids recomputes it:
//   w[0..3] = Philox4x32-10(counter = (i, j, k >> 2, offset), key = (seed & 0xffffffff, seed >> 32))
//   keep = w[k & 3] >= T,  T = floor(p * 2^32);  multiplier m_ijk = keep ? 1 / (1 - p) : 0
// i is the row-major row id (index into el / o), j the neighbour id (index into er / V), in that order in both
// orientations.  Parallel edges (the same (i, j) more than once) share one decision.
#pragma once
#include <type_traits>

#include "kernels_base.h"
#include "kernels_generic.h"

namespace graphop {

// host-prepared arguments of the decision; scale = 1 / (1 - p) in the op's dtype
template <typename T>
struct DropArgs {
  unsigned key0, key1, offset, thresh;
  T scale;
};

// the dropout argument of a kernel templated on DROP: nothing to pass without dropout.  Only `if constexpr (DROP)`
// code may name its members.
struct NoDrop {};
template <bool DROP, typename T>
using DropArgsIf = std::conditional_t<DROP, DropArgs<T>, NoDrop>;

// Philox4x32-10 (Salmon et al., Random123): ten rounds of two 32 x 32 -> 64 multiplies and a key bump
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&w)[4]) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// keep bits of the four heads 4 * blk .. 4 * blk + 3 of edge (i, j): bit t = head 4 * blk + t is kept
template <typename T>
__device__ __forceinline__ int drop_keep4(unsigned i, unsigned j, unsigned blk, const DropArgs<T>& dr) {
  unsigned w[4];
  philox4x32_10(i, j, blk, dr.offset, dr.key0, dr.key1, w);
  return (int)(w[0] >= dr.thresh) | ((int)(w[1] >= dr.thresh) << 1) | ((int)(w[2] >= dr.thresh) << 2) |
         ((int)(w[3] >= dr.thresh) << 3);
}

// m_ijk of one head (generic kernels: one Philox call per use)
template <typename T>
__device__ __forceinline__ T drop_mult(i64 i, i64 j, i64 k, const DropArgs<T>& dr) {
  return (drop_keep4<T>((unsigned)i, (unsigned)j, (unsigned)(k >> 2), dr) >> (int)(k & 3)) & 1 ? dr.scale : (T)0;
}

// ---- the decision in the fast gather passes of the fused GAT and GATv2 layers (16-lane groups) ------------------------
// The lanes that load a batch's neighbour ids also run Philox for them: lane t < SB holds slot t.  One call covers four
// heads; for H = 8 lane SB + t takes the second block of slot t where the group has room (2 * SB <= L), else lane t
// makes both calls.  `own` is the chunk's node, `oth` the gathered one; COL says which of them is the row-major row i.
template <int H, int SB>
struct GatDropCfg {
  static constexpr int L = 16;
  static constexpr int NB = (H + 3) / 4;            // Philox blocks per slot
  static constexpr bool SPREAD = NB * SB <= L;      // one block per lane
  static constexpr int LANES = SPREAD ? NB * SB : SB;   // lanes that load an id
};

template <int H, int SB, bool COL>
__device__ __forceinline__ int gat_drop_lane_bits(int l, i64 own, int oth, const DropArgs<float>& dr) {
  using C = GatDropCfg<H, SB>;
  const unsigned i = COL ? (unsigned)oth : (unsigned)own, j = COL ? (unsigned)own : (unsigned)oth;
  if constexpr (C::SPREAD) {
    return drop_keep4<float>(i, j, (unsigned)(l / SB), dr);
  } else {
    int bits = 0;
#pragma unroll
    for (int b = 0; b < C::NB; ++b) bits |= drop_keep4<float>(i, j, (unsigned)b, dr) << (4 * b);
    return bits;
  }
}

// keep bits of slot U's heads (bit k = head k), in every lane of the group
template <int H, int SB, int U>
__device__ __forceinline__ int gat_drop_slot_bits(int lane_bits) {
  using C = GatDropCfg<H, SB>;
  int bits = group_bcast<C::L, U>(lane_bits);
  if constexpr (C::SPREAD && C::NB == 2) bits |= group_bcast<C::L, SB + U>(lane_bits) << 4;
  return bits;
}

// y[eid[j], k] = m_ijk over the row-major chunks (i = row[c], j = indices[slot]); one wave per chunk, lanes over
// (slot, block of four heads) pairs: one Philox call per four values.
template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_edge_dropout_mask(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, T* __restrict__ y, i64 n_chunks, i64 h, DropArgs<T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c];
  const i64 nblk = (h + 3) / 4;
  const i64 items = (indptr[c + 1] - j0) * nblk;
  for (i64 it = lane; it < items; it += kWave) {
    const i64 j = j0 + it / nblk, b = it % nblk;
    const int bits = drop_keep4<T>((unsigned)r, (unsigned)indices[j], (unsigned)b, dr);
    T* out = y + eid[j] * h + b * 4;
    const int n = h - b * 4 < 4 ? (int)(h - b * 4) : 4;
    for (int t = 0; t < n; ++t) out[t] = (bits >> t) & 1 ? dr.scale : (T)0;
  }
}

// y[eid[slot], k] = x[eid[slot], k] * m_{i j (head0 + k)} for the call's heads k < h over the row-major chunks (the
// composed path of the fused attention op with dropout); x == y is allowed.  Lanes over (slot, Philox
// block) pairs like k_edge_dropout_mask: the blocks are those the GLOBAL heads head0 .. head0 + h - 1 fall into, so a
// head0 that is no multiple of 4 costs one more call per slot, not one per value.  A dropped value is written as 0
// whatever x holds.
template <typename T>
__global__ __launch_bounds__(kGenericBlock) void k_attn_drop_apply(
    const i64* __restrict__ row, const i64* __restrict__ indptr, const i64* __restrict__ eid,
    const i64* __restrict__ indices, const T* x, T* y, i64 n_chunks, i64 h, i64 head0, DropArgs<T> dr) {
  const i64 c = generic_chunk_id();
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const i64 r = row[c];
  const i64 j0 = indptr[c];
  const i64 b0 = head0 >> 2;
  const i64 nblk = ((head0 + h + 3) >> 2) - b0;
  const i64 len = indptr[c + 1] - j0;
  if (nblk == 1) {   // the call's heads share one Philox block (every head group of up to four aligned heads): no division
    for (i64 s = lane; s < len; s += kWave) {
      const i64 j = j0 + s;
      const int bits = drop_keep4<T>((unsigned)r, (unsigned)indices[j], (unsigned)b0, dr);
      const i64 base = eid[j] * h;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const i64 k = b0 * 4 + t - head0;
        if (k >= 0 && k < h) y[base + k] = (bits >> t) & 1 ? x[base + k] * dr.scale : (T)0;
      }
    }
    return;
  }
  const i64 items = len * nblk;
  for (i64 it = lane; it < items; it += kWave) {
    const i64 j = j0 + it / nblk, b = b0 + it % nblk;
    const int bits = drop_keep4<T>((unsigned)r, (unsigned)indices[j], (unsigned)b, dr);
    const i64 base = eid[j] * h;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const i64 k = b * 4 + t - head0;
      if (k >= 0 && k < h) y[base + k] = (bits >> t) & 1 ? x[base + k] * dr.scale : (T)0;
    }
  }
}

}  // namespace graphop
