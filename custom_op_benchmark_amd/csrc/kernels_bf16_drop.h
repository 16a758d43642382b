// The keep decision of attention dropout as the bfloat16 fused GAT and GATv2 layers take it (kernels_gat_attn_bf16.h,
// kernels_gatv2_attn_bf16.h): lane groups of L lanes, SB <= L slots per batch, Philox per slot in the lane that holds the
// slot's id, the keep bits handed round the group like the id.  kernels_dropout.h has the decision itself.
#pragma once
#include "common.h"
#include "kernels_dropout.h"

namespace graphop {

// ---- the keep decision in lane groups of L lanes, SB <= L slots per batch ------------------------------------------------
// Lane l holds slot l % SB.  One Philox call covers four heads; with H = 8 lane SB + t takes the second block of slot t
// where the group has room (2 SB <= L), else lane t makes both calls.
template <int H, int SB, int L>
struct GatBf16DropCfg {
  static constexpr int NB = (H + 3) / 4;
  static constexpr bool SPREAD = NB * SB <= L;
};

template <int H, int SB, int L, bool COL>
__device__ __forceinline__ int gat_bf16_lane_bits(int l, i64 own, int oth, const DropArgs<float>& dr) {
  using C = GatBf16DropCfg<H, SB, L>;
  const unsigned i = COL ? (unsigned)oth : (unsigned)own, j = COL ? (unsigned)own : (unsigned)oth;
  if constexpr (C::SPREAD) {
    return drop_keep4<float>(i, j, (unsigned)(l / SB), dr);   // (lanes past NB * SB: a block nobody reads)
  } else {
    int bits = 0;
#pragma unroll
    for (int b = 0; b < C::NB; ++b) bits |= drop_keep4<float>(i, j, (unsigned)b, dr) << (4 * b);
    return bits;
  }
}

// keep bits of slot U's heads (bit k = head k), in every lane of the group
template <int H, int SB, int L, int U>
__device__ __forceinline__ int gat_bf16_slot_bits(int lane_bits) {
  using C = GatBf16DropCfg<H, SB, L>;
  int bits = group_bcast<L, U>(lane_bits);
  if constexpr (C::SPREAD && C::NB == 2) bits |= group_bcast<L, SB + U>(lane_bits) << 4;
  return bits;
}

}  // namespace graphop
