// The keep decision of attention dropout as the bfloat16 fused GAT and GATv2 layers take it (kernels_gat_attn_bf16.h,
// kernels_gatv2_attn_bf16.h): lane groups of L lanes, SB <= L slots per batch, Philox per slot in the lane that holds the
// slot's id, the keep bits handed round the group like the id.  kernels_dropout.h has the decision itself.  The bf16 fused
// attention step with options (kernels_attn_bf16_opts.h) takes the form with a first global head at the end of this file.
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

// ---- ... with a first global head (the bf16 fused attention step with options, kernels_attn_bf16_opts.h) ---------------
// The call's heads are the global heads head0 .. head0 + H - 1, which fall into one to three Philox blocks.  Lane l works
// for slot l % SB: it runs Philox for the blocks l / SB, l / SB + L / SB, ... of those, moves each block's four decisions
// to the local heads' bit positions (a block that starts before head0 moves down), and the L / SB lanes of a slot OR
// their bits -- the xor steps are multiples of SB, so bits never cross slots and a lane that re-read the batch's last
// slot folds into nothing that is used.  At L == SB (rows of 64 elements) one lane owns a slot, makes every block's call
// itself and there is no cross-lane step.  Returns, in every lane with l % SB == u, slot u's bits (bit k = local head k
// is kept).  (i, j) = (row-major row, neighbour) as in edge_dropout_mask.
template <int H, int SB, int L>
__device__ __forceinline__ int bf16_keep_bits(int l, unsigned i, unsigned j, const DropArgs<float>& dr, int head0) {
  static_assert(SB <= L && L % SB == 0, "slots per batch must divide the lane group");
  const int b0 = head0 >> 2;
  const int nblk = ((head0 + H + 3) >> 2) - b0;
  int bits = 0;
  for (int t = l / SB; t < nblk; t += L / SB) {
    const int k4 = drop_keep4<float>(i, j, (unsigned)(b0 + t), dr);
    const int sh = (b0 + t) * 4 - head0;   // local head of the block's first decision
    bits |= sh >= 0 ? (k4 << sh) : (k4 >> -sh);
  }
#pragma unroll
  for (int s = SB; s < L; s <<= 1) bits |= __shfl_xor(bits, s, L);
  return bits & ((1 << H) - 1);
}

}  // namespace graphop
