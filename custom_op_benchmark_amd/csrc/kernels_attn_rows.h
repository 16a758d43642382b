// What the several-head chunk-driver passes of the fused dot-product attention ops share under no op's name
// (kernels_attn_rows_passes.inc).  Everything here is constexpr, a template or __forceinline__, so
// any number of translation units may include it.
#pragma once
#include "kernels_attn.h"
#include "kernels_gat_attn.h"

namespace graphop {

constexpr float kAttnNegBig = -3.0e38f;   // "no score yet" (finite: differences of two of them are 0, not NaN)
__device__ __forceinline__ float attn_rows_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }   // x <= 0

__device__ __forceinline__ float4 attn_rows_add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ void attn_rows_fma4(float4& acc, float w, const float4& x) {
  acc.x = fmaf(w, x.x, acc.x); acc.y = fmaf(w, x.y, acc.y); acc.z = fmaf(w, x.z, acc.z); acc.w = fmaf(w, x.w, acc.w);
}

// The layout of the fused GAT layer (GatAttnCfg<H, D>, kernels_gat_attn.h) for a row of F = H * D floats, H = 1 admitted:
// a lane group of L = 16 lanes holds the row's F4 = H * D / 4 float4 pieces, piece p = v * L + l, so the DQ = D / 4
// pieces of one head sit in DQ adjacent lanes.
template <int H, int D>
struct AttnRowsCfg {
  using G = GatAttnCfg<H, D>;
  static constexpr int L = G::L, F4 = G::F4, NV = G::NV, DQ = G::DQ;
  // slots per batch: the kernels gather two rows per slot (K | V, or the packed pair), 16 float4 pieces in flight per
  // lane as in AttnCfg (64 VGPRs); GatAttnCfg::SB_FWD would put 128 in flight.  An edge piece is a temporary that dies
  // into them, so no instantiation needs a smaller batch to stay out of scratch (at most 228 VGPRs).
  static constexpr int SB = 8 / NV;
};

}  // namespace graphop
