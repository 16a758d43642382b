// Host side that the two translation units of the bfloat16 fused attention step share (attention_bf16.hip: the plain
// step; attention_bf16_opts.hip: dropout and a per-edge score bias, 4.5w): the pairs of the set, what is
// refused, and the two workspace layouts.  Each exists once, here.  Not part of the C ABI.
#pragma once
#include "host_bf16.h"
#include "host_gat.h"

namespace graphop {

// the bf16 set: the pairs of GO_DISPATCH_GAT_HD, (1, 128) and (8, 64) -- rows of 64, 128, 256 or 512 elements
#define GO_DISPATCH_ATTN_BF16_HD(h, d, ...)                              \
  switch ((int)((h) * 1000 + (d))) {                                     \
    case 1128: { constexpr int H = 1, D = 128; __VA_ARGS__; } break;     \
    case 8064: { constexpr int H = 8, D = 64; __VA_ARGS__; } break;      \
    default: GO_DISPATCH_GAT_HD(h, d, __VA_ARGS__); break;               \
  }

// lanes per group of a pair of the set, 0 outside it
inline int bf16_lanes(i64 h, i64 d) {
  int lanes = 0;
  if (h >= 1 && h <= 8 && d >= 8 && d <= 128) GO_DISPATCH_ATTN_BF16_HD(h, d, { lanes = AttnBf16Cfg<H, D>::L; });
  return lanes;
}

inline bool bf16_shape_unmet(char* why, size_t cap, i64 h, i64 d) {
  if (bf16_lanes(h, d)) return false;
  snprintf(why, cap, "(h, d) = (%lld, %lld) is not in the bfloat16 set: 1 x 64, 1 x 128, 8 x 64 and the several-head pairs",
           (long long)h, (long long)d);
  return true;
}

// forward: 2 * groups records of (row word | (m, l) per head | o row), all fp32
struct Bf16FwdWs {
  unsigned* p_row;
  float *p_ml, *p_o;
  size_t total;
  Bf16FwdWs(void* base, i64 np, i64 h, i64 F) {
    Bf16Take take{(char*)base};
    p_row = (unsigned*)take(sizeof(unsigned) * (size_t)np);
    p_ml = (float*)take(sizeof(float) * 2 * (size_t)(np * h));
    p_o = (float*)take(sizeof(float) * (size_t)(np * F));
    total = take.total;
  }
};

// backward: the packed (K | V) and (Q | dO) tables of 2 F bf16 per node, stats4 per (query row, head), and the records
// of whichever pass is running -- the row pass's np_r of F floats, then the column pass's np_c of 2 F
struct Bf16BwdWs {
  uint4 *kv, *qdo;
  float4* st4;
  unsigned* p_row;
  float* p_acc;
  size_t total;
  Bf16BwdWs(void* base, i64 n_q, i64 n_k, i64 h, i64 F, i64 np_r, i64 np_c) {
    Bf16Take take{(char*)base};
    kv = (uint4*)take(2 * (size_t)(n_k * 2 * F));
    qdo = (uint4*)take(2 * (size_t)(n_q * 2 * F));
    st4 = (float4*)take(sizeof(float4) * (size_t)(n_q * h));
    p_row = (unsigned*)take(sizeof(unsigned) * (size_t)(np_r > np_c ? np_r : np_c));
    p_acc = (float*)take(sizeof(float) * (size_t)(np_r > 2 * np_c ? np_r : 2 * np_c) * (size_t)F);
    total = take.total;
  }
};

}  // namespace graphop
