// Host side of the fused dot-product attention ops, stated once: the argument checks every entry point makes first
// (attention.hip, attention_edge.hip) and the launch geometry and forward workspace of the several-head chunk-driver
// passes (attention_heads.hip, attention_edge.hip; kernels_attn_rows_passes.inc).
#pragma once
#include "common.h"
#include "host.h"
#include "host_dropout.h"

namespace graphop {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the checks every entry point of the attention ops makes first
inline int attn_check(const char* fn, int dtype, i64 n_row_chunks, i64 n_col_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h,
                      i64 d) {
  GO_CHECK_ARG(dtype == GRAPHOP_F32 || dtype == GRAPHOP_F64, "%s: bad dtype", fn);
  GO_CHECK_ARG(n_row_chunks >= 0 && n_col_chunks >= 0 && n_edges >= 0 && n_q >= 0 && n_k >= 0 && h >= 1 && d >= 0,
               "%s: negative size", fn);
  return GRAPHOP_OK;
}

// the dropout arguments of the entry points that take them, as they arrive; checked after the checks above
struct DropIn {
  double p;
  uint64_t seed;
  uint32_t offset;
  i64 head0;
};

inline int attn_drop_check(const char* fn, const DropIn& in, i64 n_q, i64 n_k, HostDrop* out) {
  GO_TRY(drop_check(fn, in.p, in.seed, n_q, n_k, in.offset, out));
  GO_CHECK_ARG(in.head0 >= 0 && in.head0 < ((i64)1 << 32), "%s: head0 must be in [0, 2^32), got %lld", fn,
               (long long)in.head0);
  return GRAPHOP_OK;
}

// Chunks per lane group and lane groups of a pass over n_chunks chunks: launch_attn_rows' rule for 16-lane groups, with
// four (not eight) rounds of resident workgroups wanted -- these kernels hold 150 to 240 VGPRs, two workgroups per CU
// where the one-head kernels hold four, so the same number of rounds per resident slot needs half the groups, and
// every group of the forward costs two piece records of (1 + 2 h + F) words.
inline void attn_rows_geometry(i64 n_chunks, i64* cpg_out, i64* groups_out) {
  constexpr int GPB = kFastBlock / 16;
  const i64 groups_wanted = (i64)tuning().n_cu * GPB * 4;
  i64 cpg = n_chunks / (groups_wanted > 0 ? groups_wanted : 1);
  cpg = cpg < 1 ? 1 : (cpg > 16 ? 16 : cpg);
  *cpg_out = cpg;
  *groups_out = ceil_div(n_chunks, cpg);
}

// the forward's workspace: np = 2 * groups piece records (row, (m, l) per head, o) and (Mtmp, Ltmp) per (row, head)
struct AttnRowsFwdWs {
  size_t o_row, o_ml, o_po, o_m, o_l, total;
  AttnRowsFwdWs(i64 np, i64 n_q, i64 h, i64 F) {
    o_row = 0;
    o_ml = o_row + up256(sizeof(int) * (size_t)np);
    o_po = o_ml + up256(sizeof(float) * 2 * (size_t)(np * h));
    o_m = o_po + up256(sizeof(float) * (size_t)(np * F));
    o_l = o_m + up256(sizeof(float) * (size_t)(n_q * h));
    total = o_l + up256(sizeof(float) * (size_t)(n_q * h));
  }
};

}  // namespace graphop
