// Host side that the bfloat16 ops share (attention_bf16.hip; gat_attention_bf16.hip, 4.5u): what a
// row-owned plan must offer a record-leaving chunk pass, the chunk geometry of such a pass, the workspace carver, the
// fill of the record row words and the alignment test of the bf16 tables.  Each exists once, here.  Not part of the C ABI.
#pragma once
#include <cstdio>
#include <initializer_list>

#include "common.h"
#include "host.h"
#include "host_attn_rows.h"
#include "kernels_attn_bf16.h"

namespace graphop {

// what one direction asks of ONE plan (own rows n_own, gathered table n_tab); `why` gets the unmet condition
inline bool bf16_plan_unmet(char* why, size_t cap, const char* name, const graphop_plan* plan, i64 n_edges, i64 n_own, i64 n_tab) {
  if (!plan) snprintf(why, cap, "%s is NULL or not the plan of the call's arrays", name);
  else if (!plan->indices) snprintf(why, cap, "%s was made without indices", name);
  else if (!plan->info.row_owned) snprintf(why, cap, "%s is not row_owned (rows sorted, indptr monotone)", name);
  else if (plan->info.max_row >= n_own || plan->info.max_index >= n_tab)
    snprintf(why, cap, "%s holds row id %lld and neighbour id %lld but the tables have %lld and %lld rows", name,
             (long long)plan->info.max_row, (long long)plan->info.max_index, (long long)n_own, (long long)n_tab);
  else if (n_edges >= 0x7fffffffLL || n_tab >= 0x7fffffffLL || n_own > (i64)kBf16RecRow)
    snprintf(why, cap, "%s: ids must lie below 2^31 and row ids below 2^30", name);
  else if (2 * attn_rows_geometry(plan->info.n_chunks).groups >= 0x7fffffffLL)
    snprintf(why, cap, "%s has too many chunks for 32-bit record slots", name);
  else return false;
  return true;
}

// the chunk geometry of a pass: attn_rows_geometry's chunks per group and groups, workgroups for this pair's lane groups
struct Bf16Geo {
  i64 cpg, groups, np;
  int lanes;
  Bf16Geo(i64 n_chunks, int lanes_) : lanes(lanes_) {
    const ChunkGeometry geo = attn_rows_geometry(n_chunks);
    cpg = geo.cpg; groups = geo.groups; np = 2 * geo.groups;
  }
  dim3 grid(i64 n_groups) const { return dim3((unsigned)ceil_div(n_groups, (i64)(kFastBlock / lanes))); }
};

struct Bf16Take {
  char* base;
  size_t total = 0;
  void* operator()(size_t bytes) {
    void* p = base ? base + total : nullptr;
    total += up256(bytes);
    return p;
  }
};

inline void bf16_fill_rows(const char* tag, unsigned* p_row, i64 np, hipStream_t st) {
  ProfScope prof(tag, st, "k_fill");
  const i64 want = ceil_div(np, 256);
  hipLaunchKernelGGL((k_fill<int>), dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(256), 0, st, (int*)p_row, np, -1);
}

inline int bf16_tables_aligned(const char* fn, std::initializer_list<const void*> ps) {
  for (const void* p : ps) GO_CHECK_ARG(aligned16(p), "%s: bfloat16 tables must be 16-byte aligned", fn);
  return GRAPHOP_OK;
}

}  // namespace graphop
