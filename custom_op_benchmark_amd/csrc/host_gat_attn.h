// Host-side helpers of the fused GAT attention entry points: argument and plan checks, the conditions of the fp32 fast
// kernels, the (h, d) dispatch and the launch geometry of the gather passes.  Shared by gat_attention.hip and
// gat_edge_attention.hip.  Not part of the C ABI.
#pragma once
#include <initializer_list>

#include "common.h"
#include "host.h"

namespace graphop {

inline int gat_attn_check(const char* fn, int dtype, i64 C, i64 C2, i64 E, i64 n_l, i64 n_r, i64 h, i64 d) {
  GO_TRY(check_async_error(false));   // a kernel of an earlier launch reported a failure: sticky until acknowledged
  GO_CHECK_ARG(dtype == GRAPHOP_F32 || dtype == GRAPHOP_F64, "%s: dtype must be GRAPHOP_F32 or GRAPHOP_F64", fn);
  GO_CHECK_ARG(C >= 0 && C2 >= 0 && E >= 0 && n_l >= 0 && n_r >= 0 && h >= 1 && d >= 1,
               "%s: negative size (n_chunks=%lld/%lld n_edges=%lld n_l=%lld n_r=%lld h=%lld d=%lld)", fn,
               (long long)C, (long long)C2, (long long)E, (long long)n_l, (long long)n_r, (long long)h, (long long)d);
  return GRAPHOP_OK;
}

inline int gat_attn_check_plan(const char* fn, const graphop_plan* p, const char* seg_name, i64 n_seg,
                               const char* idx_name, i64 n_idx) {
  if (!p) return GRAPHOP_OK;
  GO_CHECK_ARG(p->info.max_row < n_seg, "%s: row id %lld but %s has only %lld rows", fn, (long long)p->info.max_row,
               seg_name, (long long)n_seg);
  GO_CHECK_ARG(p->info.max_index < n_idx, "%s: neighbour id %lld but %s has only %lld rows", fn,
               (long long)p->info.max_index, idx_name, (long long)n_idx);
  return GRAPHOP_OK;
}

inline bool a16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fp32 fast kernels: the (h, d) pairs below, ids that fit 31 bits, 16-byte-aligned tables
inline bool gat_attn_fast_ok(int dtype, i64 h, i64 d, i64 E, i64 n_l, i64 n_r, std::initializer_list<const void*> ps) {
  if (tuning().force_generic || dtype != GRAPHOP_F32) return false;
  if (h != 1 && h != 2 && h != 4 && h != 8) return false;
  if (d != 8 && d != 16 && d != 32 && d != 64) return false;
  if (h * d != 64 && h * d != 128 && h * d != 256) return false;
  if (E >= 0x7fffffffLL || n_l >= 0x7fffffffLL || n_r >= 0x7fffffffLL) return false;
  for (const void* p : ps)
    if (!a16(p)) return false;
  return true;
}

#define GO_DISPATCH_GAT_ATTN(h, d, ...)                                 \
  switch ((int)((h) * 1000 + (d))) {                                    \
    case 1064: { constexpr int H = 1, D = 64; __VA_ARGS__; } break;     \
    case 2032: { constexpr int H = 2, D = 32; __VA_ARGS__; } break;     \
    case 2064: { constexpr int H = 2, D = 64; __VA_ARGS__; } break;     \
    case 4016: { constexpr int H = 4, D = 16; __VA_ARGS__; } break;     \
    case 4032: { constexpr int H = 4, D = 32; __VA_ARGS__; } break;     \
    case 4064: { constexpr int H = 4, D = 64; __VA_ARGS__; } break;     \
    case 8008: { constexpr int H = 8, D = 8; __VA_ARGS__; } break;      \
    case 8016: { constexpr int H = 8, D = 16; __VA_ARGS__; } break;     \
    case 8032: { constexpr int H = 8, D = 32; __VA_ARGS__; } break;     \
    default: break;                                                     \
  }

#define GO_DISPATCH_GAT_ATTN_H(h, ...)                  \
  switch ((int)(h)) {                                   \
    case 1: { constexpr int H = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int H = 2; __VA_ARGS__; } break; \
    case 4: { constexpr int H = 4; __VA_ARGS__; } break; \
    case 8: { constexpr int H = 8; __VA_ARGS__; } break; \
    default: break;                                     \
  }

// a run-time bool as the template argument NAME of the statement
#define GO_DISPATCH_BOOL(b, NAME, ...)                   \
  if (b) { constexpr bool NAME = true; __VA_ARGS__; }    \
  else { constexpr bool NAME = false; __VA_ARGS__; }

// ProfScope tag [drop] and kernel label [drop][fast] of a gather pass ("fwd", "bwd_row", "bwd_col").  The drop names
// are those of the DROP = true instantiations of the pass's one kernel template: they name the path taken.
struct GatAttnLabels {
  const char* tag[2];
  const char* kernel[2][2];
};
#define GO_GAT_ATTN_LABELS_OF(op, pass)                               \
  GatAttnLabels{{op "_" pass, op "_drop_" pass},                      \
                {{"k_" op "_" pass "_generic", "k_" op "_" pass "_f32"}, \
                 {"k_" op "_drop_" pass "_generic", "k_" op "_drop_" pass "_f32"}}}
#define GO_GAT_ATTN_LABELS(EDGE, pass) \
  (EDGE ? GO_GAT_ATTN_LABELS_OF("gat_edge_attn", pass) : GO_GAT_ATTN_LABELS_OF("gat_attn", pass))

// chunks per lane group: up to the SpMM cap on big graphs, fewer on small ones so every CU still gets groups
inline int gat_attn_cpg(i64 n_chunks) {
  constexpr int G = 16;
  const i64 groups_wanted = (i64)tuning().n_cu * (kFastBlock / G) * 8;
  i64 c = n_chunks / (groups_wanted > 0 ? groups_wanted : 1);
  if (c < 1) c = 1;
  const int cap = tuning().spmm_cpg > 0 ? tuning().spmm_cpg : 16;
  return (int)(c < cap ? c : cap);
}

// grid of a fast gather pass: lane groups of 16, cpg chunks each
inline unsigned gat_attn_grid(i64 n_chunks, int cpg) {
  return (unsigned)ceil_div(ceil_div(n_chunks, cpg), kFastBlock / 16);
}

inline unsigned grid_of(i64 n) {
  const i64 b = ceil_div(n, 256);
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace graphop
