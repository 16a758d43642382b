// Host-side helpers of the GAT family of entry points (gat.hip, gatv2.hip, gat_attention.hip, gat_edge_attention.hip,
// gatv2_attention.hip, gatv2_edge_attention.hip, gat_weights.hip, host_gat_attn_ops.h and host_gatv2_attn_ops.h):
// argument and plan checks (the plan of an orientation, its bounds and its edge-id argument are host.h's Csr), the
// conditions of the fp32
// fast kernels, the (h, d), bool and fp32 / fp64 dispatch, the one launch statement of a kernel with and without edge
// term (go_launch, arg_if, GO_EDGE_KERNEL), the profile labels, the launch geometry
// of the gather passes and the opening of the two GATv2 backwards.  Each exists once, here.  Not part of the C ABI.
#pragma once
#include <cstdio>
#include <initializer_list>
#include <tuple>
#include <type_traits>

#include "common.h"
#include "host.h"

namespace graphop {

constexpr int kGatGroup = 16;            // lanes per group of the (h, d) fast kernels
constexpr i64 kGatMaxRowBlocks = 8192;   // workgroups of a fast GATv2 row pass at most: bounds the datt partials

// has_d = false: an op without a feature width (gat_scores), whose message has no d= field
inline int gat_check(const char* fn, int dtype, i64 C, i64 C2, i64 E, i64 n_l, i64 n_r, i64 h, i64 d,
                     bool has_d = true) {
  GO_TRY(check_async_error(false));   // a kernel of an earlier launch reported a failure: sticky until acknowledged
  GO_CHECK_ARG(dtype == GRAPHOP_F32 || dtype == GRAPHOP_F64, "%s: dtype must be GRAPHOP_F32 or GRAPHOP_F64", fn);
  char d_field[32] = "";
  if (has_d) snprintf(d_field, sizeof(d_field), " d=%lld", (long long)d);
  GO_CHECK_ARG(C >= 0 && C2 >= 0 && E >= 0 && n_l >= 0 && n_r >= 0 && h >= 1 && d >= 1,
               "%s: negative size (n_chunks=%lld/%lld n_edges=%lld n_l=%lld n_r=%lld h=%lld%s)", fn, (long long)C,
               (long long)C2, (long long)E, (long long)n_l, (long long)n_r, (long long)h, d_field);
  return GRAPHOP_OK;
}
inline int gat_check(const char* fn, int dtype, i64 C, i64 C2, i64 E, i64 n_l, i64 n_r, i64 h) {
  return gat_check(fn, dtype, C, C2, E, n_l, n_r, h, 1, false);
}

// a per-(node or edge, head) array as the fast kernels read and write it: aligned to its item width, 4 * min(h, 4) bytes
inline bool gat_aligned(const void* p, i64 h) {
  const uintptr_t a = h >= 4 ? 16 : (uintptr_t)(4 * h);
  return ((uintptr_t)p % a) == 0;
}

// fp32 fast kernels of the (h, d) ops: the pairs of GO_DISPATCH_GAT_HD, ids that fit 31 bits, 16-byte-aligned tables
inline bool gat_hd_fast_ok(int dtype, i64 h, i64 d, i64 E, i64 n_l, i64 n_r, std::initializer_list<const void*> ps) {
  if (tuning().force_generic || dtype != GRAPHOP_F32) return false;
  if (h != 1 && h != 2 && h != 4 && h != 8) return false;
  if (d != 8 && d != 16 && d != 32 && d != 64) return false;
  if (h * d != 64 && h * d != 128 && h * d != 256) return false;
  if (E >= 0x7fffffffLL || n_l >= 0x7fffffffLL || n_r >= 0x7fffffffLL) return false;
  for (const void* p : ps)
    if (!aligned16(p)) return false;
  return true;
}

// fp32 fast kernels of an op without a feature width (gat_weights.hip): the head counts of GO_DISPATCH_GAT_ATTN_H, ids
// that fit 31 bits, the per-(node or edge, head) arrays `items` aligned to their item width (NULL: an operand the call
// does not have) and the (n, h, 2) statistics to the float2 they are loaded as
inline bool gat_h_fast_ok(int dtype, i64 h, i64 E, i64 n_l, i64 n_r, std::initializer_list<const void*> items,
                          const void* stats) {
  if (tuning().force_generic || dtype != GRAPHOP_F32) return false;
  if (h != 1 && h != 2 && h != 4 && h != 8) return false;
  if (E >= 0x7fffffffLL || n_l >= 0x7fffffffLL || n_r >= 0x7fffffffLL) return false;
  for (const void* p : items)
    if (!gat_aligned(p, h)) return false;
  return ((uintptr_t)stats % 8) == 0;
}

#define GO_DISPATCH_GAT_HD(h, d, ...)                                   \
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

// the head counts of the fused stats kernel (gat.hip has its own list, which also holds 16)
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

// the run-time dtype (GRAPHOP_F32 or GRAPHOP_F64: gat_check) as the type NAME of the statement
#define GO_DISPATCH_FLOAT(dtype, NAME, ...)                         \
  if ((dtype) == GRAPHOP_F32) { using NAME = float; __VA_ARGS__; } \
  else { using NAME = double; __VA_ARGS__; }

// One launch statement for a kernel and its edge form, whose parameter list is the plain one with the edge arguments
// spliced in (eid, ee / xe, dee / dxe): the call lists every argument in the edge kernel's order and wraps those that
// only the edge kernel takes in arg_if<EDGE>(...).  arg_if<false>(x) adds nothing to the list (x is still evaluated).
// A std::tuple in the list stands for its elements (host_attn_edge_ops.h: the arguments a form's edge rows arrive as);
// go_launch_lds is go_launch with dynamic LDS.
template <bool ON, class T> struct ArgIf { T v; };
template <bool ON, class T> ArgIf<ON, T> arg_if(T v) { return {v}; }
template <class T> std::tuple<T> launch_arg(T v) { return {v}; }
template <class T> std::tuple<T> launch_arg(ArgIf<true, T> a) { return {a.v}; }
template <class T> std::tuple<> launch_arg(ArgIf<false, T>) { return {}; }
template <class... T> std::tuple<T...> launch_arg(std::tuple<T...> t) { return t; }   // a run of arguments, in place
template <class K, class... A>
void go_launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  std::apply([&](auto... a) { hipLaunchKernelGGL(kernel, grid, block, lds, st, a...); },
             std::tuple_cat(launch_arg(args)...));
}
template <class K, class... A>
void go_launch(K kernel, dim3 grid, dim3 block, hipStream_t st, A... args) {
  go_launch_lds(kernel, grid, block, 0, st, args...);
}
static_assert(std::is_same_v<decltype(std::tuple_cat(launch_arg(arg_if<false>(1)), launch_arg(2.f))),
                             std::tuple<float>>, "arg_if<false> drops its argument");
static_assert(std::is_same_v<decltype(std::tuple_cat(launch_arg(arg_if<true>(1)), launch_arg(2.f))),
                             std::tuple<int, float>>, "arg_if<true> keeps its argument, in place");

// &plain<...> or, with the edge term, &edge<...>: only the chosen one is instantiated, so a translation unit compiles
// only its own EDGE's kernels.  The template arguments must be constants usable without capture (H, D, OWNED, DROP, T).
#define GO_EDGE_KERNEL(EDGE, plain, edge, ...) \
  ([] { if constexpr (EDGE) return &edge<__VA_ARGS__>; else return &plain<__VA_ARGS__>; }())

// ProfScope tag [drop] and kernel label [drop][fast] of a gather pass ("fwd", "bwd_row", "bwd_col") of the fused op
// `op`.  The drop names are those of the path taken: the DROP = true instantiations, the k_gv2drop_* kernels.
struct GatLabels {
  const char* tag[2];
  const char* kernel[2][2];
};
#define GO_GAT_LABELS_OF(op, pass)                                \
  GatLabels{{op "_" pass, op "_drop_" pass},                      \
            {{"k_" op "_" pass "_generic", "k_" op "_" pass "_f32"}, \
             {"k_" op "_drop_" pass "_generic", "k_" op "_drop_" pass "_f32"}}}

// chunks per lane group of G lanes (chunks_per_group) with the tuned cap, sddmm_cpg or spmm_cpg; below 1 it counts as 1
inline int gat_cpg(i64 n_chunks, int cap, int G = kGatGroup) {
  return (int)chunks_per_group(n_chunks, G, cap < 1 ? 1 : cap);
}

// grid of a fast gather pass: lane groups of G lanes, cpg chunks each
inline i64 gat_grid(i64 n_chunks, i64 cpg, int G = kGatGroup) {
  return ceil_div(ceil_div(n_chunks, cpg), (i64)(kFastBlock / G));
}

// rows of datt partials a fast GATv2 row pass may write (include/graphop_hip.h states this in the workspace minimum)
inline i64 gat_part_rows(i64 n_row_chunks) {
  const i64 b = ceil_div(n_row_chunks, (i64)(kFastBlock / kGatGroup));
  return b < kGatMaxRowBlocks ? b : kGatMaxRowBlocks;
}

// cpg and grid of a fast GATv2 row pass: gat_cpg, raised where its grid would exceed kGatMaxRowBlocks, so that
// n_blocks <= gat_part_rows(n_chunks)
struct GatRowPass {
  int cpg;
  i64 n_blocks;
};
inline GatRowPass gat_row_pass(i64 n_chunks, int cap) {
  i64 cpg = gat_cpg(n_chunks, cap);
  if (gat_grid(n_chunks, cpg) > kGatMaxRowBlocks)
    cpg = ceil_div(n_chunks, kGatMaxRowBlocks * (kFastBlock / kGatGroup));
  return {(int)cpg, gat_grid(n_chunks, cpg)};
}

inline unsigned grid_of(i64 n) {
  const i64 b = ceil_div(n, 256);
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// The opening of the two GATv2 backwards (gatv2_scores_backward, gatv2_attention[_dropout]_backward), after their own
// workspace check: the plans of the two orientations checked against the operands' row counts, and the zero fills of
// the outputs.  The outputs of an orientation without chunks may be NULL: that half of the op is skipped.
inline int gatv2_bwd_open(const char* fn, int dtype, const Csr& r, const Csr& c, void* dxl, void* dxr, void* datt, i64 n_l,
                          i64 n_r, i64 f, hipStream_t st) {
  const size_t es = esize(dtype);
  const i64 n_row_chunks = r.n_chunks, n_col_chunks = c.n_chunks;
  GO_TRY(Csr::check_bounds(fn, r.plan, "xl / dxl", n_l, "xr", n_r));
  GO_TRY(Csr::check_bounds(fn, c.plan, "xr / dxr", n_r, "xl", n_l));
  const bool row_half = !(dxl == nullptr && datt == nullptr && n_row_chunks == 0);
  const bool col_half = !(dxr == nullptr && n_col_chunks == 0);
  if (row_half) {
    if (n_l > 0) {
      GO_PTR(fn, dxl);
      GO_HIP(zero_async(dxl, es * (size_t)(n_l * f), st));
    }
    GO_PTR(fn, datt);
    GO_HIP(zero_async(datt, es * (size_t)f, st));
  }
  if (col_half && n_r > 0) {
    GO_PTR(fn, dxr);
    GO_HIP(zero_async(dxr, es * (size_t)(n_r * f), st));
  }
  return GRAPHOP_OK;
}

}  // namespace graphop
