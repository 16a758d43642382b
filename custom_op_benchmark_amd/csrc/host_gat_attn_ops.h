// The stats, forward and backward of the fused GAT layer behind the entry points of gat_attention.hip (EDGE = false:
// z = el[i] + er[j], the k_gat_attn_* kernels) and gat_edge_attention.hip (EDGE = true: z = (el[i] + er[j]) + ee[e], the
// k_gat_edge_attn_* kernels, and the extra output dee).  One implementation: validation, fills, early returns, the
// choice between the fp32 fast kernels and the generic ones, the launch geometry and the profile tags are the same for
// both; with the edge term ee / dee must also be aligned for the fast kernels, a plan with eid_identity passes them a
// NULL eid, and dee is zero-filled unless the plan proves every edge id is written.  A translation unit instantiates
// only its own EDGE, so only its own kernels; ee and dee are ignored without the edge term.  Every launch is written
// once, with the edge kernel's argument list: GO_EDGE_KERNEL names the kernel of this EDGE, and the arguments that only
// the edge kernels take (eid, ee, dee) stand in arg_if<EDGE>(...), which drops them without the edge term (host_gat.h).
// Not part of the C ABI.
#pragma once
#include <type_traits>

#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_gat_edge_attn.h"

namespace graphop {

#define GO_GAT_ATTN_LABELS(EDGE, pass) \
  (EDGE ? GO_GAT_LABELS_OF("gat_edge_attn", pass) : GO_GAT_LABELS_OF("gat_attn", pass))

// stats = (m, 1 / l) per (row, head); rows without slots keep (-1e9, 0)
template <bool EDGE>
int gat_attn_stats(int dtype, const Csr& g, const void* el, const void* er, const void* ee, void* stats, i64 C, i64 n_l,
                   i64 h, double slope, bool fast, hipStream_t st) {
  const graphop_plan* pm = g.plan;   // (fast: not NULL)
  GO_DISPATCH_FLOAT(dtype, T, {
    hipLaunchKernelGGL((k_gat_attn_stats_init_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
  });
  GO_LAUNCH_CHECK();
  if (C == 0) return GRAPHOP_OK;
  const char* tag = EDGE ? "gat_edge_attn_stats" : "gat_attn_stats";
  if (fast && pm->info.row_owned && pm->seg_chunk) {
    const i64 S = pm->info.n_segments;
    if (S == 0) return GRAPHOP_OK;
    ProfScope prof(tag, st, EDGE ? "k_gat_edge_attn_stats_f32" : "k_gat_attn_stats_f32");
    const int n_long = (int)pm->n_long;
    const i64 long_len = n_long > 0 ? kLongSegment : ((i64)1 << 62);
    const bool wide = pm->info.n_edges / S >= 64;   // long rows on average: a wave per segment
    GO_DISPATCH_GAT_ATTN_H(h, GO_DISPATCH_BOOL(wide, WIDE, {
      constexpr int G = WIDE ? 64 : 16;
      const unsigned nbs = (unsigned)ceil_div(S, kFastBlock / G);
      const dim3 grid(nbs + (unsigned)n_long);
      go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_stats_f32, k_gat_edge_attn_stats_f32, H, G), grid, dim3(kFastBlock), st,
                g.row, g.indptr, arg_if<EDGE>(g.eid_or_null()), g.indices, (const i64*)pm->seg_chunk, (const float*)el,
                (const float*)er, arg_if<EDGE>((const float*)ee), (float2*)stats, S, nbs, long_len,
                (const int*)pm->long_segs, (float)slope);
    }));
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
  ProfScope prof(tag, st, EDGE ? "k_gat_edge_attn_stats_generic" : "k_gat_attn_stats_generic");
  const dim3 grid((unsigned)ceil_div(C, kGenericWavesPerBlock));
  GO_DISPATCH_FLOAT(dtype, T, {
    auto pass = [&](auto sum) {
      constexpr bool SUM = decltype(sum)::value;
      go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_stats_generic, k_gat_edge_attn_stats_generic, T, SUM), grid,
                dim3(kGenericBlock), st, g.row, g.indptr, arg_if<EDGE>(g.eid), g.indices, (const T*)el, (const T*)er,
                arg_if<EDGE>((const T*)ee), (T*)stats, C, h, (T)slope);
    };
    pass(std::false_type{});   // the maxima
    pass(std::true_type{});    // the sums of exp(s - m)
    hipLaunchKernelGGL((k_gat_attn_stats_fin_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

// drop == nullptr: the op without dropout (the DROP = false kernels, whatever the entry point)
template <bool EDGE>
int gat_attn_forward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                     const int64_t* indices, const void* el, const void* er, const void* ee, const void* V, void* o,
                     void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                     double negative_slope, const HostDrop* drop, const graphop_plan_t* plan, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "el / o", n_l, "er / V", n_r));
  if (n_l == 0) return GRAPHOP_OK;
  GO_PTR(fn, o); GO_PTR(fn, stats);
  GO_HIP(zero_async(o, es * (size_t)(n_l * h * d), st));
  const bool slots = n_chunks > 0 && n_edges > 0;
  if (slots) {
    GO_TRY(g.require(fn));
    GO_PTR(fn, el); GO_PTR(fn, er);
    if constexpr (EDGE) GO_PTR(fn, ee);
    GO_PTR(fn, V);
  }
  const bool fast = pm && gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {el, er, V, o, stats}) &&
                    (!EDGE || gat_aligned(ee, h));
  GO_TRY(gat_attn_stats<EDGE>(dtype, g, el, er, ee, stats, slots ? n_chunks : 0, n_l, h, negative_slope, fast, st));
  if (!slots) return GRAPHOP_OK;
  const bool dropped = drop != nullptr;
  static const GatLabels lab = GO_GAT_ATTN_LABELS(EDGE, "fwd");
  ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][fast]);
  if (fast) {
    const int cpg = gat_cpg(n_chunks, tuning().spmm_cpg);
    const bool owned = g.owned();
    const dim3 grid((unsigned)gat_grid(n_chunks, cpg));
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
      go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_fwd_f32, k_gat_edge_attn_fwd_f32, H, D, OWNED, DROP), grid,
                dim3(kFastBlock), st, g.row, g.indptr, arg_if<EDGE>(g.eid_or_null()),
                g.indices, (const float*)el, (const float*)er, arg_if<EDGE>((const float*)ee),
                (const float2*)stats, (const float*)V, (float*)o, n_chunks, cpg, (float)negative_slope,
                drop_arg<DROP, float>(drop));
    })));
  } else {
    const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
    GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
      go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_fwd_generic, k_gat_edge_attn_fwd_generic, T, DROP), grid,
                dim3(kGenericBlock), st, g.row, g.indptr, arg_if<EDGE>(g.eid),
                g.indices, (const T*)el, (const T*)er, arg_if<EDGE>((const T*)ee), (const T*)stats,
                (const T*)V, (T*)o, n_chunks, h, d, (T)negative_slope, drop_arg<DROP, T>(drop));
    }));
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

template <bool EDGE>
int gat_attn_backward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                      const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c, const int64_t* eid_c,
                      const int64_t* indices_c, const void* el, const void* er, const void* ee, const void* V,
                      const void* o, const void* stats, const void* dO, void* del, void* der, void* dee, void* dV,
                      void* workspace, int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                      int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope,
                      const HostDrop* drop, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || n_col_chunks > 0);
  const size_t need = slots ? es * 4 * (size_t)(n_l * h) : 0;   // P: (n_l, h, 4)
  GO_CHECK_ARG(workspace_bytes >= 0 && (size_t)workspace_bytes >= need,
               "%s: workspace of %lld bytes needed (n_l * h * 4 values), got %lld", fn, (long long)need,
               (long long)workspace_bytes);
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const graphop_plan *pr = r.plan, *pc = c.plan;
  GO_TRY(Csr::check_bounds(fn, pr, "el / del", n_l, "er / V", n_r));
  GO_TRY(Csr::check_bounds(fn, pc, "er / der", n_r, "el", n_l));
  if (n_l > 0 && !(del == nullptr && n_row_chunks == 0)) {
    GO_PTR(fn, del);
    GO_HIP(zero_async(del, es * (size_t)(n_l * h), st));
  }
  if (n_r > 0 && !(der == nullptr && dV == nullptr && n_col_chunks == 0)) {
    GO_PTR(fn, der); GO_PTR(fn, dV);
    GO_HIP(zero_async(der, es * (size_t)(n_r * h), st));
    GO_HIP(zero_async(dV, es * (size_t)(n_r * h * d), st));
  }
  if constexpr (EDGE) {
    // edge ids that no row-major slot names get dee = 0: skip the fill only where the plan proves every id is written
    const bool dee_run = slots && n_l > 0 && n_r > 0 && n_row_chunks > 0;
    const bool covered = dee_run && r.covered();
    if (dee && n_edges > 0 && !covered) GO_HIP(zero_async(dee, es * (size_t)(n_edges * h), st));
  }
  if (!slots || n_l == 0 || n_r == 0) return GRAPHOP_OK;
  GO_PTR(fn, el); GO_PTR(fn, er);
  if constexpr (EDGE) GO_PTR(fn, ee);
  GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  GO_PTR(fn, workspace);
  const bool ok = gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {el, er, V, o, stats, dO, workspace, dV}) &&
                  (!EDGE || (gat_aligned(ee, h) && gat_aligned(dee, h)));
  const float slope = (float)negative_slope;
  const bool dropped = drop != nullptr;
  const int G = 16;
  {   // P[i, k] = (el, m, 1/l, D): the edge term is not in it
    const bool fast = ok && (pr || pc);
    ProfScope prof(EDGE ? "gat_edge_attn_pack" : "gat_attn_pack", st,
                   fast ? "k_gat_attn_pack_f32" : "k_gat_attn_pack_generic");
    if (fast) {
      GO_DISPATCH_GAT_HD(h, d, {
        hipLaunchKernelGGL((k_gat_attn_pack_f32<H, D>), dim3((unsigned)ceil_div(n_l, kFastBlock / G)),
                           dim3(kFastBlock), 0, st, (const float*)el, (const float2*)stats, (const float*)dO,
                           (const float*)o, (float4*)workspace, n_l);
      });
    } else {
      GO_DISPATCH_FLOAT(dtype, T, {
        hipLaunchKernelGGL((k_gat_attn_pack_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (const T*)el,
                           (const T*)stats, (const T*)dO, (const T*)o, (T*)workspace, n_l * h, d);
      });
    }
    GO_LAUNCH_CHECK();
  }
  if (n_row_chunks > 0) {
    GO_TRY(r.require(fn));
    const i64 C = n_row_chunks;
    const bool fast = ok && pr;
    static const GatLabels lab = GO_GAT_ATTN_LABELS(EDGE, "bwd_row");
    ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][fast]);
    if (fast) {
      const int cpg = gat_cpg(C, tuning().spmm_cpg);
      const bool owned = r.owned();
      const dim3 grid((unsigned)gat_grid(C, cpg));
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_bwd_row_f32, k_gat_edge_attn_bwd_row_f32, H, D, OWNED, DROP), grid,
                  dim3(kFastBlock), st, r.row, r.indptr, arg_if<EDGE>(r.eid_or_null()),
                  r.indices, (const float*)er, arg_if<EDGE>((const float*)ee), (const float*)V,
                  (const float4*)workspace, (const float*)dO, (float*)del, arg_if<EDGE>((float*)dee), C, cpg, slope,
                  drop_arg<DROP, float>(drop));
      })));
    } else {
      const dim3 grid((unsigned)ceil_div(C, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_bwd_row_generic, k_gat_edge_attn_bwd_row_generic, T, DROP), grid,
                  dim3(kGenericBlock), st, r.row, r.indptr, arg_if<EDGE>(r.eid),
                  r.indices, (const T*)er, arg_if<EDGE>((const T*)ee), (const T*)V, (const T*)workspace,
                  (const T*)dO, (T*)del, arg_if<EDGE>((T*)dee), C, h, d, (T)negative_slope, drop_arg<DROP, T>(drop));
      }));
    }
    GO_LAUNCH_CHECK();
  }
  if (n_col_chunks > 0) {
    GO_TRY(c.require(fn));
    const i64 C = n_col_chunks;
    const bool fast = ok && pc;
    static const GatLabels lab = GO_GAT_ATTN_LABELS(EDGE, "bwd_col");
    ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][fast]);
    if (fast) {
      const int cpg = gat_cpg(C, tuning().spmm_cpg);
      const bool owned = c.owned();
      const dim3 grid((unsigned)gat_grid(C, cpg));
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_bwd_col_f32, k_gat_edge_attn_bwd_col_f32, H, D, OWNED, DROP), grid,
                  dim3(kFastBlock), st, c.row, c.indptr, arg_if<EDGE>(c.eid_or_null()),
                  c.indices, (const float*)er, arg_if<EDGE>((const float*)ee), (const float*)V,
                  (const float4*)workspace, (const float*)dO, (float*)der, (float*)dV, C, cpg, slope,
                  drop_arg<DROP, float>(drop));
      })));
    } else {
      const dim3 grid((unsigned)ceil_div(C, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch(GO_EDGE_KERNEL(EDGE, k_gat_attn_bwd_col_generic, k_gat_edge_attn_bwd_col_generic, T, DROP), grid,
                  dim3(kGenericBlock), st, c.row, c.indptr, arg_if<EDGE>(c.eid),
                  c.indices, (const T*)er, arg_if<EDGE>((const T*)ee), (const T*)V, (const T*)workspace,
                  (const T*)dO, (T*)der, (T*)dV, C, h, d, (T)negative_slope, drop_arg<DROP, T>(drop));
      }));
    }
    GO_LAUNCH_CHECK();
  }
  return GRAPHOP_OK;
}

}  // namespace graphop
