// The forward and backward of the fused GATv2 layer behind the entry points of gatv2_attention.hip (EDGE = false:
// z = xl[i] + xr[j], the k_gv2attn_* / k_gv2drop_* kernels) and gatv2_edge_attention.hip (EDGE = true:
// z = (xl[i] + xr[j]) + xe[e], the k_gv2edge_* / k_gv2edrop_* kernels, and the extra output dxe).  One implementation:
// validation, fills, early returns, the choice between the fp32 fast kernels and the generic ones, the launch geometry
// and the workspace are the same for both.  With the edge row, xe / dxe must also be 16-byte aligned for the fast
// kernels, xe must not be NULL, a row-major plan with eid_identity passes the kernels a NULL eid, dxe is zero-filled
// unless the plan proves every edge id is written, and the profile labels start with gv2edge.  A translation unit
// instantiates only its own EDGE, so only its own kernels; xe and dxe are ignored without the edge row.  Every launch
// is written once, with the edge kernel's argument list: the gv2attn_*_kernel selectors below (fast) and GO_EDGE_KERNEL
// (generic) name the kernel of this EDGE, and the arguments that only the edge kernels take (eid, xe, dxe) stand in
// arg_if<EDGE>(...), which drops them without the edge row (host_gat.h).  Not part of the C ABI.
#pragma once
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_gatv2_edge_attn.h"

namespace graphop {

// datt[p] = the sum of the row pass's n_part rows of partials, f4 pieces each: k_gv2attn_datt_fin_f32, the family's one
// kernel that is no template, defined with this launcher in gatv2_attention.hip
void gv2attn_datt_fin(const void* part, void* datt, i64 n_part, i64 f4, hipStream_t st);

#define GO_GV2_ATTN_LABELS(EDGE, pass) (EDGE ? GO_GAT_LABELS_OF("gv2edge", pass) : GO_GAT_LABELS_OF("gv2attn", pass))

// The gather passes are compiled from one text (kernels_gatv2_attn_passes.inc) per (EDGE, DROP): k_gv2attn_* and
// k_gv2drop_*, with the edge row k_gv2edge_* and k_gv2edrop_*.  The pair picks the kernel here, so that each pass is one
// launch.
template <int H, int D, bool DROP, bool EDGE>
constexpr auto gv2attn_fwd_kernel() {
  if constexpr (EDGE) {
    if constexpr (DROP) return &k_gv2edrop_fwd_f32<H, D>;
    else return &k_gv2edge_fwd_f32<H, D>;
  } else {
    if constexpr (DROP) return &k_gv2drop_fwd_f32<H, D>;
    else return &k_gv2attn_fwd_f32<H, D>;
  }
}
template <int H, int D, bool OWNED, bool DROP, bool EDGE>
constexpr auto gv2attn_bwd_row_kernel() {
  if constexpr (EDGE) {
    if constexpr (DROP) return &k_gv2edrop_bwd_row_f32<H, D, OWNED>;
    else return &k_gv2edge_bwd_row_f32<H, D, OWNED>;
  } else {
    if constexpr (DROP) return &k_gv2drop_bwd_row_f32<H, D, OWNED>;
    else return &k_gv2attn_bwd_row_f32<H, D, OWNED>;
  }
}
template <int H, int D, bool OWNED, bool DROP, bool EDGE>
constexpr auto gv2attn_bwd_col_kernel() {
  if constexpr (EDGE) {
    if constexpr (DROP) return &k_gv2edrop_bwd_col_f32<H, D, OWNED>;
    else return &k_gv2edge_bwd_col_f32<H, D, OWNED>;
  } else {
    if constexpr (DROP) return &k_gv2drop_bwd_col_f32<H, D, OWNED>;
    else return &k_gv2attn_bwd_col_f32<H, D, OWNED>;
  }
}

// drop == nullptr: the op without dropout (the DROP = false kernels, whatever the entry point)
template <bool EDGE>
int gv2attn_forward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                    const int64_t* indices, const void* xl, const void* xr, const void* xe, const void* att, void* o,
                    void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                    double negative_slope, const HostDrop* drop, const graphop_plan_t* plan, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "xl / o", n_l, "xr", n_r));
  if (n_l == 0) return GRAPHOP_OK;
  GO_PTR(fn, o); GO_PTR(fn, stats);
  // rows without chunks keep o = 0 and stats = (-1e9, 0)
  GO_HIP(zero_async(o, es * (size_t)(n_l * h * d), st));
  GO_DISPATCH_FLOAT(dtype, T, {
    hipLaunchKernelGGL((k_gv2attn_stats_init_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
  });
  GO_LAUNCH_CHECK();
  if (n_chunks == 0 || n_edges == 0 || n_r == 0) return GRAPHOP_OK;
  GO_TRY(g.require(fn));
  GO_PTR(fn, xl); GO_PTR(fn, xr);
  if constexpr (EDGE) GO_PTR(fn, xe);
  GO_PTR(fn, att);
  const bool fast = pm && pm->info.row_owned && pm->seg_chunk &&
                    gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att, o, stats}) && (!EDGE || aligned16(xe));
  const bool dropped = drop != nullptr;
  static const GatLabels lab = GO_GV2_ATTN_LABELS(EDGE, "fwd");
  if (fast) {
    const i64 S = pm->info.n_segments;
    if (S == 0) return GRAPHOP_OK;
    ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][1]);
    const int n_long = (int)pm->n_long;
    const i64 long_len = n_long > 0 ? kLongSegment : ((i64)1 << 62);
    const unsigned nbs = (unsigned)ceil_div(S, (i64)(kFastBlock / kGatGroup));
    const dim3 grid(nbs + (unsigned)n_long);
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      go_launch(gv2attn_fwd_kernel<H, D, DROP, EDGE>(), grid, dim3(kFastBlock), st, g.row,
                g.indptr, arg_if<EDGE>(g.eid_or_null()), g.indices, (const i64*)pm->seg_chunk,
                (const float*)xl, (const float*)xr, arg_if<EDGE>((const float*)xe), (const float*)att, (float*)o,
                (float2*)stats, S, nbs, long_len, (const int*)pm->long_segs, (float)negative_slope,
                drop_arg<DROP, float>(drop));
    }));
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
  ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][0]);
  const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
  GO_DISPATCH_FLOAT(dtype, T, {
    auto pass = [&](auto sum) {
      constexpr bool SUM = decltype(sum)::value;
      go_launch(GO_EDGE_KERNEL(EDGE, k_gv2attn_stats_generic, k_gv2edge_stats_generic, T, SUM), grid,
                dim3(kGenericBlock), st, g.row, g.indptr, arg_if<EDGE>(g.eid),
                g.indices, (const T*)xl, (const T*)xr, arg_if<EDGE>((const T*)xe), (const T*)att, (T*)stats,
                n_chunks, h, d, (T)negative_slope);
    };
    pass(std::false_type{});   // the maxima
    pass(std::true_type{});    // the sums of exp(s - m)
    hipLaunchKernelGGL((k_gv2attn_stats_fin_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
    GO_DISPATCH_BOOL(dropped, DROP, {
      go_launch(GO_EDGE_KERNEL(EDGE, k_gv2attn_fwd_generic, k_gv2edge_fwd_generic, T, DROP), grid, dim3(kGenericBlock),
                st, g.row, g.indptr, arg_if<EDGE>(g.eid), g.indices,
                (const T*)xl, (const T*)xr, arg_if<EDGE>((const T*)xe), (const T*)att, (const T*)stats, (T*)o, n_chunks,
                h, d, (T)negative_slope, drop_arg<DROP, T>(drop));
    });
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

template <bool EDGE>
int gv2attn_backward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c, const int64_t* eid_c,
                     const int64_t* indices_c, const void* xl, const void* xr, const void* xe, const void* att,
                     const void* o, const void* stats, const void* dO, void* dxl, void* dxr, void* dxe, void* datt,
                     void* workspace, int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                     int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope,
                     const HostDrop* drop, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const i64 f = h * d;
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || n_col_chunks > 0) && n_l > 0 && n_r > 0;
  const bool row_slots = slots && n_row_chunks > 0, col_slots = slots && n_col_chunks > 0;
  const i64 p_values = n_l * h * 4;   // P: (n_l, h, 4), then the datt partials
  const size_t need = slots ? es * (size_t)(p_values + gat_part_rows(n_row_chunks) * f) : 0;
  GO_CHECK_ARG(workspace_bytes >= 0 && (size_t)workspace_bytes >= need,
               "%s: workspace of %lld bytes needed (n_l * h * 4 + min(ceil(n_row_chunks / 16), 8192) * h * d values), "
               "got %lld", fn, (long long)need, (long long)workspace_bytes);
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const graphop_plan *pr = r.plan, *pc = c.plan;
  GO_TRY(gatv2_bwd_open(fn, dtype, r, c, dxl, dxr, datt, n_l, n_r, f, st));
  if constexpr (EDGE) {
    // edge ids that no row-major slot names get dxe = 0: skip the fill only where the plan proves every id is written
    const bool covered = row_slots && r.covered();
    if (dxe && n_edges > 0 && !covered) GO_HIP(zero_async(dxe, es * (size_t)(n_edges * f), st));
  }
  if (!slots) return GRAPHOP_OK;
  GO_PTR(fn, xl); GO_PTR(fn, xr);
  if constexpr (EDGE) GO_PTR(fn, xe);
  GO_PTR(fn, att); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  GO_PTR(fn, workspace);
  const bool ok = gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att, o, stats, dO, workspace}) &&
                  (!EDGE || (aligned16(xe) && aligned16(dxe)));
  const float slope = (float)negative_slope;
  const bool dropped = drop != nullptr;
  void* part = (char*)workspace + es * (size_t)p_values;
  {   // P[i, k] = (m, 1 / l, D, 0): the edge row is not in it
    const bool fast = ok && (pr || pc);
    ProfScope prof("gv2attn_pack", st, fast ? "k_gv2attn_pack_f32" : "k_gv2attn_pack_generic");
    if (fast) {
      GO_DISPATCH_GAT_HD(h, d, {
        hipLaunchKernelGGL((k_gv2attn_pack_f32<H, D>), dim3((unsigned)ceil_div(n_l, (i64)(kFastBlock / kGatGroup))),
                           dim3(kFastBlock), 0, st, (const float2*)stats, (const float*)dO, (const float*)o,
                           (float4*)workspace, n_l);
      });
    } else {
      GO_DISPATCH_FLOAT(dtype, T, {
        hipLaunchKernelGGL((k_gv2attn_pack_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st,
                           (const T*)stats, (const T*)dO, (const T*)o, (T*)workspace, n_l * h, d);
      });
    }
    GO_LAUNCH_CHECK();
  }
  if (row_slots) {
    GO_TRY(r.require(fn));
    GO_PTR(fn, dxl); GO_PTR(fn, datt);
    const i64 C = n_row_chunks;
    static const GatLabels lab = GO_GV2_ATTN_LABELS(EDGE, "bwd_row");
    if (ok && pr && (((uintptr_t)dxl | (uintptr_t)datt) & 15) == 0) {
      const GatRowPass geo = gat_row_pass(C, tuning().spmm_cpg);   // n_blocks <= gat_part_rows(C)
      {
        ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][1]);
        const bool owned = r.owned();
        const dim3 grid((unsigned)geo.n_blocks);
        GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
          go_launch(gv2attn_bwd_row_kernel<H, D, OWNED, DROP, EDGE>(), grid, dim3(kFastBlock), st, r.row,
                    r.indptr, arg_if<EDGE>(r.eid_or_null()), r.indices, (const float*)xl,
                    (const float*)xr, arg_if<EDGE>((const float*)xe), (const float*)att, (const float4*)workspace,
                    (const float*)dO, (float*)dxl, arg_if<EDGE>((float*)dxe), (float4*)part, C, geo.cpg, slope,
                    drop_arg<DROP, float>(drop));
        })));
        GO_LAUNCH_CHECK();
      }
      ProfScope prof("gv2attn_datt_fin", st, "k_gv2attn_datt_fin_f32");
      gv2attn_datt_fin(part, datt, geo.n_blocks, f / 4, st);
    } else {
      ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][0]);
      const dim3 grid((unsigned)ceil_div(C, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch(GO_EDGE_KERNEL(EDGE, k_gv2attn_bwd_row_generic, k_gv2edge_bwd_row_generic, T, DROP), grid,
                  dim3(kGenericBlock), st, r.row, r.indptr, arg_if<EDGE>(r.eid),
                  r.indices, (const T*)xl, (const T*)xr, arg_if<EDGE>((const T*)xe), (const T*)att,
                  (const T*)workspace, (const T*)dO, (T*)dxl, arg_if<EDGE>((T*)dxe), (T*)datt, C, h, d,
                  (T)negative_slope, drop_arg<DROP, T>(drop));
      }));
    }
    GO_LAUNCH_CHECK();
  }
  if (col_slots) {
    GO_TRY(c.require(fn));
    GO_PTR(fn, dxr);
    const i64 C = n_col_chunks;
    static const GatLabels lab = GO_GV2_ATTN_LABELS(EDGE, "bwd_col");
    if (ok && pc && ((uintptr_t)dxr & 15) == 0) {
      ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][1]);
      const int cpg = gat_cpg(C, tuning().spmm_cpg);
      const bool owned = c.owned();
      const dim3 grid((unsigned)gat_grid(C, cpg));
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
        // with the edge row the column pass always reads eid_c: no eid_or_null() here
        go_launch(gv2attn_bwd_col_kernel<H, D, OWNED, DROP, EDGE>(), grid, dim3(kFastBlock), st, c.row,
                  c.indptr, arg_if<EDGE>(c.eid), c.indices, (const float*)xl,
                  (const float*)xr, arg_if<EDGE>((const float*)xe), (const float*)att, (const float4*)workspace,
                  (const float*)dO, (float*)dxr, C, cpg, slope, drop_arg<DROP, float>(drop));
      })));
    } else {
      ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][0]);
      const dim3 grid((unsigned)ceil_div(C, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch(GO_EDGE_KERNEL(EDGE, k_gv2attn_bwd_col_generic, k_gv2edge_bwd_col_generic, T, DROP), grid,
                  dim3(kGenericBlock), st, c.row, c.indptr, arg_if<EDGE>(c.eid),
                  c.indices, (const T*)xl, (const T*)xr, arg_if<EDGE>((const T*)xe), (const T*)att,
                  (const T*)workspace, (const T*)dO, (T*)dxr, C, h, d, (T)negative_slope, drop_arg<DROP, T>(drop));
      }));
    }
    GO_LAUNCH_CHECK();
  }
  return GRAPHOP_OK;
}

}  // namespace graphop
