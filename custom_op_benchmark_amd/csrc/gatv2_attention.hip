// Fused GATv2 attention (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : o[i] = sum_j softmax_j(att . LeakyReLU(xl[i] + xr[j])) xr[j] per head, leaving only o and the row statistics
//   backward: dxl, dxr, datt from (xl, xr, att, o, stats, dO), z, s and a recomputed per slot (kernels_gatv2_attn.h).
// No E-sized tensor exists in either direction.  Host-side dispatch in the style of gatv2.hip and gat_attention.hip:
// validation, fills, and the choice between the fp32 fast kernels (a plan of the same arrays, the (h, d) pairs of the
// fused GAT layer, ids below 2^31, 16-byte-aligned tables) and the generic ones (fp64, other shapes, NULL plans; the
// forward also where the plan is not row_owned).  Checks, fast conditions, dispatch and launch geometry: host_gat.h.
// The *_dropout_* entry points are the same op with attention dropout (kernels_dropout.h: the keep decision of an edge
// is recomputed from Philox in each gather pass, so still no E-sized tensor); p == 0 is the op without it.
#include "common.h"
#include "host.h"
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_gatv2_attn.h"

using namespace graphop;

namespace {

// The gather passes are compiled twice from one text (kernels_gatv2_attn_passes.inc): k_gv2drop_* with dropout,
// k_gv2attn_* without.  DROP picks the kernel here, so that each pass is one launch.
template <int H, int D, bool DROP>
constexpr auto gv2attn_fwd_kernel() {
  if constexpr (DROP) return &k_gv2drop_fwd_f32<H, D>;
  else return &k_gv2attn_fwd_f32<H, D>;
}
template <int H, int D, bool OWNED, bool DROP>
constexpr auto gv2attn_bwd_row_kernel() {
  if constexpr (DROP) return &k_gv2drop_bwd_row_f32<H, D, OWNED>;
  else return &k_gv2attn_bwd_row_f32<H, D, OWNED>;
}
template <int H, int D, bool OWNED, bool DROP>
constexpr auto gv2attn_bwd_col_kernel() {
  if constexpr (DROP) return &k_gv2drop_bwd_col_f32<H, D, OWNED>;
  else return &k_gv2attn_bwd_col_f32<H, D, OWNED>;
}

// drop == nullptr: the op without dropout (the DROP = false kernels, whatever the entry point)
int gv2attn_forward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                    const int64_t* indices, const void* xl, const void* xr, const void* att, void* o, void* stats,
                    int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                    double negative_slope, const HostDrop* drop, const graphop_plan_t* plan, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const graphop_plan* pm = plan_matches_full(plan, (const i64*)row, (const i64*)indptr, (const i64*)eid,
                                             (const i64*)indices, n_chunks, n_edges) ? plan : nullptr;
  GO_TRY(gat_check_plan(fn, pm, "xl / o", n_l, "xr", n_r));
  if (n_l == 0) return GRAPHOP_OK;
  GO_PTR(fn, o); GO_PTR(fn, stats);
  // rows without chunks keep o = 0 and stats = (-1e9, 0)
  GO_HIP(zero_async(o, es * (size_t)(n_l * h * d), st));
  auto init = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((k_gv2attn_stats_init_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
  };
  if (dtype == GRAPHOP_F32) init(0.f); else init(0.0);
  GO_LAUNCH_CHECK();
  if (n_chunks == 0 || n_edges == 0 || n_r == 0) return GRAPHOP_OK;
  GO_PTR(fn, row); GO_PTR(fn, indptr); GO_PTR(fn, eid); GO_PTR(fn, indices);
  GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att);
  const bool fast = pm && pm->info.row_owned && pm->seg_chunk &&
                    gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att, o, stats});
  const bool dropped = drop != nullptr;
  static const GatLabels lab = GO_GAT_LABELS_OF("gv2attn", "fwd");
  if (fast) {
    const i64 S = pm->info.n_segments;
    if (S == 0) return GRAPHOP_OK;
    ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][1]);
    const int n_long = (int)pm->n_long;
    const i64 long_len = n_long > 0 ? kLongSegment : ((i64)1 << 62);
    const unsigned nbs = (unsigned)ceil_div(S, (i64)(kFastBlock / kGatGroup));
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((gv2attn_fwd_kernel<H, D, DROP>()), dim3(nbs + (unsigned)n_long), dim3(kFastBlock), 0, st,
                         (const i64*)row, (const i64*)indptr, (const i64*)indices, (const i64*)pm->seg_chunk,
                         (const float*)xl, (const float*)xr, (const float*)att, (float*)o, (float2*)stats, S, nbs,
                         long_len, (const int*)pm->long_segs, (float)negative_slope, drop_arg<DROP, float>(drop));
    }));
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
  ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][0]);
  const unsigned nb = (unsigned)ceil_div(n_chunks, kGenericWavesPerBlock);
  auto go = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((k_gv2attn_stats_generic<T, false>), dim3(nb), dim3(kGenericBlock), 0, st, (const i64*)row,
                       (const i64*)indptr, (const i64*)indices, (const T*)xl, (const T*)xr, (const T*)att, (T*)stats,
                       n_chunks, h, d, (T)negative_slope);
    hipLaunchKernelGGL((k_gv2attn_stats_generic<T, true>), dim3(nb), dim3(kGenericBlock), 0, st, (const i64*)row,
                       (const i64*)indptr, (const i64*)indices, (const T*)xl, (const T*)xr, (const T*)att, (T*)stats,
                       n_chunks, h, d, (T)negative_slope);
    hipLaunchKernelGGL((k_gv2attn_stats_fin_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
    GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_gv2attn_fwd_generic<T, DROP>), dim3(nb), dim3(kGenericBlock), 0, st, (const i64*)row,
                         (const i64*)indptr, (const i64*)indices, (const T*)xl, (const T*)xr, (const T*)att,
                         (const T*)stats, (T*)o, n_chunks, h, d, (T)negative_slope, drop_arg<DROP, T>(drop));
    });
  };
  if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int gv2attn_backward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c, const int64_t* eid_c,
                     const int64_t* indices_c, const void* xl, const void* xr, const void* att, const void* o,
                     const void* stats, const void* dO, void* dxl, void* dxr, void* datt, void* workspace,
                     int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                     int64_t n_r, int64_t h, int64_t d, double negative_slope, const HostDrop* drop,
                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
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
  const graphop_plan *pr, *pc;
  GO_TRY(gatv2_bwd_open(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, dxl, dxr, datt,
                        n_row_chunks, n_col_chunks, n_edges, n_l, n_r, f, plan_r, plan_c, st, &pr, &pc));
  if (!slots) return GRAPHOP_OK;
  GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  GO_PTR(fn, workspace);
  const bool ok = gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att, o, stats, dO, workspace});
  const float slope = (float)negative_slope;
  const bool dropped = drop != nullptr;
  void* part = (char*)workspace + es * (size_t)p_values;
  {   // P[i, k] = (m, 1 / l, D, 0)
    const bool fast = ok && (pr || pc);
    ProfScope prof("gv2attn_pack", st, fast ? "k_gv2attn_pack_f32" : "k_gv2attn_pack_generic");
    if (fast) {
      GO_DISPATCH_GAT_HD(h, d, {
        hipLaunchKernelGGL((k_gv2attn_pack_f32<H, D>), dim3((unsigned)ceil_div(n_l, (i64)(kFastBlock / kGatGroup))),
                           dim3(kFastBlock), 0, st, (const float2*)stats, (const float*)dO, (const float*)o,
                           (float4*)workspace, n_l);
      });
    } else {
      auto go = [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL((k_gv2attn_pack_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st,
                           (const T*)stats, (const T*)dO, (const T*)o, (T*)workspace, n_l * h, d);
      };
      if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
    }
    GO_LAUNCH_CHECK();
  }
  if (row_slots) {
    GO_PTR(fn, row); GO_PTR(fn, indptr_r); GO_PTR(fn, eid_r); GO_PTR(fn, indices_r);
    GO_PTR(fn, dxl); GO_PTR(fn, datt);
    const i64 C = n_row_chunks;
    if (ok && pr && (((uintptr_t)dxl | (uintptr_t)datt) & 15) == 0) {
      const GatRowPass geo = gat_row_pass(C, tuning().spmm_cpg);   // n_blocks <= gat_part_rows(C)
      {
        static const GatLabels lab = GO_GAT_LABELS_OF("gv2attn", "bwd_row");
        ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][1]);
        const bool owned = pr->info.rows_sorted != 0;
        GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
          hipLaunchKernelGGL((gv2attn_bwd_row_kernel<H, D, OWNED, DROP>()), dim3((unsigned)geo.n_blocks),
                             dim3(kFastBlock), 0, st, (const i64*)row, (const i64*)indptr_r, (const i64*)indices_r,
                             (const float*)xl, (const float*)xr, (const float*)att, (const float4*)workspace,
                             (const float*)dO, (float*)dxl, (float4*)part, C, geo.cpg, slope,
                             drop_arg<DROP, float>(drop));
        })));
        GO_LAUNCH_CHECK();
      }
      ProfScope prof("gv2attn_datt_fin", st, "k_gv2attn_datt_fin_f32");
      hipLaunchKernelGGL(k_gv2attn_datt_fin_f32, dim3((unsigned)(f / 4)), dim3(kFastBlock), 0, st,
                         (const float4*)part, (float4*)datt, geo.n_blocks, (int)(f / 4));
    } else {
      static const GatLabels lab = GO_GAT_LABELS_OF("gv2attn", "bwd_row");
      ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][0]);
      const unsigned nb = (unsigned)ceil_div(C, kGenericWavesPerBlock);
      auto go = [&](auto zero) {
        using T = decltype(zero);
        GO_DISPATCH_BOOL(dropped, DROP, {
          hipLaunchKernelGGL((k_gv2attn_bwd_row_generic<T, DROP>), dim3(nb), dim3(kGenericBlock), 0, st,
                             (const i64*)row, (const i64*)indptr_r, (const i64*)indices_r, (const T*)xl, (const T*)xr,
                             (const T*)att, (const T*)workspace, (const T*)dO, (T*)dxl, (T*)datt, C, h, d,
                             (T)negative_slope, drop_arg<DROP, T>(drop));
        });
      };
      if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
    }
    GO_LAUNCH_CHECK();
  }
  if (col_slots) {
    GO_PTR(fn, col); GO_PTR(fn, indptr_c); GO_PTR(fn, eid_c); GO_PTR(fn, indices_c);
    GO_PTR(fn, dxr);
    const i64 C = n_col_chunks;
    static const GatLabels lab = GO_GAT_LABELS_OF("gv2attn", "bwd_col");
    if (ok && pc && ((uintptr_t)dxr & 15) == 0) {
      ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][1]);
      const int cpg = gat_cpg(C, tuning().spmm_cpg);
      const bool owned = pc->info.rows_sorted != 0;
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((gv2attn_bwd_col_kernel<H, D, OWNED, DROP>()), dim3((unsigned)gat_grid(C, cpg)),
                           dim3(kFastBlock), 0, st, (const i64*)col, (const i64*)indptr_c, (const i64*)indices_c,
                           (const float*)xl, (const float*)xr, (const float*)att, (const float4*)workspace,
                           (const float*)dO, (float*)dxr, C, cpg, slope, drop_arg<DROP, float>(drop));
      })));
    } else {
      ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][0]);
      const unsigned nb = (unsigned)ceil_div(C, kGenericWavesPerBlock);
      auto go = [&](auto zero) {
        using T = decltype(zero);
        GO_DISPATCH_BOOL(dropped, DROP, {
          hipLaunchKernelGGL((k_gv2attn_bwd_col_generic<T, DROP>), dim3(nb), dim3(kGenericBlock), 0, st,
                             (const i64*)col, (const i64*)indptr_c, (const i64*)indices_c, (const T*)xl, (const T*)xr,
                             (const T*)att, (const T*)workspace, (const T*)dO, (T*)dxr, C, h, d, (T)negative_slope,
                             drop_arg<DROP, T>(drop));
        });
      };
      if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
    }
    GO_LAUNCH_CHECK();
  }
  return GRAPHOP_OK;
}

}  // namespace

extern "C" {

int graphop_gatv2_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* xl, const void* xr, const void* att, void* o,
                                    void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                    int64_t h, int64_t d, double negative_slope, const graphop_plan_t* plan,
                                    void* stream) {
  const char* fn = "gatv2_attention_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  return gv2attn_forward(fn, dtype, row, indptr, eid, indices, xl, xr, att, o, stats, n_chunks, n_edges, n_l, n_r, h, d,
                         negative_slope, nullptr, plan, stream);
}

int graphop_gatv2_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* xl, const void* xr,
                                     const void* att, const void* o, const void* stats, const void* dO, void* dxl,
                                     void* dxr, void* datt, void* workspace, int64_t workspace_bytes,
                                     int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                     int64_t n_r, int64_t h, int64_t d, double negative_slope,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gatv2_attention_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  return gv2attn_backward(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o,
                          stats, dO, dxl, dxr, datt, workspace, workspace_bytes, n_row_chunks, n_col_chunks, n_edges,
                          n_l, n_r, h, d, negative_slope, nullptr, plan_r, plan_c, stream);
}

// p == 0 runs the kernels of the entry points above: bit-identical results
int graphop_gatv2_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                            const int64_t* indices, const void* xl, const void* xr, const void* att,
                                            void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                            int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                            uint64_t seed, uint32_t offset, const graphop_plan_t* plan, void* stream) {
  const char* fn = "gatv2_attention_dropout_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gv2attn_forward(fn, dtype, row, indptr, eid, indices, xl, xr, att, o, stats, n_chunks, n_edges, n_l, n_r, h, d,
                         negative_slope, p > 0.0 ? &drop : nullptr, plan, stream);
}

int graphop_gatv2_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                             const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                             const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                             const void* xl, const void* xr, const void* att, const void* o,
                                             const void* stats, const void* dO, void* dxl, void* dxr, void* datt,
                                             void* workspace, int64_t workspace_bytes, int64_t n_row_chunks,
                                             int64_t n_col_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                             int64_t h, int64_t d, double negative_slope, double p, uint64_t seed,
                                             uint32_t offset, const graphop_plan_t* plan_r,
                                             const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gatv2_attention_dropout_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gv2attn_backward(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, att, o,
                          stats, dO, dxl, dxr, datt, workspace, workspace_bytes, n_row_chunks, n_col_chunks, n_edges,
                          n_l, n_r, h, d, negative_slope, p > 0.0 ? &drop : nullptr, plan_r, plan_c, stream);
}

}  // extern "C"
