// Fused GAT attention (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : o[i] = sum_j softmax_j(LeakyReLU(el[i] + er[j])) V[j] per head, leaving only o and the row statistics
//   backward: del, der, dV from (el, er, V, o, stats, dO), a recomputed per slot (kernels_gat_attn.h).
// No E-sized tensor exists in either direction.  Host-side dispatch in the style of gat.hip: validation, fills, and the
// choice between the fp32 fast kernels (a plan of the same arrays, h in {1, 2, 4, 8}, d in {8, 16, 32, 64},
// h * d in {64, 128, 256}) and the generic ones (fp64, other shapes, NULL plans).
// The *_dropout_* entry points are the same op with attention dropout (kernels_dropout.h: the keep decision of an edge
// is recomputed from Philox in each gather pass, so still no E-sized tensor), and graphop_edge_dropout_mask writes that
// decision out as an (E, h) tensor for the composed path and for tests.
#include "common.h"
#include "host.h"
#include "host_dropout.h"
#include "host_gat_attn.h"
#include "kernels_gat_attn.h"

namespace graphop {
namespace {

// stats = (m, 1 / l) per (row, head); rows without slots keep (-1e9, 0)
int gat_attn_stats(int dtype, const i64* row, const i64* indptr, const i64* indices, const void* el, const void* er,
                   void* stats, i64 C, i64 n_l, i64 h, double slope, const graphop_plan* pm, bool fast,
                   hipStream_t st) {
  auto init = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((k_gat_attn_stats_init_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
  };
  if (dtype == GRAPHOP_F32) init(0.f); else init(0.0);
  GO_LAUNCH_CHECK();
  if (C == 0) return GRAPHOP_OK;
  if (fast && pm->info.row_owned && pm->seg_chunk) {
    const i64 S = pm->info.n_segments;
    if (S == 0) return GRAPHOP_OK;
    ProfScope prof("gat_attn_stats", st, "k_gat_attn_stats_f32");
    const int n_long = (int)pm->n_long;
    const i64 long_len = n_long > 0 ? kLongSegment : ((i64)1 << 62);
    const bool wide = pm->info.n_edges / S >= 64;   // long rows on average: a wave per segment
    GO_DISPATCH_GAT_ATTN_H(h, {
      {
        const int G = wide ? 64 : 16;
        const unsigned nbs = (unsigned)ceil_div(S, kFastBlock / G);
        const dim3 grid(nbs + (unsigned)n_long);
        if (wide)
          hipLaunchKernelGGL((k_gat_attn_stats_f32<H, 64>), grid, dim3(kFastBlock), 0, st, row, indptr, indices,
                             (const i64*)pm->seg_chunk, (const float*)el, (const float*)er, (float2*)stats, S, nbs,
                             long_len, (const int*)pm->long_segs, (float)slope);
        else
          hipLaunchKernelGGL((k_gat_attn_stats_f32<H, 16>), grid, dim3(kFastBlock), 0, st, row, indptr, indices,
                             (const i64*)pm->seg_chunk, (const float*)el, (const float*)er, (float2*)stats, S, nbs,
                             long_len, (const int*)pm->long_segs, (float)slope);
      }
    });
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
  ProfScope prof("gat_attn_stats", st, "k_gat_attn_stats_generic");
  const unsigned nb = (unsigned)ceil_div(C, kGenericWavesPerBlock);
  auto go = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((k_gat_attn_stats_generic<T, false>), dim3(nb), dim3(kGenericBlock), 0, st, row, indptr,
                       indices, (const T*)el, (const T*)er, (T*)stats, C, h, (T)slope);
    hipLaunchKernelGGL((k_gat_attn_stats_generic<T, true>), dim3(nb), dim3(kGenericBlock), 0, st, row, indptr,
                       indices, (const T*)el, (const T*)er, (T*)stats, C, h, (T)slope);
    hipLaunchKernelGGL((k_gat_attn_stats_fin_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (T*)stats,
                       n_l * h);
  };
  if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace
}  // namespace graphop

using namespace graphop;

namespace {

// drop == nullptr: the op without dropout (the DROP = false kernels, whatever the entry point)
int gat_attn_forward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                     const int64_t* indices, const void* el, const void* er, const void* V, void* o, void* stats,
                     int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                     double negative_slope, const HostDrop* drop, const graphop_plan_t* plan, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const graphop_plan* pm = plan_matches_full(plan, (const i64*)row, (const i64*)indptr, (const i64*)eid,
                                             (const i64*)indices, n_chunks, n_edges) ? plan : nullptr;
  GO_TRY(gat_attn_check_plan(fn, pm, "el / o", n_l, "er / V", n_r));
  if (n_l == 0) return GRAPHOP_OK;
  GO_PTR(fn, o); GO_PTR(fn, stats);
  GO_HIP(zero_async(o, es * (size_t)(n_l * h * d), st));
  const bool slots = n_chunks > 0 && n_edges > 0;
  if (slots) {
    GO_PTR(fn, row); GO_PTR(fn, indptr); GO_PTR(fn, eid); GO_PTR(fn, indices);
    GO_PTR(fn, el); GO_PTR(fn, er); GO_PTR(fn, V);
  }
  const bool fast = pm && gat_attn_fast_ok(dtype, h, d, n_edges, n_l, n_r, {el, er, V, o, stats});
  GO_TRY(gat_attn_stats(dtype, (const i64*)row, (const i64*)indptr, (const i64*)indices, el, er, stats,
                        slots ? n_chunks : 0, n_l, h, negative_slope, pm, fast, st));
  if (!slots) return GRAPHOP_OK;
  const bool dropped = drop != nullptr;
  static const GatAttnLabels lab = GO_GAT_ATTN_LABELS("fwd");
  ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][fast]);
  if (fast) {
    const int cpg = gat_attn_cpg(n_chunks);
    const bool owned = pm->info.rows_sorted != 0;
    GO_DISPATCH_GAT_ATTN(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_gat_attn_fwd_f32<H, D, OWNED, DROP>), dim3(gat_attn_grid(n_chunks, cpg)),
                         dim3(kFastBlock), 0, st, (const i64*)row, (const i64*)indptr, (const i64*)indices,
                         (const float*)el, (const float*)er, (const float2*)stats, (const float*)V, (float*)o,
                         n_chunks, cpg, (float)negative_slope, drop_arg<DROP, float>(drop));
    })));
  } else {
    auto go = [&](auto zero) {
      using T = decltype(zero);
      GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((k_gat_attn_fwd_generic<T, DROP>), dim3((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock)),
                           dim3(kGenericBlock), 0, st, (const i64*)row, (const i64*)indptr, (const i64*)indices,
                           (const T*)el, (const T*)er, (const T*)stats, (const T*)V, (T*)o, n_chunks, h, d,
                           (T)negative_slope, drop_arg<DROP, T>(drop));
      });
    };
    if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int gat_attn_backward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                      const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c, const int64_t* eid_c,
                      const int64_t* indices_c, const void* el, const void* er, const void* V, const void* o,
                      const void* stats, const void* dO, void* del, void* der, void* dV, void* workspace,
                      int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges,
                      int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope, const HostDrop* drop,
                      const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || n_col_chunks > 0);
  const size_t need = slots ? es * 4 * (size_t)(n_l * h) : 0;   // P: (n_l, h, 4)
  GO_CHECK_ARG(workspace_bytes >= 0 && (size_t)workspace_bytes >= need,
               "%s: workspace of %lld bytes needed (n_l * h * 4 values), got %lld", fn, (long long)need,
               (long long)workspace_bytes);
  const graphop_plan* pr = plan_matches_full(plan_r, (const i64*)row, (const i64*)indptr_r, (const i64*)eid_r,
                                             (const i64*)indices_r, n_row_chunks, n_edges) ? plan_r : nullptr;
  const graphop_plan* pc = plan_matches_full(plan_c, (const i64*)col, (const i64*)indptr_c, (const i64*)eid_c,
                                             (const i64*)indices_c, n_col_chunks, n_edges) ? plan_c : nullptr;
  GO_TRY(gat_attn_check_plan(fn, pr, "el / del", n_l, "er / V", n_r));
  GO_TRY(gat_attn_check_plan(fn, pc, "er / der", n_r, "el", n_l));
  if (n_l > 0 && !(del == nullptr && n_row_chunks == 0)) {
    GO_PTR(fn, del);
    GO_HIP(zero_async(del, es * (size_t)(n_l * h), st));
  }
  if (n_r > 0 && !(der == nullptr && dV == nullptr && n_col_chunks == 0)) {
    GO_PTR(fn, der); GO_PTR(fn, dV);
    GO_HIP(zero_async(der, es * (size_t)(n_r * h), st));
    GO_HIP(zero_async(dV, es * (size_t)(n_r * h * d), st));
  }
  if (!slots || n_l == 0 || n_r == 0) return GRAPHOP_OK;
  GO_PTR(fn, el); GO_PTR(fn, er); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  GO_PTR(fn, workspace);
  const bool ok = gat_attn_fast_ok(dtype, h, d, n_edges, n_l, n_r, {el, er, V, o, stats, dO, workspace, dV});
  const float slope = (float)negative_slope;
  const bool dropped = drop != nullptr;
  const int G = 16;
  {   // P[i, k] = (el, m, 1/l, D)
    const bool fast = ok && (pr || pc);
    ProfScope prof("gat_attn_pack", st, fast ? "k_gat_attn_pack_f32" : "k_gat_attn_pack_generic");
    if (fast) {
      GO_DISPATCH_GAT_ATTN(h, d, {
        hipLaunchKernelGGL((k_gat_attn_pack_f32<H, D>), dim3((unsigned)ceil_div(n_l, kFastBlock / G)),
                           dim3(kFastBlock), 0, st, (const float*)el, (const float2*)stats, (const float*)dO,
                           (const float*)o, (float4*)workspace, n_l);
      });
    } else {
      auto go = [&](auto zero) {
        using T = decltype(zero);
        hipLaunchKernelGGL((k_gat_attn_pack_generic<T>), dim3(grid_of(n_l * h)), dim3(256), 0, st, (const T*)el,
                           (const T*)stats, (const T*)dO, (const T*)o, (T*)workspace, n_l * h, d);
      };
      if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
    }
    GO_LAUNCH_CHECK();
  }
  if (n_row_chunks > 0) {
    GO_PTR(fn, row); GO_PTR(fn, indptr_r); GO_PTR(fn, eid_r); GO_PTR(fn, indices_r);
    const i64 C = n_row_chunks;
    const bool fast = ok && pr;
    static const GatAttnLabels lab = GO_GAT_ATTN_LABELS("bwd_row");
    ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][fast]);
    if (fast) {
      const int cpg = gat_attn_cpg(C);
      const bool owned = pr->info.rows_sorted != 0;
      GO_DISPATCH_GAT_ATTN(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((k_gat_attn_bwd_row_f32<H, D, OWNED, DROP>), dim3(gat_attn_grid(C, cpg)), dim3(kFastBlock),
                           0, st, (const i64*)row, (const i64*)indptr_r, (const i64*)indices_r, (const float*)er,
                           (const float*)V, (const float4*)workspace, (const float*)dO, (float*)del, C, cpg, slope,
                           drop_arg<DROP, float>(drop));
      })));
    } else {
      auto go = [&](auto zero) {
        using T = decltype(zero);
        GO_DISPATCH_BOOL(dropped, DROP, {
          hipLaunchKernelGGL((k_gat_attn_bwd_row_generic<T, DROP>), dim3((unsigned)ceil_div(C, kGenericWavesPerBlock)),
                             dim3(kGenericBlock), 0, st, (const i64*)row, (const i64*)indptr_r, (const i64*)indices_r,
                             (const T*)er, (const T*)V, (const T*)workspace, (const T*)dO, (T*)del, C, h, d,
                             (T)negative_slope, drop_arg<DROP, T>(drop));
        });
      };
      if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
    }
    GO_LAUNCH_CHECK();
  }
  if (n_col_chunks > 0) {
    GO_PTR(fn, col); GO_PTR(fn, indptr_c); GO_PTR(fn, eid_c); GO_PTR(fn, indices_c);
    const i64 C = n_col_chunks;
    const bool fast = ok && pc;
    static const GatAttnLabels lab = GO_GAT_ATTN_LABELS("bwd_col");
    ProfScope prof(lab.tag[dropped], st, lab.kernel[dropped][fast]);
    if (fast) {
      const int cpg = gat_attn_cpg(C);
      const bool owned = pc->info.rows_sorted != 0;
      GO_DISPATCH_GAT_ATTN(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((k_gat_attn_bwd_col_f32<H, D, OWNED, DROP>), dim3(gat_attn_grid(C, cpg)), dim3(kFastBlock),
                           0, st, (const i64*)col, (const i64*)indptr_c, (const i64*)indices_c, (const float*)er,
                           (const float*)V, (const float4*)workspace, (const float*)dO, (float*)der, (float*)dV, C,
                           cpg, slope, drop_arg<DROP, float>(drop));
      })));
    } else {
      auto go = [&](auto zero) {
        using T = decltype(zero);
        GO_DISPATCH_BOOL(dropped, DROP, {
          hipLaunchKernelGGL((k_gat_attn_bwd_col_generic<T, DROP>), dim3((unsigned)ceil_div(C, kGenericWavesPerBlock)),
                             dim3(kGenericBlock), 0, st, (const i64*)col, (const i64*)indptr_c, (const i64*)indices_c,
                             (const T*)er, (const T*)V, (const T*)workspace, (const T*)dO, (T*)der, (T*)dV, C, h, d,
                             (T)negative_slope, drop_arg<DROP, T>(drop));
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

int graphop_gat_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                  const int64_t* indices, const void* el, const void* er, const void* V, void* o,
                                  void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                  int64_t h, int64_t d, double negative_slope, const graphop_plan_t* plan,
                                  void* stream) {
  const char* fn = "gat_attention_forward";
  GO_TRY(gat_attn_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  return gat_attn_forward(fn, dtype, row, indptr, eid, indices, el, er, V, o, stats, n_chunks, n_edges, n_l, n_r, h, d,
                          negative_slope, nullptr, plan, stream);
}

int graphop_gat_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                   const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                   const int64_t* eid_c, const int64_t* indices_c, const void* el, const void* er,
                                   const void* V, const void* o, const void* stats, const void* dO, void* del,
                                   void* der, void* dV, void* workspace, int64_t workspace_bytes,
                                   int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                   int64_t n_r, int64_t h, int64_t d, double negative_slope,
                                   const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gat_attention_backward";
  GO_TRY(gat_attn_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  return gat_attn_backward(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o,
                           stats, dO, del, der, dV, workspace, workspace_bytes, n_row_chunks, n_col_chunks, n_edges,
                           n_l, n_r, h, d, negative_slope, nullptr, plan_r, plan_c, stream);
}

// p == 0 runs the kernels of the entry points above: bit-identical results
int graphop_gat_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                          const int64_t* indices, const void* el, const void* er, const void* V,
                                          void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                          int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                          uint64_t seed, uint32_t offset, const graphop_plan_t* plan, void* stream) {
  const char* fn = "gat_attention_dropout_forward";
  GO_TRY(gat_attn_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gat_attn_forward(fn, dtype, row, indptr, eid, indices, el, er, V, o, stats, n_chunks, n_edges, n_l, n_r, h, d,
                          negative_slope, p > 0.0 ? &drop : nullptr, plan, stream);
}

int graphop_gat_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                           const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                           const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                           const void* el, const void* er, const void* V, const void* o,
                                           const void* stats, const void* dO, void* del, void* der, void* dV,
                                           void* workspace, int64_t workspace_bytes, int64_t n_row_chunks,
                                           int64_t n_col_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h,
                                           int64_t d, double negative_slope, double p, uint64_t seed, uint32_t offset,
                                           const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gat_attention_dropout_backward";
  GO_TRY(gat_attn_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gat_attn_backward(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, V, o,
                           stats, dO, del, der, dV, workspace, workspace_bytes, n_row_chunks, n_col_chunks, n_edges,
                           n_l, n_r, h, d, negative_slope, p > 0.0 ? &drop : nullptr, plan_r, plan_c, stream);
}

int graphop_edge_dropout_mask(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, void* y, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                              int64_t n_r, int64_t h, double p, uint64_t seed, uint32_t offset,
                              const graphop_plan_t* plan, void* stream) {
  const char* fn = "edge_dropout_mask";
  GO_TRY(gat_attn_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, 1));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  hipStream_t st = (hipStream_t)stream;
  if (n_edges == 0) return GRAPHOP_OK;
  GO_PTR(fn, y);
  const graphop_plan* pm = plan_matches_full(plan, (const i64*)row, (const i64*)indptr, (const i64*)eid,
                                             (const i64*)indices, n_chunks, n_edges) ? plan : nullptr;
  GO_TRY(gat_attn_check_plan(fn, pm, "the row-major rows", n_l, "the neighbours", n_r));
  const bool covered = pm && pm->info.full_coverage && pm->info.eid_identity && pm->info.indptr_monotone;
  if (!covered) GO_HIP(zero_async(y, esize(dtype) * (size_t)(n_edges * h), st));   // edges no slot names get m = 0
  if (n_chunks == 0) return GRAPHOP_OK;
  GO_PTR(fn, row); GO_PTR(fn, indptr); GO_PTR(fn, eid); GO_PTR(fn, indices);
  ProfScope prof("edge_dropout_mask", st, "k_edge_dropout_mask");
  const unsigned nb = (unsigned)ceil_div(n_chunks, kGenericWavesPerBlock);
  auto go = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((k_edge_dropout_mask<T>), dim3(nb), dim3(kGenericBlock), 0, st, (const i64*)row,
                       (const i64*)indptr, (const i64*)eid, (const i64*)indices, (T*)y, n_chunks, h, drop.as<T>());
  };
  if (dtype == GRAPHOP_F32) go(0.f); else go(0.0);
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // extern "C"
