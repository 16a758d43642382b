// Attention weights of the fused GAT and GATv2 layers (extra ops, not among the reference's eight;
// include/graphop_hip.h): a[e, k] = exp(min(s_e - m_i, 0)) * linv_i from the row statistics the fused
// forward left, with the layer's own score s_e (with or without its edge operand ee / xe).
//   GAT  : k_gatw_f32 (fp32, h in {1, 2, 4, 8}, a matching plan, operands aligned to their item width), else
//          k_gatw_generic
//   GATv2: k_gv2w_f32 (fp32, the (h, d) pairs of GO_DISPATCH_GAT_HD, a matching plan, 16-byte aligned operands), else
//          k_gv2w_generic
// Host-side dispatch only: the checks, the dispatch macros and the launch geometry are the family's (host_gat.h).  No
// workspace and no atomics; a[e] is written once for every edge id a slot names and nothing else of a is touched.
#include "common.h"
#include "host.h"
#include "host_gat.h"
#include "kernels_gat_weights.h"

using namespace graphop;

extern "C" {

int graphop_gat_attention_weights(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                  const int64_t* indices, const void* el, const void* er, const void* ee,
                                  const void* stats, void* a, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                  int64_t n_r, int64_t h, double negative_slope, const graphop_plan_t* plan,
                                  void* stream) {
  const char* fn = "gat_attention_weights";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h));
  const bool slots = n_chunks > 0 && n_edges > 0 && n_l > 0 && n_r > 0;
  if (slots) { GO_PTR(fn, stats); GO_PTR(fn, a); }
  hipStream_t st = (hipStream_t)stream;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "el / stats", n_l, "er", n_r));
  if (!slots) return GRAPHOP_OK;   // nothing is written, nothing dereferenced
  GO_TRY(g.require(fn)); GO_PTR(fn, el); GO_PTR(fn, er);
  const bool edge = ee != nullptr;
  if (pm && gat_h_fast_ok(dtype, h, n_edges, n_l, n_r, {el, er, ee, a}, stats)) {
    ProfScope prof("gat_weights", st, "k_gatw_f32");
    GO_DISPATCH_GAT_ATTN_H(h, GO_DISPATCH_BOOL(edge, EDGE, {
      constexpr int G = GatCfg<H>::G;
      const int cpg = gat_cpg(n_chunks, tuning().sddmm_cpg, G);
      go_launch(&k_gatw_f32<H, EDGE>, dim3((unsigned)gat_grid(n_chunks, cpg, G)), dim3(kFastBlock), st, g.row, g.indptr,
                g.eid_or_null(), g.indices, (const float*)el, (const float*)er, (const float*)ee, (const float2*)stats,
                (float*)a, n_chunks, cpg, (float)negative_slope);
    }));
  } else {
    ProfScope prof("gat_weights_generic", st, "k_gatw_generic");
    const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
    GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(edge, EDGE, {
      go_launch(&k_gatw_generic<T, EDGE>, grid, dim3(kGenericBlock), st, g.row, g.indptr, g.eid, g.indices,
                (const T*)el, (const T*)er, (const T*)ee, (const T*)stats, (T*)a, n_chunks, (i64)h,
                (T)negative_slope);
    }));
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_gatv2_attention_weights(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* xl, const void* xr, const void* xe,
                                    const void* att, const void* stats, void* a, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope,
                                    const graphop_plan_t* plan, void* stream) {
  const char* fn = "gatv2_attention_weights";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  const bool slots = n_chunks > 0 && n_edges > 0 && n_l > 0 && n_r > 0;
  if (slots) { GO_PTR(fn, stats); GO_PTR(fn, a); }
  hipStream_t st = (hipStream_t)stream;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "xl / stats", n_l, "xr", n_r));
  if (!slots) return GRAPHOP_OK;   // nothing is written, nothing dereferenced
  GO_TRY(g.require(fn)); GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att);
  const bool edge = xe != nullptr;
  if (pm && gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, xe, att, stats, a})) {
    ProfScope prof("gatv2_weights", st, "k_gv2w_f32");
    const int cpg = gat_cpg(n_chunks, tuning().sddmm_cpg);
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(edge, EDGE, {
      go_launch(&k_gv2w_f32<H, D, EDGE>, dim3((unsigned)gat_grid(n_chunks, cpg)), dim3(kFastBlock), st, g.row, g.indptr,
                g.eid_or_null(), g.indices, (const float*)xl, (const float*)xr, (const float*)xe, (const float*)att,
                (const float*)stats, (float*)a, n_chunks, cpg, (float)negative_slope);
    }));
  } else {
    ProfScope prof("gatv2_weights_generic", st, "k_gv2w_generic");
    const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
    GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(edge, EDGE, {
      go_launch(&k_gv2w_generic<T, EDGE>, grid, dim3(kGenericBlock), st, g.row, g.indptr, g.eid, g.indices,
                (const T*)xl, (const T*)xr, (const T*)xe, (const T*)att, (const T*)stats, (T*)a, n_chunks, (i64)h,
                (i64)d, (T)negative_slope);
    }));
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // extern "C"
