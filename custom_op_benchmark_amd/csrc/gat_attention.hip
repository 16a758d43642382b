// Fused GAT attention (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : o[i] = sum_j softmax_j(LeakyReLU(el[i] + er[j])) V[j] per head, leaving only o and the row statistics
//   backward: del, der, dV from (el, er, V, o, stats, dO), a recomputed per slot (kernels_gat_attn.h).
// No E-sized tensor exists in either direction.  Host-side dispatch in the style of gat.hip: validation, fills, and the
// choice between the fp32 fast kernels (a plan of the same arrays, h in {1, 2, 4, 8}, d in {8, 16, 32, 64},
// h * d in {64, 128, 256}) and the generic ones (fp64, other shapes, NULL plans).
// The *_dropout_* entry points are the same op with attention dropout (kernels_dropout.h: the keep decision of an edge
// is recomputed from Philox in each gather pass, so still no E-sized tensor), and graphop_edge_dropout_mask writes that
// decision out as an (E, h) tensor for the composed path and for tests.
// Stats, forward and backward are host_gat_attn_ops.h without the edge term (EDGE = false; ee and dee are NULL).
#include "common.h"
#include "host.h"
#include "host_gat_attn_ops.h"

using namespace graphop;

extern "C" {

int graphop_gat_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                  const int64_t* indices, const void* el, const void* er, const void* V, void* o,
                                  void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                  int64_t h, int64_t d, double negative_slope, const graphop_plan_t* plan,
                                  void* stream) {
  const char* fn = "gat_attention_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  return gat_attn_forward<false>(fn, dtype, row, indptr, eid, indices, el, er, nullptr, V, o, stats, n_chunks, n_edges,
                                 n_l, n_r, h, d, negative_slope, nullptr, plan, stream);
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
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  return gat_attn_backward<false>(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er,
                                  nullptr, V, o, stats, dO, del, der, nullptr, dV, workspace, workspace_bytes,
                                  n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d, negative_slope,
                                  nullptr, plan_r, plan_c, stream);
}

// p == 0 runs the kernels of the entry points above: bit-identical results
int graphop_gat_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                          const int64_t* indices, const void* el, const void* er, const void* V,
                                          void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                          int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                          uint64_t seed, uint32_t offset, const graphop_plan_t* plan, void* stream) {
  const char* fn = "gat_attention_dropout_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gat_attn_forward<false>(fn, dtype, row, indptr, eid, indices, el, er, nullptr, V, o, stats, n_chunks, n_edges,
                                 n_l, n_r, h, d, negative_slope, p > 0.0 ? &drop : nullptr, plan, stream);
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
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gat_attn_backward<false>(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er,
                                  nullptr, V, o, stats, dO, del, der, nullptr, dV, workspace, workspace_bytes,
                                  n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d, negative_slope,
                                  p > 0.0 ? &drop : nullptr, plan_r, plan_c, stream);
}

int graphop_edge_dropout_mask(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, void* y, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                              int64_t n_r, int64_t h, double p, uint64_t seed, uint32_t offset,
                              const graphop_plan_t* plan, void* stream) {
  const char* fn = "edge_dropout_mask";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, 1));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  hipStream_t st = (hipStream_t)stream;
  if (n_edges == 0) return GRAPHOP_OK;
  GO_PTR(fn, y);
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "the row-major rows", n_l, "the neighbours", n_r));
  const bool covered = g.covered();
  if (!covered) GO_HIP(zero_async(y, esize(dtype) * (size_t)(n_edges * h), st));   // edges no slot names get m = 0
  if (n_chunks == 0) return GRAPHOP_OK;
  GO_TRY(g.require(fn));
  ProfScope prof("edge_dropout_mask", st, "k_edge_dropout_mask");
  const unsigned nb = (unsigned)ceil_div(n_chunks, kGenericWavesPerBlock);
  GO_DISPATCH_FLOAT(dtype, T, {
    hipLaunchKernelGGL((k_edge_dropout_mask<T>), dim3(nb), dim3(kGenericBlock), 0, st, g.row,
                       g.indptr, g.eid, g.indices, (T*)y, n_chunks, h, drop.as<T>());
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // extern "C"
