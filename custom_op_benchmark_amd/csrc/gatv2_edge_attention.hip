// Fused GATv2 attention with edge features (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : o[i] = sum_j softmax_j(att . LeakyReLU((xl[i] + xr[j]) + xe[e])) m_ij xr[j] per head, leaving o and the row
//             statistics
//   backward: dxl, dxr, datt and dxe[e] = ds att t from (xl, xr, xe, att, o, stats, dO), z, s and a recomputed per slot
// (kernels_gatv2_edge_attn.h).  xe and dxe are the only edge-sized operands; nothing else edge-sized exists, the dropout
// mask included.  Validation, fills and the choice between the fp32 fast kernels and the generic ones are the one
// implementation gatv2_attention.hip also uses (host_gatv2_attn_ops.h, here with EDGE = true); p == 0 takes the
// kernels without the keep decision.
#include "common.h"
#include "host.h"
#include "host_gatv2_attn_ops.h"

using namespace graphop;

extern "C" {

int graphop_gatv2_edge_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                         const int64_t* indices, const void* xl, const void* xr, const void* xe,
                                         const void* att, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                         int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope,
                                         double p, uint64_t seed, uint32_t offset, const graphop_plan_t* plan,
                                         void* stream) {
  const char* fn = "gatv2_edge_attention_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gv2attn_forward<true>(fn, dtype, row, indptr, eid, indices, xl, xr, xe, att, o, stats, n_chunks, n_edges, n_l,
                               n_r, h, d, negative_slope, p > 0.0 ? &drop : nullptr, plan, stream);
}

int graphop_gatv2_edge_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                          const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                          const int64_t* eid_c, const int64_t* indices_c, const void* xl,
                                          const void* xr, const void* xe, const void* att, const void* o,
                                          const void* stats, const void* dO, void* dxl, void* dxr, void* dxe,
                                          void* datt, void* workspace, int64_t workspace_bytes, int64_t n_row_chunks,
                                          int64_t n_col_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h,
                                          int64_t d, double negative_slope, double p, uint64_t seed, uint32_t offset,
                                          const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gatv2_edge_attention_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gv2attn_backward<true>(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr, xe,
                                att, o, stats, dO, dxl, dxr, dxe, datt, workspace, workspace_bytes, n_row_chunks,
                                n_col_chunks, n_edges, n_l, n_r, h, d, negative_slope, p > 0.0 ? &drop : nullptr,
                                plan_r, plan_c, stream);
}

}  // extern "C"
