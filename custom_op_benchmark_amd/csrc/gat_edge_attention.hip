// Fused GAT attention with an edge term (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : o[i] = sum_j softmax_j(LeakyReLU(el[i] + er[j] + ee[e])) m_ij V[j] per head, leaving o and the row statistics
//   backward: del, der, dV and dee[e] = dz_e from (el, er, ee, V, o, stats, dO), a recomputed per slot
// (kernels_gat_edge_attn.h).  ee and dee are the only edge-sized operands; nothing else edge-sized exists, the dropout
// mask included.  Validation, fills and the choice between the fp32 fast kernels and the generic ones are the one
// implementation gat_attention.hip also uses (host_gat_attn_ops.h, here with EDGE = true); p == 0 takes the
// DROP = false kernels.
#include "common.h"
#include "host.h"
#include "host_gat_attn_ops.h"

using namespace graphop;

extern "C" {

int graphop_gat_edge_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                       const int64_t* indices, const void* el, const void* er, const void* ee,
                                       const void* V, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                       int64_t n_l, int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                       uint64_t seed, uint32_t offset, const graphop_plan_t* plan, void* stream) {
  const char* fn = "gat_edge_attention_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &hd));
  return gat_attn_forward<true>(fn, dtype, row, indptr, eid, indices, el, er, ee, V, o, stats, n_chunks, n_edges, n_l,
                                n_r, h, d, negative_slope, p > 0.0 ? &hd : nullptr, plan, stream);
}

int graphop_gat_edge_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                        const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                        const int64_t* eid_c, const int64_t* indices_c, const void* el, const void* er,
                                        const void* ee, const void* V, const void* o, const void* stats,
                                        const void* dO, void* del, void* der, void* dee, void* dV, void* workspace,
                                        int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                                        int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                        double negative_slope, double p, uint64_t seed, uint32_t offset,
                                        const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gat_edge_attention_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &hd));
  return gat_attn_backward<true>(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, el, er, ee,
                                 V, o, stats, dO, del, der, dee, dV, workspace, workspace_bytes, n_row_chunks,
                                 n_col_chunks, n_edges, n_l, n_r, h, d, negative_slope, p > 0.0 ? &hd : nullptr, plan_r,
                                 plan_c, stream);
}

}  // extern "C"
