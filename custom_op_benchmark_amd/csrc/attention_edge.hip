// Fused dot-product attention with edge features (extra op, not one of the reference's eight; include/graphop_hip.h,
// DESIGN.md 4.5m): for edge e = (i, j), kx = K_j + xe[e] and vx = V_j + xe[e] with xe indexed by edge id,
//   forward : o[i] = sum_e softmax_e(<Q_i, kx_e>) mult_e vx_e per head, leaving o and the row statistics
//   backward: dQ, dK, dV and dxe[e] = ds_e Q_i + a_e mult_e dO_i from (Q, K, V, xe, o, stats, dO), s and a recomputed per slot
// xe and dxe are the only edge-sized operands; nothing else edge-sized exists, the dropout mask included.  The fp32
// fast kernels (kernels_attn_edge.h: the chunk-driver passes of the several-head kernels with the edge row streamed per
// slot) run for the (h, d) pairs of GO_DISPATCH_GAT_HD with 16-byte aligned operands and matching plans; the generic
// kernels of the same header run for everything else, pass by pass.  There is no composed form and no knob of its own:
// force_generic selects the generic kernels.  p == 0 takes the kernels without the keep decision.  The host side is
// host_attn_edge_ops.h, shared with attention_etype.hip: this file states the form and the entry points.
#include "kernels_attn_edge.h"
#include "host_attn_edge_ops.h"

using namespace graphop;

namespace {

struct EdgeForm {
  GO_ATTN_EDGE_FORM_NAMES(edge, Edge);
  struct Rows {
    const void* xe;
    void* dxe;   // NULL: not wanted; the binding clears what the row pass does not write
  };
  static int check(const char* fn, const Rows& x, i64 n_edges, i64 h, i64 d) {
    GO_CHECK_ARG(n_edges * h * d == 0 || x.xe != nullptr, "%s: xe is NULL", fn);
    return GRAPHOP_OK;
  }
  static bool fast_ok(const Rows& x, i64, bool backward) { return aligned16(x.xe) && (!backward || aligned16(x.dxe)); }
  static bool row_fast_ok(const Rows&, i64) { return true; }
  static size_t ws_tail(const Rows&, i64) { return 0; }
  static int grad_fill(const Rows&, size_t, i64, bool, hipStream_t) { return GRAPHOP_OK; }
  static void set_fwd(FwdArgs& a, const Rows& x) { a.xe = (const float*)x.xe; }
  static auto rows_args(const Rows& x) { return std::make_tuple((const float*)x.xe); }
  template <class T> static auto generic_args(const Rows& x) { return std::make_tuple((const T*)x.xe); }
  static float* row_grad(const Rows& x, bool, void*) { return (float*)x.dxe; }
  static void* grad(const Rows& x) { return x.dxe; }
  static size_t row_lds(const Rows&, const float*, i64) { return 0; }
  static int row_open(const Rows&, float*, i64, hipStream_t) { return GRAPHOP_OK; }
  static int row_close(const Rows&, float*, i64, hipStream_t) { return GRAPHOP_OK; }
};

}  // namespace

extern "C" {

int graphop_attention_edge_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                           int64_t d, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                           void* stream, int64_t* bytes_out) {
  (void)stream;
  return attn_edge_workspace_bytes<EdgeForm>("attention_edge_workspace_bytes", dtype, backward, n_edges, n_q, n_k, h, d,
                                             true, {}, plan_r, plan_c, bytes_out);
}

int graphop_attention_edge_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                   const int64_t* indices, const void* Q, const void* K, const void* V, const void* xe,
                                   void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                                   int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                   const graphop_plan_t* plan, void* stream, double p, uint64_t seed, uint32_t offset,
                                   int64_t head0) {
  return attn_edge_forward<EdgeForm>("attention_edge_forward", dtype, row, indptr, eid, indices, Q, K, V, {xe, nullptr},
                                     o, stats, n_chunks, n_edges, n_q, n_k, h, d, workspace, workspace_bytes, plan,
                                     stream, DropIn{p, seed, offset, head0});
}

int graphop_attention_edge_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                    const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                    const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                    const void* V, const void* xe, const void* o, const void* stats, const void* dO,
                                    void* dQ, void* dK, void* dV, void* dxe, int64_t n_row_chunks, int64_t n_col_chunks,
                                    int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                    void* stream, double p, uint64_t seed, uint32_t offset, int64_t head0) {
  return attn_edge_backward<EdgeForm>("attention_edge_backward", dtype, row, indptr_r, eid_r, indices_r, col, indptr_c,
                                      eid_c, indices_c, Q, K, V, {xe, dxe}, o, stats, dO, dQ, dK, dV, n_row_chunks,
                                      n_col_chunks, n_edges, n_q, n_k, h, d, workspace, workspace_bytes, plan_r, plan_c,
                                      stream, DropIn{p, seed, offset, head0});
}

}  // extern "C"
