// Fused dot-product attention with edge-type embeddings (extra op, not one of the reference's eight;
// include/graphop_hip.h): for edge e = (i, j) of type t_e = etype[e] (by edge id), kx = K_j + R[t_e] and
// vx = V_j + R[t_e],
//   forward : o[i] = sum_e softmax_e(<Q_i, kx_e>) mult_e vx_e per head, leaving o and the row statistics
//   backward: dQ, dK, dV and dR[t] = sum_{e : t_e = t} (ds_e Q_i + a_e mult_e dO_i) from (Q, K, V, R, etype, o, stats, dO)
// etype is the only edge-sized operand; nothing else edge-sized exists, the dropout mask included.  The host side is
// host_attn_edge_ops.h, shared with attention_edge.hip: this file states the form -- the table where the edge rows
// are, the replicas of dR around the fast row pass -- and the entry points.  The fp32 fast kernels (kernels_attn_etype.h: the
// chunk-driver passes with the edge piece read from the table) run for the (h, d) pairs of GO_DISPATCH_GAT_HD with
// 16-byte aligned operands and matching plans; the row pass with dR sums it in LDS and so also wants
// n_types <= attn_etype_max_types(h d).  The generic kernels of the same header run for everything else, pass by pass.
// No kernel trusts a type: each clamps it into [0, n_types - 1], and nothing here scans etype (a scan would synchronise
// and break stream capture).  force_generic selects the generic kernels.  p == 0 takes the kernels without the keep
// decision.
#include "kernels_attn_etype.h"
#include "host_attn_edge_ops.h"

using namespace graphop;

namespace {

struct EtypeForm {
  GO_ATTN_EDGE_FORM_NAMES(etype, Etype);
  struct Rows {
    const void* R;
    const int32_t* etype;
    i64 n_types;
    void* dR;   // NULL: not wanted
    unsigned tmax() const { return (unsigned)(n_types - 1); }
  };
  static int check(const char* fn, const Rows& x, i64 n_edges, i64 h, i64 d) {
    GO_CHECK_ARG(x.n_types >= 0 && (n_edges == 0 || x.n_types >= 1), "%s: n_types must be >= 1 with n_edges > 0, got %lld",
                 fn, (long long)x.n_types);
    GO_CHECK_ARG(n_edges * h * d == 0 || x.R != nullptr, "%s: R is NULL", fn);
    GO_CHECK_ARG(n_edges * h * d == 0 || x.etype != nullptr, "%s: etype is NULL", fn);
    return GRAPHOP_OK;
  }
  static bool fast_ok(const Rows& x, i64 F, bool backward) {
    return x.n_types < 0x7fffffffLL / (F > 0 ? F : 1) && aligned16(x.R) && aligned16(x.etype) && (!backward || aligned16(x.dR));
  }
  // the row pass may sum dR on chip
  static bool table_ok(const Rows& x, i64 F) { return x.n_types <= attn_etype_max_types(F); }
  static bool row_fast_ok(const Rows& x, i64 F) { return x.dR == nullptr || table_ok(x, F); }
  // the replicas of dR where the table fits: the size does not depend on whether dR is wanted
  static size_t ws_tail(const Rows& x, i64 F) {
    return table_ok(x, F) ? up256(sizeof(float) * (size_t)(kAttnEtypeReplicas * x.n_types * F)) : 0;
  }
  // types no edge carries get dR = 0; the fast row pass writes dR from its replicas instead (row_close)
  static int grad_fill(const Rows& x, size_t es, i64 F, bool fast_r, hipStream_t st) {
    if (x.dR != nullptr && x.n_types * F > 0 && !fast_r) GO_HIP(zero_async(x.dR, es * (size_t)(x.n_types * F), st));
    return GRAPHOP_OK;
  }
  static void set_fwd(FwdArgs& a, const Rows& x) {
    a.R = (const float*)x.R; a.etype = (const int*)x.etype; a.tmax = x.tmax();
  }
  static auto rows_args(const Rows& x) {
    return std::make_tuple((const float*)x.R, (const int*)x.etype, x.tmax(), kAttnEtypeReplicas);
  }
  template <class T> static auto generic_args(const Rows& x) {
    return std::make_tuple((const T*)x.R, (const int*)x.etype, x.tmax());
  }
  // the fast row pass adds into the replicas of dR (n_types * F floats each), NULL: dR is not wanted
  static float* row_grad(const Rows& x, bool fast_r, void* tail) { return fast_r && x.dR != nullptr ? (float*)tail : nullptr; }
  static void* grad(const Rows& x) { return x.dR; }
  static size_t row_lds(const Rows& x, const float* rep, i64 F) { return rep ? sizeof(float) * (size_t)(x.n_types * F) : 0; }
  static int row_open(const Rows& x, float* rep, i64 F, hipStream_t st) {
    if (rep) GO_HIP(zero_async(rep, ws_tail(x, F), st));
    return GRAPHOP_OK;
  }
  static int row_close(const Rows& x, float* rep, i64 F, hipStream_t st) {
    if (!rep) return GRAPHOP_OK;
    ProfScope prof("attn_etype_dr_reduce", st, "k_attn_etype_dr_reduce");
    hipLaunchKernelGGL(k_attn_etype_dr_reduce, dim3(grid_of(x.n_types * F)), dim3(256), 0, st, (const float*)rep,
                       (float*)x.dR, (int)(x.n_types * F), kAttnEtypeReplicas);
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
};

}  // namespace

extern "C" {

int graphop_attention_etype_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                            int64_t d, int64_t n_types, const graphop_plan_t* plan_r,
                                            const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out) {
  (void)stream;
  return attn_edge_workspace_bytes<EtypeForm>("attention_etype_workspace_bytes", dtype, backward, n_edges, n_q, n_k, h, d,
                                              n_types >= 0, {nullptr, nullptr, n_types, nullptr}, plan_r, plan_c,
                                              bytes_out);
}

int graphop_attention_etype_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* Q, const void* K, const void* V, const void* R,
                                    const int32_t* etype, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_q, int64_t n_k, int64_t h, int64_t d, int64_t n_types, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan, void* stream, double p,
                                    uint64_t seed, uint32_t offset, int64_t head0) {
  return attn_edge_forward<EtypeForm>("attention_etype_forward", dtype, row, indptr, eid, indices, Q, K, V,
                                      {R, etype, n_types, nullptr}, o, stats, n_chunks, n_edges, n_q, n_k, h, d,
                                      workspace, workspace_bytes, plan, stream, DropIn{p, seed, offset, head0});
}

int graphop_attention_etype_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                     const void* V, const void* R, const int32_t* etype, const void* o, const void* stats,
                                     const void* dO, void* dQ, void* dK, void* dV, void* dR, int64_t n_row_chunks,
                                     int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                                     int64_t n_types, void* workspace, int64_t workspace_bytes,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream, double p,
                                     uint64_t seed, uint32_t offset, int64_t head0) {
  return attn_edge_backward<EtypeForm>("attention_etype_backward", dtype, row, indptr_r, eid_r, indices_r, col, indptr_c,
                                       eid_c, indices_c, Q, K, V, {R, etype, n_types, dR}, o, stats, dO, dQ, dK, dV,
                                       n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d, workspace, workspace_bytes,
                                       plan_r, plan_c, stream, DropIn{p, seed, offset, head0});
}

}  // extern "C"
