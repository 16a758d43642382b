// Fused dot-product attention with an edge-type score bias (extra op, not one of the reference's eight;
// include/graphop_hip.h): for edge e = (i, j) of type t_e = etype[e] (by edge id) and head k,
//   forward : s_e = <Q_i, K_j> + B[t_e, k], o[i] = sum_e softmax_e(s) mult_e V_j, leaving o and the row statistics
//   backward: dQ, dK, dV and dB[t, k] = sum_{e : t_e = t} ds_e from (Q, K, V, B, etype, o, stats, dO)
// etype is the only edge-sized operand; nothing else edge-sized exists, the dropout mask included.  The host side is
// host_attn_edge_ops.h, shared with attention_edge.hip and attention_etype.hip: this file states the form -- the table
// where the edge rows are, its row being h scalars that enter the score and not h d floats that enter key and value,
// the replicas of dB around the fast row pass -- and the entry points.  The fp32 fast kernels (kernels_attn_tbias.h)
// run for the (h, d) pairs of GO_DISPATCH_GAT_HD with 16-byte aligned operands and matching plans; the row pass with dB
// sums it in LDS and so also wants n_types * h <= kAttnTbiasMaxWords.  The generic kernels of the same header run for
// everything else, pass by pass.  No kernel trusts a type: each clamps it into [0, n_types - 1], and nothing here scans
// etype (a scan would synchronise and break stream capture).  force_generic selects the generic kernels.  p == 0 takes
// the kernels without the keep decision.
#include "kernels_attn_tbias.h"
#include "host_attn_edge_ops.h"

using namespace graphop;

namespace {

// The shared host side passes F = h d, the width of an edge ROW; this form's table row is h words wide, so Rows carries
// h itself and the hooks ignore F.
struct TbiasForm {
  GO_ATTN_EDGE_FORM_NAMES(tbias, Tbias);
  struct Rows {
    const void* B;
    const int32_t* etype;
    i64 n_types;
    void* dB;   // NULL: not wanted
    i64 h;      // words of a table row
    unsigned tmax() const { return (unsigned)(n_types - 1); }
    i64 words() const { return n_types * h; }
  };
  static int check(const char* fn, const Rows& x, i64 n_edges, i64 h, i64 d) {
    GO_CHECK_ARG(x.n_types >= 0 && (n_edges == 0 || x.n_types >= 1), "%s: n_types must be >= 1 with n_edges > 0, got %lld",
                 fn, (long long)x.n_types);
    GO_CHECK_ARG(n_edges * h * d == 0 || x.B != nullptr, "%s: B is NULL", fn);
    GO_CHECK_ARG(n_edges * h * d == 0 || x.etype != nullptr, "%s: etype is NULL", fn);
    return GRAPHOP_OK;
  }
  static bool fast_ok(const Rows& x, i64, bool backward) {
    return x.n_types < 0x7fffffffLL / (x.h > 0 ? x.h : 1) && aligned16(x.B) && aligned16(x.etype) &&
           (!backward || aligned16(x.dB));
  }
  // the row pass may sum dB on chip
  static bool table_ok(const Rows& x) { return x.words() <= kAttnTbiasMaxWords; }
  static bool row_fast_ok(const Rows& x, i64) { return x.dB == nullptr || table_ok(x); }
  // the replicas of dB where the table fits: the size does not depend on whether dB is wanted
  static size_t ws_tail(const Rows& x, i64) {
    return table_ok(x) ? up256(sizeof(float) * (size_t)(kAttnTbiasReplicas * x.words())) : 0;
  }
  // types no edge carries get dB = 0; the fast row pass writes dB from its replicas instead (row_close)
  static int grad_fill(const Rows& x, size_t es, i64, bool fast_r, hipStream_t st) {
    if (x.dB != nullptr && x.words() > 0 && !fast_r) GO_HIP(zero_async(x.dB, es * (size_t)x.words(), st));
    return GRAPHOP_OK;
  }
  static void set_fwd(FwdArgs& a, const Rows& x) {
    a.B = (const float*)x.B; a.etype = (const int*)x.etype; a.tmax = x.tmax();
  }
  static auto rows_args(const Rows& x) {
    return std::make_tuple((const float*)x.B, (const int*)x.etype, x.tmax(), kAttnTbiasReplicas);
  }
  template <class T> static auto generic_args(const Rows& x) {
    return std::make_tuple((const T*)x.B, (const int*)x.etype, x.tmax());
  }
  // the fast row pass adds into the replicas of dB (n_types * h floats each), NULL: dB is not wanted
  static float* row_grad(const Rows& x, bool fast_r, void* tail) { return fast_r && x.dB != nullptr ? (float*)tail : nullptr; }
  static void* grad(const Rows& x) { return x.dB; }
  static size_t row_lds(const Rows& x, const float* rep, i64) { return rep ? sizeof(float) * (size_t)x.words() : 0; }
  static int row_open(const Rows& x, float* rep, i64 F, hipStream_t st) {
    if (rep) GO_HIP(zero_async(rep, ws_tail(x, F), st));
    return GRAPHOP_OK;
  }
  static int row_close(const Rows& x, float* rep, i64, hipStream_t st) {
    if (!rep) return GRAPHOP_OK;
    ProfScope prof("attn_tbias_db_reduce", st, "k_attn_tbias_db_reduce");
    hipLaunchKernelGGL(k_attn_tbias_db_reduce, dim3(grid_of(x.words())), dim3(256), 0, st, (const float*)rep,
                       (float*)x.dB, (int)x.words(), kAttnTbiasReplicas);
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
};

}  // namespace

extern "C" {

int graphop_attention_tbias_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                            int64_t d, int64_t n_types, const graphop_plan_t* plan_r,
                                            const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out) {
  (void)stream;
  return attn_edge_workspace_bytes<TbiasForm>("attention_tbias_workspace_bytes", dtype, backward, n_edges, n_q, n_k, h, d,
                                              n_types >= 0, {nullptr, nullptr, n_types, nullptr, h}, plan_r, plan_c,
                                              bytes_out);
}

int graphop_attention_tbias_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* Q, const void* K, const void* V, const void* B,
                                    const int32_t* etype, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_q, int64_t n_k, int64_t h, int64_t d, int64_t n_types, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan, void* stream, double p,
                                    uint64_t seed, uint32_t offset, int64_t head0) {
  return attn_edge_forward<TbiasForm>("attention_tbias_forward", dtype, row, indptr, eid, indices, Q, K, V,
                                      {B, etype, n_types, nullptr, h}, o, stats, n_chunks, n_edges, n_q, n_k, h, d,
                                      workspace, workspace_bytes, plan, stream, DropIn{p, seed, offset, head0});
}

int graphop_attention_tbias_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                     const void* V, const void* B, const int32_t* etype, const void* o, const void* stats,
                                     const void* dO, void* dQ, void* dK, void* dV, void* dB, int64_t n_row_chunks,
                                     int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                                     int64_t n_types, void* workspace, int64_t workspace_bytes,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream, double p,
                                     uint64_t seed, uint32_t offset, int64_t head0) {
  return attn_edge_backward<TbiasForm>("attention_tbias_backward", dtype, row, indptr_r, eid_r, indices_r, col, indptr_c,
                                       eid_c, indices_c, Q, K, V, {B, etype, n_types, dB, h}, o, stats, dO, dQ, dK, dV,
                                       n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d, workspace, workspace_bytes,
                                       plan_r, plan_c, stream, DropIn{p, seed, offset, head0});
}

}  // extern "C"
