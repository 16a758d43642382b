// The bfloat16 fused attention step with edge features and, as an option, attention dropout
// (kernels_attn_edge_bf16.h): the three graphop_attention_edge_bf16_* entry points.  One form and no
// composed path: an unmet condition is an error that names it, nothing is upcast.  The workspace is the plain bf16 step's
// (host_attn_bf16.h), byte for byte: the edge row adds nothing to records or tables, and dxe is the caller's.
#include "common.h"
#include "host.h"
#include "host_attn_bf16.h"
#include "host_attn_rows.h"
#include "host_dropout.h"
#include "kernels_attn_edge_bf16.h"

namespace graphop {
namespace {

const char* const kQuery = "attention_edge_bf16_workspace_bytes";

// the dropout arguments, checked in the header's order; *drop: the kernels' record, meaningful where p > 0
int edge_drop_check(const char* fn, double p, uint64_t seed, uint32_t offset, i64 head0, i64 n_q, i64 n_k, i64 h,
                    AttnBf16Drop* drop) {
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_q, n_k, offset, &hd));
  GO_CHECK_ARG(head0 >= 0 && head0 + h < ((i64)1 << 31), "%s: head0 >= 0 and head0 + h < 2^31 wanted, got head0 = %lld, h = %lld",
               fn, (long long)head0, (long long)h);
  *drop = AttnBf16Drop{hd.as<float>(), (int)head0};
  return GRAPHOP_OK;
}

template <bool DROP>
AttnBf16DropIf<DROP> drop_if(const AttnBf16Drop& d) {
  if constexpr (DROP) return d;
  else return NoDrop{};
}

// one backward pass and its merge; dxe: the row pass's, NULL = not wanted
template <bool COL>
int edge_bwd_pass(const char* tag, const Csr& g, i64 h, i64 d, const uint4* own, const uint4* xt,
                  const float4* st4, const uint4* xe, uint4* out0, uint4* out1, uint4* dxe, const Bf16BwdWs& w,
                  bool dropped, const AttnBf16Drop& drop, hipStream_t st) {
  if (g.n_chunks == 0) return GRAPHOP_OK;
  const Bf16Geo geo(g.n_chunks, bf16_lanes(h, d));
  const AttnBf16BwdRec rec{w.p_row, w.p_acc};
  bf16_fill_rows("attn_edge_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof(tag, st, "k_edge_bf16_bwd_rows");
    GO_DISPATCH_ATTN_BF16_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_edge_bf16_bwd_rows<H, D, COL, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row,
                         g.indptr, g.eid_or_null(), g.indices, own, xt, st4, xe, out0, out1, dxe, rec, g.n_chunks, (int)geo.cpg,
                         drop_if<DROP>(drop));
    }));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("attn_edge_bf16_bwd_merge", st, "k_attn_bf16_bwd_merge");
  GO_DISPATCH_ATTN_BF16_HD(h, d, {
    hipLaunchKernelGGL((k_attn_bf16_bwd_merge<H, D, COL>), geo.grid(geo.np), dim3(kFastBlock), 0, st, rec, out0, out1, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace
}  // namespace graphop

using namespace graphop;

extern "C" {

int graphop_attention_edge_bf16_workspace_bytes(int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                                int64_t d, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                                void* stream, int64_t* bytes_out) {
  const char* fn = kQuery;
  (void)stream;
  GO_CHECK_ARG(bytes_out != nullptr, "%s: bytes_out is NULL", fn);
  *bytes_out = 0;
  GO_TRY(attn_check(fn, GRAPHOP_F32, 0, 0, n_edges, n_q, n_k, h, d));
  *bytes_out = (int64_t)attn_bf16_workspace(backward != 0, h, d, n_edges, n_q, n_k, plan_r, plan_c);   // 0: would refuse
  return GRAPHOP_OK;
}

int graphop_attention_edge_bf16_forward(const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                        const int64_t* indices, const void* Q, const void* K, const void* V,
                                        const void* xe, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                        int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                                        int64_t workspace_bytes, const graphop_plan_t* plan, void* stream, double p,
                                        uint64_t seed, uint32_t offset, int64_t head0) {
  const char* fn = "attention_edge_bf16_forward";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, GRAPHOP_F32, n_chunks, 0, n_edges, n_q, n_k, h, d));
  AttnBf16Drop drop;
  GO_TRY(edge_drop_check(fn, p, seed, offset, head0, n_q, n_k, h, &drop));
  GO_CHECK_ARG(n_edges * h * d == 0 || xe != nullptr, "%s: xe is NULL", fn);
  hipStream_t st = (hipStream_t)stream;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const i64 F = h * d;
  if (n_q * h == 0) return GRAPHOP_OK;
  GO_PTR(fn, stats);
  if (F > 0) GO_PTR(fn, o);
  const bool slots = n_edges > 0 && n_chunks > 0 && F > 0 && n_k > 0;
  if (slots) {
    char why[256];
    GO_CHECK_ARG(!bf16_shape_unmet(why, sizeof(why), h, d) && !bf16_plan_unmet(why, sizeof(why), "plan", g.plan, n_edges, n_q, n_k),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V);
    GO_TRY(bf16_tables_aligned(fn, {Q, K, V, xe, o}));
  }
  // rows without slots: o = 0, stats = (0, 0)
  GO_HIP(zero_async(stats, sizeof(float) * (size_t)(n_q * h * 2), st));
  GO_HIP(zero_async(o, 2 * (size_t)(n_q * F), st));
  if (!slots) return GRAPHOP_OK;
  const Bf16Geo geo(n_chunks, bf16_lanes(h, d));
  const Bf16FwdWs w(workspace, geo.np, h, F);
  GO_TRY(attn_ws_check(fn, kQuery, true, w.total, workspace, workspace_bytes));
  const AttnBf16FwdArgs a{(const uint4*)Q, (const uint4*)K, (const uint4*)V, (uint4*)o, (float*)stats, w.p_row, w.p_ml, w.p_o};
  const bool dropped = p > 0.0;
  bf16_fill_rows("attn_edge_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof("attn_edge_bf16_fwd_rows", st, "k_edge_bf16_fwd_rows");
    GO_DISPATCH_ATTN_BF16_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_edge_bf16_fwd_rows<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row, g.indptr,
                         g.eid_or_null(), g.indices, a, (const uint4*)xe, n_chunks, (int)geo.cpg, drop_if<DROP>(drop));
    }));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("attn_edge_bf16_fwd_merge", st, "k_attn_bf16_fwd_merge");
  GO_DISPATCH_ATTN_BF16_HD(h, d, {
    hipLaunchKernelGGL((k_attn_bf16_fwd_merge<H, D>), geo.grid(geo.np), dim3(kFastBlock), 0, st, a, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_attention_edge_bf16_backward(const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                         const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                         const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                         const void* V, const void* xe, const void* o, const void* stats, const void* dO,
                                         void* dQ, void* dK, void* dV, void* dxe, int64_t n_row_chunks,
                                         int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                         int64_t d, void* workspace, int64_t workspace_bytes,
                                         const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream,
                                         double p, uint64_t seed, uint32_t offset, int64_t head0) {
  const char* fn = "attention_edge_bf16_backward";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, GRAPHOP_F32, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d));
  AttnBf16Drop drop;
  GO_TRY(edge_drop_check(fn, p, seed, offset, head0, n_q, n_k, h, &drop));
  GO_CHECK_ARG(n_edges * h * d == 0 || xe != nullptr, "%s: xe is NULL", fn);
  hipStream_t st = (hipStream_t)stream;
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const i64 F = h * d;
  const bool empty = n_q * F == 0 || n_k * F == 0 || n_edges == 0 || (n_row_chunks == 0 && n_col_chunks == 0);
  if (!empty) {
    char why[256];
    GO_CHECK_ARG(!bf16_shape_unmet(why, sizeof(why), h, d) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan_r", r.plan, n_edges, n_q, n_k) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan_c", c.plan, n_edges, n_k, n_q),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  }
  if (n_q * F > 0) GO_PTR(fn, dQ);
  if (n_k * F > 0) { GO_PTR(fn, dK); GO_PTR(fn, dV); }
  if (!empty) GO_TRY(bf16_tables_aligned(fn, {Q, K, V, xe, o, dO, dQ, dK, dV, dxe}));
  GO_HIP(zero_async(dQ, 2 * (size_t)(n_q * F), st));
  GO_HIP(zero_async(dK, 2 * (size_t)(n_k * F), st));
  GO_HIP(zero_async(dV, 2 * (size_t)(n_k * F), st));
  if (empty) return GRAPHOP_OK;   // (no row-major slot names an edge id: dxe is left untouched)
  const int lanes = bf16_lanes(h, d);
  const Bf16BwdWs w(workspace, n_q, n_k, h, F, Bf16Geo(n_row_chunks, lanes).np, Bf16Geo(n_col_chunks, lanes).np);
  GO_TRY(attn_ws_check(fn, kQuery, true, w.total, workspace, workspace_bytes));
  {
    ProfScope prof("attn_edge_bf16_pack", st, "k_attn_bf16_pack");
    const i64 rpb = kFastBlock / lanes;
    GO_DISPATCH_ATTN_BF16_HD(h, d, {
      hipLaunchKernelGGL((k_attn_bf16_pack<H, D, false>), dim3((unsigned)ceil_div(n_k, rpb)), dim3(kFastBlock), 0, st,
                         (const uint4*)K, (const uint4*)V, w.kv, n_k, (const uint4*)nullptr, (const float*)nullptr,
                         (float4*)nullptr);
      hipLaunchKernelGGL((k_attn_bf16_pack<H, D, true>), dim3((unsigned)ceil_div(n_q, rpb)), dim3(kFastBlock), 0, st,
                         (const uint4*)Q, (const uint4*)dO, w.qdo, n_q, (const uint4*)o, (const float*)stats, w.st4);
    });
    GO_LAUNCH_CHECK();
  }
  const bool dropped = p > 0.0;
  GO_TRY((edge_bwd_pass<false>("attn_edge_bf16_rows_row", r, h, d, w.qdo, w.kv, w.st4, (const uint4*)xe,
                               (uint4*)dQ, nullptr, (uint4*)dxe, w, dropped, drop, st)));
  GO_TRY((edge_bwd_pass<true>("attn_edge_bf16_rows_col", c, h, d, w.kv, w.qdo, w.st4, (const uint4*)xe, (uint4*)dK,
                              (uint4*)dV, nullptr, w, dropped, drop, st)));
  return GRAPHOP_OK;
}

}  // extern "C"
