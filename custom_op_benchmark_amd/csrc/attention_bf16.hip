// The plain fused attention step on bfloat16 tables (kernels_attn_bf16.h): what is supported, the
// workspace layouts and the launches.  attention.hip calls these from the four entry points that take GRAPHOP_BF16
// (graphop_attention_forward / _backward / _workspace_bytes / _backward_is_fused); there is one form and no composed
// path behind it, so an unmet condition is an error that names it, and no knob steers anything.
#include "common.h"
#include "host.h"
#include "host_attn_bf16.h"

namespace graphop {
namespace {

template <bool COL>
int bf16_bwd_pass(const char* tag, const Csr& g, i64 h, i64 d, const uint4* own, const uint4* xt, const float4* st4,
                  uint4* out0, uint4* out1, const Bf16BwdWs& w, hipStream_t st) {
  if (g.n_chunks == 0) return GRAPHOP_OK;
  const Bf16Geo geo(g.n_chunks, bf16_lanes(h, d));
  const AttnBf16BwdRec rec{w.p_row, w.p_acc};
  bf16_fill_rows("attn_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof(tag, st, "k_attn_bf16_bwd_rows");
    GO_DISPATCH_ATTN_BF16_HD(h, d, {
      hipLaunchKernelGGL((k_attn_bf16_bwd_rows<H, D, COL>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row, g.indptr,
                         g.indices, own, xt, st4, out0, out1, rec, g.n_chunks, (int)geo.cpg);
    });
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("attn_bf16_bwd_merge", st, "k_attn_bf16_bwd_merge");
  GO_DISPATCH_ATTN_BF16_HD(h, d, {
    hipLaunchKernelGGL((k_attn_bf16_bwd_merge<H, D, COL>), geo.grid(geo.np), dim3(kFastBlock), 0, st, rec, out0, out1, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace

bool attn_bf16_ok(i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r, const graphop_plan* plan_c) {
  char why[256];
  return n_edges > 0 && !bf16_shape_unmet(why, sizeof(why), h, d) &&
         !bf16_plan_unmet(why, sizeof(why), "plan_r", plan_r, n_edges, n_q, n_k) &&
         !bf16_plan_unmet(why, sizeof(why), "plan_c", plan_c, n_edges, n_k, n_q);
}

size_t attn_bf16_workspace(bool backward, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r,
                           const graphop_plan* plan_c) {
  char why[256];
  if (n_edges == 0 || bf16_shape_unmet(why, sizeof(why), h, d) ||
      bf16_plan_unmet(why, sizeof(why), "plan_r", plan_r, n_edges, n_q, n_k))
    return 0;
  const int lanes = bf16_lanes(h, d);
  const i64 np_r = Bf16Geo(plan_r->info.n_chunks, lanes).np;
  if (!backward) return Bf16FwdWs(nullptr, np_r, h, h * d).total;
  if (bf16_plan_unmet(why, sizeof(why), "plan_c", plan_c, n_edges, n_k, n_q)) return 0;
  return Bf16BwdWs(nullptr, n_q, n_k, h, h * d, np_r, Bf16Geo(plan_c->info.n_chunks, lanes).np).total;
}

int attn_bf16_forward(const char* fn, const Csr& g, i64 n_q, i64 n_k, i64 h, i64 d, const void* Q, const void* K,
                      const void* V, void* o, void* stats, void* ws, i64 ws_bytes, hipStream_t st) {
  const i64 F = h * d;
  if (n_q * h == 0) return GRAPHOP_OK;
  GO_PTR(fn, stats);
  if (F > 0) GO_PTR(fn, o);
  if (g.n_edges > 0 && g.n_chunks > 0) {
    char why[256];
    GO_CHECK_ARG(!bf16_shape_unmet(why, sizeof(why), h, d) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan", g.plan, g.n_edges, n_q, n_k),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V);
    GO_TRY(bf16_tables_aligned(fn, {Q, K, V, o}));
  }
  // rows without slots: o = 0, stats = (0, 0)
  GO_HIP(zero_async(stats, sizeof(float) * (size_t)(n_q * h * 2), st));
  GO_HIP(zero_async(o, 2 * (size_t)(n_q * F), st));
  if (g.n_edges == 0 || g.n_chunks == 0) return GRAPHOP_OK;
  const Bf16Geo geo(g.n_chunks, bf16_lanes(h, d));
  const Bf16FwdWs w(ws, geo.np, h, F);
  GO_TRY(attn_ws_check(fn, "attention_workspace_bytes", true, w.total, ws, ws_bytes));
  const AttnBf16FwdArgs a{(const uint4*)Q, (const uint4*)K, (const uint4*)V, (uint4*)o, (float*)stats, w.p_row, w.p_ml, w.p_o};
  bf16_fill_rows("attn_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof("attn_bf16_fwd_rows", st, "k_attn_bf16_fwd_rows");
    GO_DISPATCH_ATTN_BF16_HD(h, d, {
      hipLaunchKernelGGL((k_attn_bf16_fwd_rows<H, D>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row, g.indptr,
                         g.indices, a, g.n_chunks, (int)geo.cpg);
    });
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("attn_bf16_fwd_merge", st, "k_attn_bf16_fwd_merge");
  GO_DISPATCH_ATTN_BF16_HD(h, d, {
    hipLaunchKernelGGL((k_attn_bf16_fwd_merge<H, D>), geo.grid(geo.np), dim3(kFastBlock), 0, st, a, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int attn_bf16_backward(const char* fn, const Csr& r, const Csr& c, i64 n_q, i64 n_k, i64 h, i64 d, const void* Q,
                       const void* K, const void* V, const void* o, const void* stats, const void* dO, void* dQ, void* dK,
                       void* dV, void* ws, i64 ws_bytes, hipStream_t st) {
  const i64 F = h * d;
  if ((n_q + n_k) * F == 0) return GRAPHOP_OK;
  const bool empty = r.n_edges == 0 || (r.n_chunks == 0 && c.n_chunks == 0);
  if (!empty) {
    char why[256];
    GO_CHECK_ARG(!bf16_shape_unmet(why, sizeof(why), h, d) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan_r", r.plan, r.n_edges, n_q, n_k) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan_c", c.plan, c.n_edges, n_k, n_q),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  }
  if (n_q > 0) GO_PTR(fn, dQ);
  if (n_k > 0) { GO_PTR(fn, dK); GO_PTR(fn, dV); }
  if (!empty) GO_TRY(bf16_tables_aligned(fn, {Q, K, V, o, dO, dQ, dK, dV}));
  GO_HIP(zero_async(dQ, 2 * (size_t)(n_q * F), st));
  GO_HIP(zero_async(dK, 2 * (size_t)(n_k * F), st));
  GO_HIP(zero_async(dV, 2 * (size_t)(n_k * F), st));
  if (empty) return GRAPHOP_OK;
  const int lanes = bf16_lanes(h, d);
  const Bf16BwdWs w(ws, n_q, n_k, h, F, Bf16Geo(r.n_chunks, lanes).np, Bf16Geo(c.n_chunks, lanes).np);
  GO_TRY(attn_ws_check(fn, "attention_workspace_bytes", true, w.total, ws, ws_bytes));
  {
    ProfScope prof("attn_bf16_pack", st, "k_attn_bf16_pack");
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
  GO_TRY((bf16_bwd_pass<false>("attn_bf16_rows_row", r, h, d, w.qdo, w.kv, w.st4, (uint4*)dQ, nullptr, w, st)));
  GO_TRY((bf16_bwd_pass<true>("attn_bf16_rows_col", c, h, d, w.kv, w.qdo, w.st4, (uint4*)dK, (uint4*)dV, w, st)));
  return GRAPHOP_OK;
}

}  // namespace graphop
