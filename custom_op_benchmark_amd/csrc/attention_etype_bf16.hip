// The bfloat16 fused attention step with edge-type embeddings and, as an option, attention dropout
// (kernels_attn_etype_bf16.h): the three graphop_attention_etype_bf16_* entry points.  One form and no
// composed path: an unmet condition is an error that names it, nothing is upcast.  The workspace is the plain bf16 step's
// (host_attn_bf16.h) plus, last in the backward's, the row pass's partial tables of dR: a bounded number of them.
#include "common.h"
#include "host.h"
#include "host_attn_bf16.h"
#include "host_attn_rows.h"
#include "host_dropout.h"
#include "kernels_attn_etype_bf16.h"

namespace graphop {
namespace {

const char* const kQuery = "attention_etype_bf16_workspace_bytes";

// the dropout arguments, checked in the header's order; *drop: the kernels' record, meaningful where p > 0
int etype_drop_check(const char* fn, double p, uint64_t seed, uint32_t offset, i64 head0, i64 n_q, i64 n_k, i64 h,
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

// what the table may hold: n_types >= 1 with edges, and the words of the on-chip tables (both directions: the forms do not
// differ by pass)
bool etype_table_fits(i64 n_types, i64 h, i64 d) {
  return n_types <= kEtypeBf16MaxWords && h <= kEtypeBf16MaxWords && d <= kEtypeBf16MaxWords &&
         n_types * h * d <= kEtypeBf16MaxWords;
}
int etype_table_check(const char* fn, i64 n_types, i64 n_edges, i64 h, i64 d) {
  GO_CHECK_ARG(n_types >= 0 && (n_edges == 0 || n_types >= 1), "%s: n_types must be >= 1 with n_edges > 0, got %lld", fn,
               (long long)n_types);
  GO_CHECK_ARG(etype_table_fits(n_types, h, d),
               "%s: bfloat16 unsupported: n_types * h * d = %llu is above %lld, the words of the on-chip tables of R and "
               "dR (attention_edge_bf16_* on the gathered rows R[etype] serves a larger table)",
               fn, (unsigned long long)n_types * (unsigned long long)h * (unsigned long long)d, (long long)kEtypeBf16MaxWords);
  return GRAPHOP_OK;
}

i64 etype_wp(i64 words) { return (i64)(up256(sizeof(float) * (size_t)words) / sizeof(float)); }

// the virtual workgroups of the row pass -- those of the plain launch -- and the workgroups that run with dR, each of
// which leaves one partial table
i64 etype_row_vblocks(i64 n_row_chunks, int lanes) {
  return n_row_chunks > 0 ? ceil_div(Bf16Geo(n_row_chunks, lanes).groups, (i64)(kFastBlock / lanes)) : 0;
}
i64 etype_parts(i64 vblocks) { return vblocks < kEtypeBf16Parts ? vblocks : kEtypeBf16Parts; }

// a row-pass instantiation whose dynamic LDS exceeds the default 64 KiB says so, once per device (the attribute is the
// most the kernel can ever ask for: R and the four tables at the bound)
template <int H, int D, bool COL, bool DROP, bool DR>
int etype_lds_limit(size_t lds) {
  constexpr int kDevices = 64;
  static bool raised[kDevices] = {};
  if (lds <= 65536) return GRAPHOP_OK;
  int dev = 0;
  GO_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < kDevices && raised[dev]) return GRAPHOP_OK;
  const size_t most = (size_t)kEtypeBf16MaxWords * (2 + 4 * sizeof(float));
  GO_HIP(hipFuncSetAttribute((const void*)k_etype_bf16_bwd_rows<H, D, COL, DROP, DR>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
  if (dev >= 0 && dev < kDevices) raised[dev] = true;
  return GRAPHOP_OK;
}

// one backward pass and its merge; partial: the row pass's tables of dR, NULL = not wanted
template <bool COL>
int etype_bwd_pass(const char* tag, const Csr& g, i64 h, i64 d, const uint4* own, const uint4* xt, const float4* st4,
                   const EtypeBf16Tab& tb, uint4* out0, uint4* out1, float* partial, const Bf16BwdWs& w, bool dropped,
                   const AttnBf16Drop& drop, hipStream_t st) {
  if (g.n_chunks == 0) return GRAPHOP_OK;
  const int lanes = bf16_lanes(h, d);
  const Bf16Geo geo(g.n_chunks, lanes);
  const AttnBf16BwdRec rec{w.p_row, w.p_acc};
  bf16_fill_rows("attn_etype_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof(tag, st, "k_etype_bf16_bwd_rows");
    const i64 words = (i64)tb.pieces * 8, vblocks = geo.grid(geo.groups).x;
    GO_DISPATCH_ATTN_BF16_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, GO_DISPATCH_BOOL(partial != nullptr, WANTED, {
      constexpr bool DR = WANTED && !COL;
      const size_t lds = (size_t)words * (DR ? 2 + 4 * sizeof(float) : 2);
      GO_TRY((etype_lds_limit<H, D, COL, DROP, DR>(lds)));
      const dim3 grid((unsigned)(DR ? etype_parts(vblocks) : vblocks));
      hipLaunchKernelGGL((k_etype_bf16_bwd_rows<H, D, COL, DROP, DR>), grid, dim3(kFastBlock), lds, st, g.row, g.indptr,
                         g.eid_or_null(), g.indices, own, xt, st4, tb, out0, out1, partial, (int)etype_wp(words), rec,
                         g.n_chunks, (int)geo.cpg, vblocks, drop_if<DROP>(drop));
    })));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("attn_etype_bf16_bwd_merge", st, "k_attn_bf16_bwd_merge");
  GO_DISPATCH_ATTN_BF16_HD(h, d, {
    hipLaunchKernelGGL((k_attn_bf16_bwd_merge<H, D, COL>), geo.grid(geo.np), dim3(kFastBlock), 0, st, rec, out0, out1, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

// the tree over n partial tables: its shape follows from n alone
int etype_dr_reduce(float* partial, i64 n, i64 words, bf16_bits_t* dR, hipStream_t st) {
  ProfScope prof("attn_etype_bf16_dr_reduce", st, "k_etype_bf16_dr_reduce");
  const unsigned bx = (unsigned)ceil_div(words, (i64)64);
  i64 stride = etype_wp(words);
  if (n > kEtypeBf16Fan) {
    const i64 per = ceil_div(n, (i64)kEtypeBf16Fan), segs = ceil_div(n, per);
    hipLaunchKernelGGL(k_etype_bf16_dr_reduce, dim3(bx, (unsigned)segs), dim3(256), 0, st, partial, n, stride, per,
                       (bf16_bits_t*)nullptr, (int)words);
    GO_LAUNCH_CHECK();
    n = segs;
    stride *= per;
  }
  hipLaunchKernelGGL(k_etype_bf16_dr_reduce, dim3(bx, 1), dim3(256), 0, st, partial, n, stride, n, dR, (int)words);
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace
}  // namespace graphop

using namespace graphop;

extern "C" {

int graphop_attention_etype_bf16_workspace_bytes(int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                                 int64_t d, int64_t n_types, const graphop_plan_t* plan_r,
                                                 const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out) {
  const char* fn = kQuery;
  (void)stream;
  GO_CHECK_ARG(bytes_out != nullptr, "%s: bytes_out is NULL", fn);
  *bytes_out = 0;
  GO_TRY(attn_check(fn, GRAPHOP_F32, 0, 0, n_edges, n_q, n_k, h, d));
  if (n_types < 0 || (n_edges > 0 && n_types < 1) || !etype_table_fits(n_types, h, d)) return GRAPHOP_OK;   // (would refuse)
  size_t total = attn_bf16_workspace(backward != 0, h, d, n_edges, n_q, n_k, plan_r, plan_c);
  if (backward && total > 0)   // the size does not depend on whether dR is wanted
    total += (size_t)etype_parts(etype_row_vblocks(plan_r->info.n_chunks, bf16_lanes(h, d))) *
             up256(sizeof(float) * (size_t)(n_types * h * d));
  *bytes_out = (int64_t)total;
  return GRAPHOP_OK;
}

int graphop_attention_etype_bf16_forward(const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                         const int64_t* indices, const void* Q, const void* K, const void* V,
                                         const void* R, const int32_t* etype, void* o, void* stats, int64_t n_chunks,
                                         int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d, int64_t n_types,
                                         void* workspace, int64_t workspace_bytes, const graphop_plan_t* plan, void* stream,
                                         double p, uint64_t seed, uint32_t offset, int64_t head0) {
  const char* fn = "attention_etype_bf16_forward";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, GRAPHOP_F32, n_chunks, 0, n_edges, n_q, n_k, h, d));
  AttnBf16Drop drop;
  GO_TRY(etype_drop_check(fn, p, seed, offset, head0, n_q, n_k, h, &drop));
  GO_TRY(etype_table_check(fn, n_types, n_edges, h, d));
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
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, R); GO_PTR(fn, etype);
    GO_TRY(bf16_tables_aligned(fn, {Q, K, V, R, o}));
  }
  // rows without slots: o = 0, stats = (0, 0)
  GO_HIP(zero_async(stats, sizeof(float) * (size_t)(n_q * h * 2), st));
  GO_HIP(zero_async(o, 2 * (size_t)(n_q * F), st));
  if (!slots) return GRAPHOP_OK;
  const Bf16Geo geo(n_chunks, bf16_lanes(h, d));
  const Bf16FwdWs w(workspace, geo.np, h, F);
  GO_TRY(attn_ws_check(fn, kQuery, true, w.total, workspace, workspace_bytes));
  const AttnBf16FwdArgs a{(const uint4*)Q, (const uint4*)K, (const uint4*)V, (uint4*)o, (float*)stats, w.p_row, w.p_ml, w.p_o};
  const EtypeBf16Tab tb{(const uint4*)R, (const int*)etype, (unsigned)(n_types - 1), (int)(n_types * F / 8)};
  const bool dropped = p > 0.0;
  bf16_fill_rows("attn_etype_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof("attn_etype_bf16_fwd_rows", st, "k_etype_bf16_fwd_rows");
    GO_DISPATCH_ATTN_BF16_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_etype_bf16_fwd_rows<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock),
                         sizeof(uint4) * (size_t)tb.pieces, st, g.row, g.indptr, g.eid_or_null(), g.indices, a, tb, n_chunks,
                         (int)geo.cpg, drop_if<DROP>(drop));
    }));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("attn_etype_bf16_fwd_merge", st, "k_attn_bf16_fwd_merge");
  GO_DISPATCH_ATTN_BF16_HD(h, d, {
    hipLaunchKernelGGL((k_attn_bf16_fwd_merge<H, D>), geo.grid(geo.np), dim3(kFastBlock), 0, st, a, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_attention_etype_bf16_backward(const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                          const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                          const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                          const void* V, const void* R, const int32_t* etype, const void* o,
                                          const void* stats, const void* dO, void* dQ, void* dK, void* dV, void* dR,
                                          int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_q,
                                          int64_t n_k, int64_t h, int64_t d, int64_t n_types, void* workspace,
                                          int64_t workspace_bytes, const graphop_plan_t* plan_r,
                                          const graphop_plan_t* plan_c, void* stream, double p, uint64_t seed,
                                          uint32_t offset, int64_t head0) {
  const char* fn = "attention_etype_bf16_backward";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, GRAPHOP_F32, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d));
  AttnBf16Drop drop;
  GO_TRY(etype_drop_check(fn, p, seed, offset, head0, n_q, n_k, h, &drop));
  GO_TRY(etype_table_check(fn, n_types, n_edges, h, d));
  hipStream_t st = (hipStream_t)stream;
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const i64 F = h * d, words = n_types * F;
  const bool empty = n_q * F == 0 || n_k * F == 0 || n_edges == 0 || (n_row_chunks == 0 && n_col_chunks == 0);
  if (!empty) {
    char why[256];
    GO_CHECK_ARG(!bf16_shape_unmet(why, sizeof(why), h, d) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan_r", r.plan, n_edges, n_q, n_k) &&
                     !bf16_plan_unmet(why, sizeof(why), "plan_c", c.plan, n_edges, n_k, n_q),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, R); GO_PTR(fn, etype); GO_PTR(fn, o); GO_PTR(fn, stats);
    GO_PTR(fn, dO);
  }
  if (n_q * F > 0) GO_PTR(fn, dQ);
  if (n_k * F > 0) { GO_PTR(fn, dK); GO_PTR(fn, dV); }
  if (!empty) GO_TRY(bf16_tables_aligned(fn, {Q, K, V, R, o, dO, dQ, dK, dV}));
  GO_HIP(zero_async(dQ, 2 * (size_t)(n_q * F), st));
  GO_HIP(zero_async(dK, 2 * (size_t)(n_k * F), st));
  GO_HIP(zero_async(dV, 2 * (size_t)(n_k * F), st));
  // without a row pass no edge adds to dR: every element is 0
  if (dR && (empty || n_row_chunks == 0)) GO_HIP(zero_async(dR, 2 * (size_t)words, st));
  if (empty) return GRAPHOP_OK;
  const int lanes = bf16_lanes(h, d);
  const Bf16BwdWs w(workspace, n_q, n_k, h, F, Bf16Geo(n_row_chunks, lanes).np, Bf16Geo(n_col_chunks, lanes).np);
  const i64 parts = etype_parts(etype_row_vblocks(n_row_chunks, lanes));
  const size_t total = w.total + (size_t)parts * up256(sizeof(float) * (size_t)words);
  GO_TRY(attn_ws_check(fn, kQuery, true, total, workspace, workspace_bytes));
  float* partial = dR && parts > 0 ? (float*)((char*)workspace + w.total) : nullptr;
  {
    ProfScope prof("attn_etype_bf16_pack", st, "k_attn_bf16_pack");
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
  const EtypeBf16Tab tb{(const uint4*)R, (const int*)etype, (unsigned)(n_types - 1), (int)(words / 8)};
  const bool dropped = p > 0.0;
  GO_TRY((etype_bwd_pass<false>("attn_etype_bf16_rows_row", r, h, d, w.qdo, w.kv, w.st4, tb, (uint4*)dQ, nullptr, partial, w,
                                dropped, drop, st)));
  if (partial) GO_TRY(etype_dr_reduce(partial, parts, words, (bf16_bits_t*)dR, st));
  GO_TRY((etype_bwd_pass<true>("attn_etype_bf16_rows_col", c, h, d, w.kv, w.qdo, w.st4, tb, (uint4*)dK, (uint4*)dV, nullptr, w,
                               dropped, drop, st)));
  return GRAPHOP_OK;
}

}  // extern "C"
