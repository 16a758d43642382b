// The fused GAT attention layer on bfloat16 tables (kernels_gat_attn_bf16.h; include/graphop_hip.h:
// graphop_gat_attention_bf16_*): what is supported, the workspace layout and the launches.  One form, with and without
// attention dropout (p == 0 runs the DROP = false kernels); there is no generic path, no upcast and no knob behind it,
// so an unmet condition is an error that names it.  The statistics are the fp32 op's stats pass on widened copies of el
// and er (gat_attn_stats_f32, host.h).
#include "common.h"
#include "host.h"
#include "host_bf16.h"
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_gat_attn_bf16.h"

using namespace graphop;

namespace graphop {

// ---- widen: the fp32 copies of el and er the stats pass reads -------------------------------------------------------------
__global__ void k_gat_attn_bf16_widen(const bf16_t* __restrict__ a, float* __restrict__ a32, i64 n_a,
                                      const bf16_t* __restrict__ b, float* __restrict__ b32, i64 n_b) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_a + n_b; i += stride) {
    if (i < n_a) a32[i] = bf16_widen(a[i]);
    else b32[i - n_a] = bf16_widen(b[i - n_a]);
  }
}

}  // namespace graphop

namespace {

// lanes per group of a pair of GO_DISPATCH_GAT_HD, 0 outside it
int gat_bf16_lanes(i64 h, i64 d) {
  int lanes = 0;
  if (h >= 1 && h <= 8 && d >= 8 && d <= 64) GO_DISPATCH_GAT_HD(h, d, { lanes = GatBf16Cfg<H, D>::L; });
  return lanes;
}

// the first unmet condition of a direction into `why`; false: supported
bool gat_bf16_unmet(char* why, size_t cap, bool backward, i64 h, i64 d, i64 n_edges, i64 n_l, i64 n_r,
                    const graphop_plan* plan_r, const graphop_plan* plan_c) {
  if (!gat_bf16_lanes(h, d)) {
    snprintf(why, cap, "(h, d) = (%lld, %lld) is not in the bfloat16 set: h in {1, 2, 4, 8}, d in {8, 16, 32, 64}, "
             "h * d in {64, 128, 256}", (long long)h, (long long)d);
    return true;
  }
  const char* name_r = backward ? "plan_r" : "plan";
  if (bf16_plan_unmet(why, cap, name_r, plan_r, n_edges, n_l, n_r)) return true;
  if (!plan_r->seg_chunk) {
    snprintf(why, cap, "%s has no segment table for the stats pass", name_r);
    return true;
  }
  return backward && bf16_plan_unmet(why, cap, "plan_c", plan_c, n_edges, n_r, n_l);
}

// The workspace of one direction, stated once for the query and the call (base == NULL: only `total` means anything).
//   forward : 4 n_l h (el as fp32) + 4 n_r h (er as fp32) + 4 np_r (row words) + 4 np_r F (o records)
//   backward: 16 n_l h (P) + 4 max(np_r, np_c) (row words) + 4 h max(np_r, np_c) (del / der records) + 4 F np_c (dV
//             records): ONE record area for whichever pass is running
// np = 2 * lane groups of the orientation's chunk list (Bf16Geo); every term is rounded up to 256 bytes.
struct GatBf16Ws {
  float *el32 = nullptr, *er32 = nullptr, *p_o = nullptr;   // forward
  float4* P = nullptr;                                      // backward
  float *p_h = nullptr, *p_v = nullptr;
  unsigned* p_row;
  size_t total;
  GatBf16Ws(void* base, bool backward, i64 n_l, i64 n_r, i64 h, i64 F, i64 np_r, i64 np_c) {
    Bf16Take take{(char*)base};
    if (!backward) {
      el32 = (float*)take(sizeof(float) * (size_t)(n_l * h));
      er32 = (float*)take(sizeof(float) * (size_t)(n_r * h));
      p_row = (unsigned*)take(sizeof(unsigned) * (size_t)np_r);
      p_o = (float*)take(sizeof(float) * (size_t)(np_r * F));
    } else {
      const i64 np = np_r > np_c ? np_r : np_c;
      P = (float4*)take(sizeof(float4) * (size_t)(n_l * h));
      p_row = (unsigned*)take(sizeof(unsigned) * (size_t)np);
      p_h = (float*)take(sizeof(float) * (size_t)(np * h));
      p_v = (float*)take(sizeof(float) * (size_t)(np_c * F));
    }
    total = take.total;
  }
};

GatBf16Ws gat_bf16_ws(void* base, bool backward, i64 n_row_chunks, i64 n_col_chunks, i64 n_l, i64 n_r, i64 h, i64 d) {
  const int lanes = gat_bf16_lanes(h, d);
  return GatBf16Ws(base, backward, n_l, n_r, h, h * d, Bf16Geo(n_row_chunks, lanes).np,
                   backward ? Bf16Geo(n_col_chunks, lanes).np : 0);
}

// one backward pass over an orientation: row words, the gather kernel, the merge
template <bool COL>
int gat_bf16_bwd_pass(const Csr& g, i64 h, i64 d, const void* er, const void* V, const GatBf16Ws& w, const void* dO,
                      void* out_h, void* out_v, float slope, const HostDrop* drop, hipStream_t st) {
  if (g.n_chunks == 0) return GRAPHOP_OK;
  const Bf16Geo geo(g.n_chunks, gat_bf16_lanes(h, d));
  const GatBf16BwdRec rec{w.p_row, w.p_h, w.p_v};
  const bool dropped = drop != nullptr;
  bf16_fill_rows("gat_attn_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof(COL ? "gat_attn_bf16_bwd_col" : "gat_attn_bf16_bwd_row", st,
                   COL ? (dropped ? "k_gat_attn_bf16_drop_bwd_col" : "k_gat_attn_bf16_bwd_col")
                       : (dropped ? "k_gat_attn_bf16_drop_bwd_row" : "k_gat_attn_bf16_bwd_row"));
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      if constexpr (COL)
        hipLaunchKernelGGL((k_gat_attn_bf16_bwd_col<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row,
                           g.indptr, g.indices, (const bf16_t*)er, (const uint4*)V, (const float4*)w.P, (const uint4*)dO,
                           (bf16_t*)out_h, (uint4*)out_v, rec, g.n_chunks, (int)geo.cpg, slope,
                           drop_arg<DROP, float>(drop));
      else
        hipLaunchKernelGGL((k_gat_attn_bf16_bwd_row<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row,
                           g.indptr, g.indices, (const bf16_t*)er, (const uint4*)V, (const float4*)w.P, (const uint4*)dO,
                           (bf16_t*)out_h, rec, g.n_chunks, (int)geo.cpg, slope, drop_arg<DROP, float>(drop));
    }));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("gat_attn_bf16_bwd_merge", st, "k_gat_attn_bf16_bwd_merge");
  GO_DISPATCH_GAT_HD(h, d, {
    hipLaunchKernelGGL((k_gat_attn_bf16_bwd_merge<H, D, COL>), geo.grid(geo.np), dim3(kFastBlock), 0, st, rec,
                       (bf16_t*)out_h, (uint4*)out_v, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace

extern "C" {

int graphop_gat_attention_bf16_workspace_bytes(int backward, int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges,
                                               int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                               const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                               int64_t* bytes_out) {
  const char* fn = "gat_attention_bf16_workspace_bytes";
  GO_PTR(fn, bytes_out);
  *bytes_out = 0;
  GO_TRY(gat_check(fn, GRAPHOP_F32, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  char why[256];
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || (backward && n_col_chunks > 0)) && n_l > 0 && n_r > 0;
  if (!slots || gat_bf16_unmet(why, sizeof(why), backward != 0, h, d, n_edges, n_l, n_r, plan_r, plan_c) ||
      plan_r->info.n_chunks != n_row_chunks || (backward && plan_c->info.n_chunks != n_col_chunks))
    return GRAPHOP_OK;
  *bytes_out = (int64_t)gat_bf16_ws(nullptr, backward != 0, n_row_chunks, n_col_chunks, n_l, n_r, h, d).total;
  return GRAPHOP_OK;
}

int graphop_gat_attention_bf16_forward(const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                       const int64_t* indices, const void* el, const void* er, const void* V, void* o,
                                       void* stats, void* workspace, int64_t workspace_bytes, int64_t n_chunks,
                                       int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                       double negative_slope, double p, uint64_t seed, uint32_t offset,
                                       const graphop_plan_t* plan, void* stream) {
  const char* fn = "gat_attention_bf16_forward";
  GO_TRY(gat_check(fn, GRAPHOP_F32, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &hd));
  const HostDrop* drop = p > 0.0 ? &hd : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  GO_TRY(Csr::check_bounds(fn, g.plan, "el / o", n_l, "er / V", n_r));
  if (n_l == 0) return GRAPHOP_OK;
  GO_PTR(fn, o); GO_PTR(fn, stats);
  GO_CHECK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", fn);
  const i64 F = h * d;
  const bool slots = n_chunks > 0 && n_edges > 0 && n_r > 0;
  if (!slots) {   // o = 0, stats = (-1e9, 0)
    GO_HIP(zero_async(o, 2 * (size_t)(n_l * F), st));
    return gat_attn_stats_f32(g, nullptr, nullptr, stats, 0, n_l, h, negative_slope, "gat_attn_bf16_stats", st);
  }
  char why[256];
  GO_CHECK_ARG(!gat_bf16_unmet(why, sizeof(why), false, h, d, n_edges, n_l, n_r, g.plan, nullptr),
               "%s: bfloat16 unsupported: %s", fn, why);
  GO_TRY(g.require(fn));
  GO_PTR(fn, el); GO_PTR(fn, er); GO_PTR(fn, V);
  GO_TRY(bf16_tables_aligned(fn, {V, o}));
  const GatBf16Ws w = gat_bf16_ws(workspace, false, n_chunks, 0, n_l, n_r, h, d);
  GO_TRY(attn_ws_check(fn, "gat_attention_bf16_workspace_bytes", true, w.total, workspace, workspace_bytes));
  const Bf16Geo geo(n_chunks, gat_bf16_lanes(h, d));
  GO_HIP(zero_async(o, 2 * (size_t)(n_l * F), st));
  {
    ProfScope prof("gat_attn_bf16_setup", st, "k_gat_attn_bf16_widen");
    hipLaunchKernelGGL(k_gat_attn_bf16_widen, dim3(grid_of((n_l + n_r) * h)), dim3(256), 0, st, (const bf16_t*)el, w.el32,
                       n_l * h, (const bf16_t*)er, w.er32, n_r * h);
    GO_LAUNCH_CHECK();
  }
  GO_TRY(gat_attn_stats_f32(g, w.el32, w.er32, stats, n_chunks, n_l, h, negative_slope, "gat_attn_bf16_stats", st));
  bf16_fill_rows("gat_attn_bf16_setup", w.p_row, geo.np, st);
  const GatBf16FwdArgs a{(const bf16_t*)el, (const bf16_t*)er, (const float2*)stats, (const uint4*)V, (uint4*)o, w.p_row,
                         w.p_o};
  const bool dropped = drop != nullptr;
  {
    ProfScope prof("gat_attn_bf16_fwd", st, dropped ? "k_gat_attn_bf16_drop_fwd" : "k_gat_attn_bf16_fwd");
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_gat_attn_bf16_fwd<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row, g.indptr,
                         g.indices, a, n_chunks, (int)geo.cpg, (float)negative_slope, drop_arg<DROP, float>(drop));
    }));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("gat_attn_bf16_fwd_merge", st, "k_gat_attn_bf16_fwd_merge");
  GO_DISPATCH_GAT_HD(h, d, {
    hipLaunchKernelGGL((k_gat_attn_bf16_fwd_merge<H, D>), geo.grid(geo.np), dim3(kFastBlock), 0, st, a, geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_gat_attention_bf16_backward(const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                        const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                        const int64_t* eid_c, const int64_t* indices_c, const void* el, const void* er,
                                        const void* V, const void* o, const void* stats, const void* dO, void* del,
                                        void* der, void* dV, void* workspace, int64_t workspace_bytes,
                                        int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                        int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                        uint64_t seed, uint32_t offset, const graphop_plan_t* plan_r,
                                        const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gat_attention_bf16_backward";
  GO_TRY(gat_check(fn, GRAPHOP_F32, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &hd));
  const HostDrop* drop = p > 0.0 ? &hd : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  GO_TRY(Csr::check_bounds(fn, r.plan, "el / del", n_l, "er / V", n_r));
  GO_TRY(Csr::check_bounds(fn, c.plan, "er / der", n_r, "el", n_l));
  const i64 F = h * d;
  if (n_l > 0) GO_PTR(fn, del);
  if (n_r > 0) { GO_PTR(fn, der); GO_PTR(fn, dV); }
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || n_col_chunks > 0) && n_l > 0 && n_r > 0;
  GatBf16Ws w(nullptr, true, 0, 0, 0, 0, 0, 0);
  if (slots) {
    char why[256];
    GO_CHECK_ARG(!gat_bf16_unmet(why, sizeof(why), true, h, d, n_edges, n_l, n_r, r.plan, c.plan),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_TRY(r.require(fn));
    GO_TRY(c.require(fn));
    GO_PTR(fn, el); GO_PTR(fn, er); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
    GO_TRY(bf16_tables_aligned(fn, {V, o, dO, dV}));
    GO_CHECK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", fn);
    w = gat_bf16_ws(workspace, true, n_row_chunks, n_col_chunks, n_l, n_r, h, d);
    GO_TRY(attn_ws_check(fn, "gat_attention_bf16_workspace_bytes", true, w.total, workspace, workspace_bytes));
  }
  // rows and columns without chunks read 0
  GO_HIP(zero_async(del, 2 * (size_t)(n_l * h), st));
  GO_HIP(zero_async(der, 2 * (size_t)(n_r * h), st));
  GO_HIP(zero_async(dV, 2 * (size_t)(n_r * F), st));
  if (!slots) return GRAPHOP_OK;
  {
    ProfScope prof("gat_attn_bf16_pack", st, "k_gat_attn_bf16_pack");
    const int lanes = gat_bf16_lanes(h, d);
    GO_DISPATCH_GAT_HD(h, d, {
      hipLaunchKernelGGL((k_gat_attn_bf16_pack<H, D>), dim3((unsigned)ceil_div(n_l, (i64)(kFastBlock / lanes))),
                         dim3(kFastBlock), 0, st, (const bf16_t*)el, (const float2*)stats, (const uint4*)dO,
                         (const uint4*)o, w.P, n_l);
    });
    GO_LAUNCH_CHECK();
  }
  const float slope = (float)negative_slope;
  GO_TRY(gat_bf16_bwd_pass<false>(r, h, d, er, V, w, dO, del, nullptr, slope, drop, st));
  GO_TRY(gat_bf16_bwd_pass<true>(c, h, d, er, V, w, dO, der, dV, slope, drop, st));
  return GRAPHOP_OK;
}

}  // extern "C"
