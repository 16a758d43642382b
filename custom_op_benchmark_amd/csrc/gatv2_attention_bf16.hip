// The fused GATv2 attention layer on bfloat16 tables (kernels_gatv2_attn_bf16.h; include/graphop_hip.h:
// graphop_gatv2_attention_bf16_*): what is supported, the workspace layout and the launches.  One form, with and without
// attention dropout (p == 0 runs the DROP = false kernels); there is no generic path, no upcast and no knob behind it,
// so an unmet condition is an error that names it.
#include "common.h"
#include "host.h"
#include "host_bf16.h"
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_gatv2_attn_bf16.h"

using namespace graphop;

namespace graphop {

// rows without segments: stats = (-1e9, 0)
__global__ void k_gv2bf16_stats_init(float2* __restrict__ stats, i64 n) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x)
    stats[i] = make_float2(kGatv2Bf16Floor, 0.f);
}

// datt[4 q .. 4 q + 3], q = blockIdx.x: each thread sums its rows of the row pass's partials in order, then the
// workgroup's 256 sums are added in a fixed tree and the four values rounded once
__global__ __launch_bounds__(kFastBlock) void k_gv2bf16_datt_fin(const float4* __restrict__ part,
                                                                         uint2* __restrict__ datt, i64 n_part, int f4) {
  __shared__ float4 red[kFastBlock / kWave];
  const int q = blockIdx.x;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (i64 i = threadIdx.x; i < n_part; i += kFastBlock) {
    const float4 o = part[i * f4 + q];
    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
  }
  t.x = wave_sum(t.x); t.y = wave_sum(t.y); t.z = wave_sum(t.z); t.w = wave_sum(t.w);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kFastBlock / kWave; ++k) {
      t.x += red[k].x; t.y += red[k].y; t.z += red[k].z; t.w += red[k].w;
    }
    datt[q] = make_uint2(bf16_pack2(t.x, t.y), bf16_pack2(t.z, t.w));
  }
}

}  // namespace graphop

namespace {

// lanes per group of a pair of GO_DISPATCH_GAT_HD, 0 outside it
int gatv2_bf16_lanes(i64 h, i64 d) {
  int lanes = 0;
  if (h >= 1 && h <= 8 && d >= 8 && d <= 64) GO_DISPATCH_GAT_HD(h, d, { lanes = Gatv2Bf16Cfg<H, D>::L; });
  return lanes;
}

// the first unmet condition of a direction into `why`; false: supported
bool gatv2_bf16_unmet(char* why, size_t cap, bool backward, i64 h, i64 d, i64 n_edges, i64 n_l, i64 n_r,
                      const graphop_plan* plan_r, const graphop_plan* plan_c) {
  if (!gatv2_bf16_lanes(h, d)) {
    snprintf(why, cap, "(h, d) = (%lld, %lld) is not in the bfloat16 set: h in {1, 2, 4, 8}, d in {8, 16, 32, 64}, "
             "h * d in {64, 128, 256}", (long long)h, (long long)d);
    return true;
  }
  const char* name_r = backward ? "plan_r" : "plan";
  if (bf16_plan_unmet(why, cap, name_r, plan_r, n_edges, n_l, n_r)) return true;
  if (!backward && !plan_r->seg_chunk) {
    snprintf(why, cap, "%s has no segment table for the forward's segment driver", name_r);
    return true;
  }
  return backward && bf16_plan_unmet(why, cap, "plan_c", plan_c, n_edges, n_r, n_l);
}

// The backward's workspace, stated once for the query and the call (base == NULL: only `total` means anything); the
// forward needs none.
//   16 n_l h (P) + 4 max(np_r, np_c) (row words) + 4 F max(np_r, np_c) (dxl / dxr records: ONE record area for whichever
//   pass is running) + 4 F nb_r (the row pass's datt partials, a row per workgroup)
// np = 2 * lane groups of the orientation's chunk list (Bf16Geo), nb_r = the row pass's workgroups; every term is rounded
// up to 256 bytes.
struct Gatv2Bf16Ws {
  float4* P;
  unsigned* p_row;
  float *p_acc, *datt_part;
  size_t total;
  Gatv2Bf16Ws(void* base, i64 n_l, i64 h, i64 F, i64 np_r, i64 np_c, i64 nb_r) {
    Bf16Take take{(char*)base};
    const i64 np = np_r > np_c ? np_r : np_c;
    P = (float4*)take(sizeof(float4) * (size_t)(n_l * h));
    p_row = (unsigned*)take(sizeof(unsigned) * (size_t)np);
    p_acc = (float*)take(sizeof(float) * (size_t)(np * F));
    datt_part = (float*)take(sizeof(float) * (size_t)(nb_r * F));
    total = take.total;
  }
};

Gatv2Bf16Ws gatv2_bf16_ws(void* base, i64 n_row_chunks, i64 n_col_chunks, i64 n_l, i64 h, i64 d) {
  const int lanes = gatv2_bf16_lanes(h, d);
  const Bf16Geo gr(n_row_chunks, lanes);
  return Gatv2Bf16Ws(base, n_l, h, h * d, gr.np, Bf16Geo(n_col_chunks, lanes).np, gr.grid(gr.groups).x);
}

struct Gatv2Bf16Tables {
  const void *xl, *xr, *att, *dO;
};

// one backward pass over an orientation: row words, the gather kernel, the merge
template <bool COL>
int gatv2_bf16_bwd_pass(const Csr& g, i64 h, i64 d, const Gatv2Bf16Tables& t, const Gatv2Bf16Ws& w, void* out, float slope,
                        const HostDrop* drop, hipStream_t st) {
  if (g.n_chunks == 0) return GRAPHOP_OK;
  const Bf16Geo geo(g.n_chunks, gatv2_bf16_lanes(h, d));
  const Gatv2Bf16Rec rec{w.p_row, w.p_acc};
  const bool dropped = drop != nullptr;
  bf16_fill_rows("gatv2_attn_bf16_setup", w.p_row, geo.np, st);
  {
    ProfScope prof(COL ? "gatv2_attn_bf16_bwd_col" : "gatv2_attn_bf16_bwd_row", st,
                   COL ? (dropped ? "k_gv2bf16_drop_bwd_col" : "k_gv2bf16_bwd_col")
                       : (dropped ? "k_gv2bf16_drop_bwd_row" : "k_gv2bf16_bwd_row"));
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
      if constexpr (COL)
        hipLaunchKernelGGL((k_gv2bf16_bwd_col<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row,
                           g.indptr, g.indices, (const uint4*)t.xl, (const uint4*)t.xr, (const uint4*)t.att,
                           (const float4*)w.P, (const uint4*)t.dO, (uint4*)out, rec, g.n_chunks, (int)geo.cpg, slope,
                           drop_arg<DROP, float>(drop));
      else
        hipLaunchKernelGGL((k_gv2bf16_bwd_row<H, D, DROP>), geo.grid(geo.groups), dim3(kFastBlock), 0, st, g.row,
                           g.indptr, g.indices, (const uint4*)t.xl, (const uint4*)t.xr, (const uint4*)t.att,
                           (const float4*)w.P, (const uint4*)t.dO, (uint4*)out, rec, w.datt_part, g.n_chunks, (int)geo.cpg,
                           slope, drop_arg<DROP, float>(drop));
    }));
    GO_LAUNCH_CHECK();
  }
  ProfScope prof("gatv2_attn_bf16_bwd_merge", st, "k_gv2bf16_bwd_merge");
  GO_DISPATCH_GAT_HD(h, d, {
    hipLaunchKernelGGL((k_gv2bf16_bwd_merge<H, D>), geo.grid(geo.np), dim3(kFastBlock), 0, st, rec, (uint4*)out,
                       geo.np);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace

extern "C" {

int graphop_gatv2_attention_bf16_workspace_bytes(int backward, int64_t n_row_chunks, int64_t n_col_chunks,
                                                 int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                                 const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                                 int64_t* bytes_out) {
  const char* fn = "gatv2_attention_bf16_workspace_bytes";
  GO_PTR(fn, bytes_out);
  *bytes_out = 0;
  GO_TRY(gat_check(fn, GRAPHOP_F32, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  char why[256];
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || n_col_chunks > 0) && n_l > 0 && n_r > 0;
  if (!backward || !slots || gatv2_bf16_unmet(why, sizeof(why), true, h, d, n_edges, n_l, n_r, plan_r, plan_c) ||
      plan_r->info.n_chunks != n_row_chunks || plan_c->info.n_chunks != n_col_chunks)
    return GRAPHOP_OK;   // the forward keeps everything in registers and LDS
  *bytes_out = (int64_t)gatv2_bf16_ws(nullptr, n_row_chunks, n_col_chunks, n_l, h, d).total;
  return GRAPHOP_OK;
}

int graphop_gatv2_attention_bf16_forward(const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                         const int64_t* indices, const void* xl, const void* xr, const void* att, void* o,
                                         void* stats, void* workspace, int64_t workspace_bytes, int64_t n_chunks,
                                         int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                         double negative_slope, double p, uint64_t seed, uint32_t offset,
                                         const graphop_plan_t* plan, void* stream) {
  const char* fn = "gatv2_attention_bf16_forward";
  (void)workspace; (void)workspace_bytes;   // the forward needs none
  GO_TRY(gat_check(fn, GRAPHOP_F32, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &hd));
  const HostDrop* drop = p > 0.0 ? &hd : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  GO_TRY(Csr::check_bounds(fn, g.plan, "xl / o", n_l, "xr", n_r));
  if (n_l == 0) return GRAPHOP_OK;
  GO_PTR(fn, o); GO_PTR(fn, stats);
  GO_CHECK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", fn);
  const i64 F = h * d;
  const bool slots = n_chunks > 0 && n_edges > 0 && n_r > 0;
  if (slots) {
    char why[256];
    GO_CHECK_ARG(!gatv2_bf16_unmet(why, sizeof(why), false, h, d, n_edges, n_l, n_r, g.plan, nullptr),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_TRY(g.require(fn));
    GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att);
    GO_TRY(bf16_tables_aligned(fn, {xl, xr, att, o}));
  }
  // rows without segments keep o = 0 and stats = (-1e9, 0)
  GO_HIP(zero_async(o, 2 * (size_t)(n_l * F), st));
  hipLaunchKernelGGL(k_gv2bf16_stats_init, dim3(grid_of(n_l * h)), dim3(256), 0, st, (float2*)stats, n_l * h);
  GO_LAUNCH_CHECK();
  if (!slots) return GRAPHOP_OK;
  const graphop_plan* pm = g.plan;
  const i64 S = pm->info.n_segments;
  if (S == 0) return GRAPHOP_OK;
  const int lanes = gatv2_bf16_lanes(h, d);
  const int n_long = (int)pm->n_long;
  const i64 long_len = n_long > 0 ? kLongSegment : ((i64)1 << 62);
  const unsigned nbs = (unsigned)ceil_div(S, (i64)(kFastBlock / lanes));
  const Gatv2Bf16FwdArgs a{(const uint4*)xl, (const uint4*)xr, (const uint4*)att, (uint4*)o, (float2*)stats};
  const bool dropped = drop != nullptr;
  ProfScope prof("gatv2_attn_bf16_fwd", st, dropped ? "k_gv2bf16_drop_fwd" : "k_gv2bf16_fwd");
  GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
    hipLaunchKernelGGL((k_gv2bf16_fwd<H, D, DROP>), dim3(nbs + (unsigned)n_long), dim3(kFastBlock), 0, st, g.row,
                       g.indptr, g.indices, (const i64*)pm->seg_chunk, a, S, nbs, long_len, (const int*)pm->long_segs,
                       (float)negative_slope, drop_arg<DROP, float>(drop));
  }));
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_gatv2_attention_bf16_backward(const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                          const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                          const int64_t* eid_c, const int64_t* indices_c, const void* xl, const void* xr,
                                          const void* att, const void* o, const void* stats, const void* dO, void* dxl,
                                          void* dxr, void* datt, void* workspace, int64_t workspace_bytes,
                                          int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                          int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                          uint64_t seed, uint32_t offset, const graphop_plan_t* plan_r,
                                          const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gatv2_attention_bf16_backward";
  GO_TRY(gat_check(fn, GRAPHOP_F32, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop hd;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &hd));
  const HostDrop* drop = p > 0.0 ? &hd : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  GO_TRY(Csr::check_bounds(fn, r.plan, "xl / dxl", n_l, "xr", n_r));
  GO_TRY(Csr::check_bounds(fn, c.plan, "xr / dxr", n_r, "xl", n_l));
  const i64 F = h * d;
  if (n_l > 0) GO_PTR(fn, dxl);
  if (n_r > 0) GO_PTR(fn, dxr);
  GO_PTR(fn, datt);
  const bool slots = n_edges > 0 && (n_row_chunks > 0 || n_col_chunks > 0) && n_l > 0 && n_r > 0;
  Gatv2Bf16Ws w(nullptr, 0, 0, 0, 0, 0, 0);
  if (slots) {
    char why[256];
    GO_CHECK_ARG(!gatv2_bf16_unmet(why, sizeof(why), true, h, d, n_edges, n_l, n_r, r.plan, c.plan),
                 "%s: bfloat16 unsupported: %s", fn, why);
    GO_TRY(r.require(fn));
    GO_TRY(c.require(fn));
    GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
    GO_TRY(bf16_tables_aligned(fn, {xl, xr, att, o, dO, dxl, dxr, datt}));
    GO_CHECK_ARG(((uintptr_t)stats & 7) == 0, "%s: stats must be 8-byte aligned", fn);
    w = gatv2_bf16_ws(workspace, n_row_chunks, n_col_chunks, n_l, h, d);
    GO_TRY(attn_ws_check(fn, "gatv2_attention_bf16_workspace_bytes", true, w.total, workspace, workspace_bytes));
  }
  // rows and columns without chunks read 0; so does datt where no row chunk exists
  GO_HIP(zero_async(dxl, 2 * (size_t)(n_l * F), st));
  GO_HIP(zero_async(dxr, 2 * (size_t)(n_r * F), st));
  GO_HIP(zero_async(datt, 2 * (size_t)F, st));
  if (!slots) return GRAPHOP_OK;
  const int lanes = gatv2_bf16_lanes(h, d);
  {
    ProfScope prof("gatv2_attn_bf16_pack", st, "k_gv2bf16_pack");
    GO_DISPATCH_GAT_HD(h, d, {
      hipLaunchKernelGGL((k_gv2bf16_pack<H, D>), dim3((unsigned)ceil_div(n_l, (i64)(kFastBlock / lanes))),
                         dim3(kFastBlock), 0, st, (const float2*)stats, (const uint4*)dO, (const uint4*)o, w.P, n_l);
    });
    GO_LAUNCH_CHECK();
  }
  const float slope = (float)negative_slope;
  const Gatv2Bf16Tables t{xl, xr, att, dO};
  GO_TRY(gatv2_bf16_bwd_pass<false>(r, h, d, t, w, dxl, slope, drop, st));
  if (n_row_chunks > 0) {
    const Bf16Geo geo(n_row_chunks, lanes);
    ProfScope prof("gatv2_attn_bf16_datt_fin", st, "k_gv2bf16_datt_fin");
    hipLaunchKernelGGL(k_gv2bf16_datt_fin, dim3((unsigned)(F / 4)), dim3(kFastBlock), 0, st,
                       (const float4*)w.datt_part, (uint2*)datt, (i64)geo.grid(geo.groups).x, (int)(F / 4));
    GO_LAUNCH_CHECK();
  }
  GO_TRY(gatv2_bf16_bwd_pass<true>(c, h, d, t, w, dxr, slope, drop, st));
  return GRAPHOP_OK;
}

}  // extern "C"
