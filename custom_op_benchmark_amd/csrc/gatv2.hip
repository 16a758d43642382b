// GATv2 attention scores (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : y[eid[j], k] = sum_c att[k, c] * LeakyReLU(xl[row[c], k, c] + xr[indices[j], k, c], negative_slope)
//   backward: dxl / datt by a row-major pass, dxr by a column-major pass (kernels_gatv2.h), z recomputed, no per-edge
//             atomics and nothing E-sized besides y and dy.
// Host-side dispatch only, in the style of gat.hip: validation, zero fills with the library's own fill kernel, and the
// choice between the fp32 fast kernels (a plan of the same arrays, the (h, d) pairs of the fused GAT layer) and the
// generic kernels (fp64, other shapes, no plan).  Checks, fast conditions, dispatch and launch geometry: host_gat.h.
#include "common.h"
#include "host.h"
#include "host_gat.h"
#include "kernels_gatv2.h"

namespace graphop {
namespace {

// power of two that covers d, a wave at most: the lanes of one head in the generic forward
inline int gatv2_dp(i64 d) { return d >= kWave ? kWave : (int)pow2ceil(d); }

}  // namespace
}  // namespace graphop

using namespace graphop;

extern "C" {

int graphop_gatv2_scores_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                 const int64_t* indices, const void* xl, const void* xr, const void* att, void* y,
                                 int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                 double negative_slope, const graphop_plan_t* plan, void* stream) {
  const char* fn = "gatv2_scores_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  hipStream_t st = (hipStream_t)stream;
  if (n_edges == 0) return GRAPHOP_OK;
  GO_PTR(fn, y);
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "xl", n_l, "xr", n_r));
  const bool covered = g.covered();
  if (!covered) GO_HIP(zero_async(y, esize(dtype) * (size_t)(n_edges * h), st));
  if (n_chunks == 0) return GRAPHOP_OK;
  GO_TRY(g.require(fn)); GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att);
  if (pm && gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att})) {
    ProfScope prof("gatv2_fwd", st, "k_gatv2_fwd_f32");
    const int cpg = gat_cpg(n_chunks, tuning().sddmm_cpg);
    GO_DISPATCH_GAT_HD(h, d, {
      hipLaunchKernelGGL((k_gatv2_fwd_f32<H, D>), dim3((unsigned)gat_grid(n_chunks, cpg)), dim3(kFastBlock), 0, st,
                         g.row, g.indptr, g.eid, g.indices, (const float*)xl,
                         (const float*)xr, (const float*)att, (float*)y, n_chunks, cpg, (float)negative_slope);
    });
  } else {
    ProfScope prof("gatv2_fwd", st, "k_gatv2_fwd_generic");
    const unsigned nb = (unsigned)ceil_div(n_chunks, kGenericWavesPerBlock);
    GO_DISPATCH_FLOAT(dtype, T, {
      hipLaunchKernelGGL((k_gatv2_fwd_generic<T>), dim3(nb), dim3(kGenericBlock), 0, st, g.row, g.indptr, g.eid,
                         g.indices, (const T*)xl, (const T*)xr, (const T*)att, (T*)y, n_chunks, h, d, gatv2_dp(d),
                         (T)negative_slope);
    });
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_gatv2_scores_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                  const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                  const int64_t* eid_c, const int64_t* indices_c, const void* xl, const void* xr,
                                  const void* att, const void* dy, void* dxl, void* dxr, void* datt, void* workspace,
                                  int64_t workspace_bytes, int64_t n_row_chunks, int64_t n_col_chunks,
                                  int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, int64_t d,
                                  double negative_slope, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                  void* stream) {
  const char* fn = "gatv2_scores_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const i64 f = h * d;
  const bool row_slots = n_edges > 0 && n_row_chunks > 0 && n_l > 0 && n_r > 0;
  const bool col_slots = n_edges > 0 && n_col_chunks > 0 && n_l > 0 && n_r > 0;
  const size_t need = row_slots ? es * (size_t)(gat_part_rows(n_row_chunks) * f) : 0;   // datt partials
  GO_CHECK_ARG(workspace_bytes >= 0 && (size_t)workspace_bytes >= need,
               "%s: workspace of %lld bytes needed (min(ceil(n_row_chunks / 16), 8192) * h * d values), got %lld", fn,
               (long long)need, (long long)workspace_bytes);
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const graphop_plan *pr = r.plan, *pc = c.plan;
  GO_TRY(gatv2_bwd_open(fn, dtype, r, c, dxl, dxr, datt, n_l, n_r, f, st));
  if (!row_slots && !col_slots) return GRAPHOP_OK;
  GO_PTR(fn, xl); GO_PTR(fn, xr); GO_PTR(fn, att); GO_PTR(fn, dy);
  if (need > 0) GO_PTR(fn, workspace);
  if (row_slots) {
    GO_TRY(r.require(fn));
    GO_PTR(fn, dxl); GO_PTR(fn, datt);
    const i64 C = n_row_chunks;
    if (pr && gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att, dxl, datt, workspace})) {
      ProfScope prof("gatv2_bwd_row", st, "k_gatv2_bwd_row_f32");
      const GatRowPass geo = gat_row_pass(C, tuning().spmm_cpg);   // n_blocks <= gat_part_rows(C)
      const bool owned = r.owned();
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, {
        hipLaunchKernelGGL((k_gatv2_bwd_row_f32<H, D, OWNED>), dim3((unsigned)geo.n_blocks), dim3(kFastBlock), 0, st,
                           r.row, r.indptr, r.eid, r.indices,
                           (const float*)xl, (const float*)xr, (const float*)att, (const float*)dy, (float*)dxl,
                           (float4*)workspace, C, geo.cpg, (float)negative_slope);
      }));
      GO_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_gatv2_datt_fin_f32, dim3((unsigned)(f / 4)), dim3(kFastBlock), 0, st,
                         (const float4*)workspace, (float4*)datt, geo.n_blocks, (int)(f / 4));
    } else {
      ProfScope prof("gatv2_bwd_row", st, "k_gatv2_bwd_row_generic");
      const unsigned nb = (unsigned)ceil_div(C, kGenericWavesPerBlock);
      GO_DISPATCH_FLOAT(dtype, T, {
        hipLaunchKernelGGL((k_gatv2_bwd_row_generic<T>), dim3(nb), dim3(kGenericBlock), 0, st, r.row, r.indptr, r.eid,
                           r.indices, (const T*)xl, (const T*)xr, (const T*)att, (const T*)dy, (T*)dxl, (T*)datt, C, h, d,
                           (T)negative_slope);
      });
    }
    GO_LAUNCH_CHECK();
  }
  if (col_slots) {
    GO_TRY(c.require(fn));
    GO_PTR(fn, dxr);
    const i64 C = n_col_chunks;
    if (pc && gat_hd_fast_ok(dtype, h, d, n_edges, n_l, n_r, {xl, xr, att, dxr})) {
      ProfScope prof("gatv2_bwd_col", st, "k_gatv2_bwd_col_f32");
      const int cpg = gat_cpg(C, tuning().spmm_cpg);
      const bool owned = c.owned();
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, {
        hipLaunchKernelGGL((k_gatv2_bwd_col_f32<H, D, OWNED>), dim3((unsigned)gat_grid(C, cpg)), dim3(kFastBlock), 0,
                           st, c.row, c.indptr, c.eid, c.indices,
                           (const float*)xl, (const float*)xr, (const float*)att, (const float*)dy, (float*)dxr, C, cpg,
                           (float)negative_slope);
      }));
    } else {
      ProfScope prof("gatv2_bwd_col", st, "k_gatv2_bwd_col_generic");
      const unsigned nb = (unsigned)ceil_div(C, kGenericWavesPerBlock);
      GO_DISPATCH_FLOAT(dtype, T, {
        hipLaunchKernelGGL((k_gatv2_bwd_col_generic<T>), dim3(nb), dim3(kGenericBlock), 0, st, c.row, c.indptr, c.eid,
                           c.indices, (const T*)xl, (const T*)xr, (const T*)att, (const T*)dy, (T*)dxr, C, h, d,
                           (T)negative_slope);
      });
    }
    GO_LAUNCH_CHECK();
  }
  return GRAPHOP_OK;
}

}  // extern "C"
