// GAT additive attention scores (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : y[eid[j], k] = LeakyReLU(el[row[c], k] + er[indices[j], k], negative_slope)
//   backward: del / der by a row-major and a column-major pass (kernels_gat.h), no per-edge atomics.
// Host-side dispatch only, in the style of the operator entry points of graphop_hip.hip: validation, zero fills with
// the library's own fill kernel, and the choice between the fp32 fast kernels (with a plan of the same arrays) and the
// generic kernels (fp64, other head counts, no plan).  The checks and the launch geometry are the family's, host_gat.h.
#include "common.h"
#include "host.h"
#include "host_gat.h"
#include "kernels_gat.h"

namespace graphop {
namespace {

// fp32 fast kernels: H in {1, 2, 4, 8, 16}, ids that fit 32 bits, value arrays aligned to their item width
inline bool gat_fast_ok(int dtype, i64 h, i64 E, i64 n_l, i64 n_r, const void* p0, const void* p1, const void* p2,
                        const void* p3) {
  if (tuning().force_generic || dtype != GRAPHOP_F32) return false;
  if (h != 1 && h != 2 && h != 4 && h != 8 && h != 16) return false;
  if (E >= 0x7fffffffLL || n_l >= 0x7fffffffLL || n_r >= 0x7fffffffLL) return false;
  return gat_aligned(p0, h) && gat_aligned(p1, h) && gat_aligned(p2, h) && (!p3 || gat_aligned(p3, h));
}

#define GO_DISPATCH_GAT_H(h, ...)                 \
  switch ((int)(h)) {                             \
    case 1: { constexpr int H = 1; __VA_ARGS__; } break;   \
    case 2: { constexpr int H = 2; __VA_ARGS__; } break;   \
    case 4: { constexpr int H = 4; __VA_ARGS__; } break;   \
    case 8: { constexpr int H = 8; __VA_ARGS__; } break;   \
    case 16: { constexpr int H = 16; __VA_ARGS__; } break; \
    default: break;                               \
  }

// One backward pass (ROW: del over the row-major chunks; else der over the column-major chunks).
template <bool ROW>
int gat_bwd_pass(int dtype, const Csr& g, const void* el, const void* er, const void* dy, void* out, i64 n_l, i64 n_r,
                 i64 h, double slope, hipStream_t st) {
  const i64 *seg = g.row, *indptr = g.indptr, *eid = g.eid, *indices = g.indices;
  const i64 C = g.n_chunks;
  if (g.plan && gat_fast_ok(dtype, h, g.n_edges, n_l, n_r, el, er, dy, out)) {
    ProfScope prof(ROW ? "gat_bwd_row" : "gat_bwd_col", st, ROW ? "k_gat_bwd_row_f32" : "k_gat_bwd_col_f32");
    GO_DISPATCH_GAT_H(h, {
      constexpr int G = GatCfg<H>::G;
      const int cpg = gat_cpg(C, tuning().spmm_cpg, G);
      const unsigned nb = (unsigned)gat_grid(C, cpg, G);
      if constexpr (ROW)
        hipLaunchKernelGGL((k_gat_bwd_row_f32<H>), dim3(nb), dim3(kFastBlock), 0, st, seg, indptr, eid, indices,
                           (const float*)el, (const float*)er, (const float*)dy, (float*)out, C, cpg, (float)slope);
      else
        hipLaunchKernelGGL((k_gat_bwd_col_f32<H>), dim3(nb), dim3(kFastBlock), 0, st, seg, indptr, eid, indices,
                           (const float*)el, (const float*)er, (const float*)dy, (float*)out, C, cpg, (float)slope);
    });
  } else {
    ProfScope prof(ROW ? "gat_bwd_row" : "gat_bwd_col", st, ROW ? "k_gat_bwd_row_generic" : "k_gat_bwd_col_generic");
    const unsigned nb = (unsigned)ceil_div(C, kGenericWavesPerBlock);
    GO_DISPATCH_FLOAT(dtype, T, {
      if constexpr (ROW)
        hipLaunchKernelGGL((k_gat_bwd_row_generic<T>), dim3(nb), dim3(kGenericBlock), 0, st, seg, indptr, eid, indices,
                           (const T*)el, (const T*)er, (const T*)dy, (T*)out, C, h, (T)slope);
      else
        hipLaunchKernelGGL((k_gat_bwd_col_generic<T>), dim3(nb), dim3(kGenericBlock), 0, st, seg, indptr, eid, indices,
                           (const T*)el, (const T*)er, (const T*)dy, (T*)out, C, h, (T)slope);
    });
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace
}  // namespace graphop

using namespace graphop;

extern "C" {

int graphop_gat_scores_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                               const int64_t* indices, const void* el, const void* er, void* y, int64_t n_chunks,
                               int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, double negative_slope,
                               const graphop_plan_t* plan, void* stream) {
  const char* fn = "gat_scores_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h));
  hipStream_t st = (hipStream_t)stream;
  if (n_edges == 0) return GRAPHOP_OK;
  GO_PTR(fn, y);
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "el", n_l, "er", n_r));
  const bool covered = g.covered();
  if (!covered) GO_HIP(zero_async(y, esize(dtype) * (size_t)(n_edges * h), st));
  if (n_chunks == 0) return GRAPHOP_OK;
  GO_TRY(g.require(fn)); GO_PTR(fn, el); GO_PTR(fn, er);
  if (pm && gat_fast_ok(dtype, h, n_edges, n_l, n_r, el, er, y, nullptr)) {
    ProfScope prof("gat_fwd", st, "k_gat_fwd_f32");
    GO_DISPATCH_GAT_H(h, {
      constexpr int G = GatCfg<H>::G;
      const int cpg = gat_cpg(n_chunks, tuning().sddmm_cpg, G);
      const unsigned nb = (unsigned)gat_grid(n_chunks, cpg, G);
      hipLaunchKernelGGL((k_gat_fwd_f32<H>), dim3(nb), dim3(kFastBlock), 0, st, g.row, g.indptr, g.eid, g.indices,
                         (const float*)el, (const float*)er, (float*)y, n_chunks, cpg, (float)negative_slope);
    });
  } else {
    ProfScope prof("gat_fwd", st, "k_gat_fwd_generic");
    const unsigned nb = (unsigned)ceil_div(n_chunks, kGenericWavesPerBlock);
    if (dtype == GRAPHOP_F32)
      hipLaunchKernelGGL((k_gat_fwd_generic<float>), dim3(nb), dim3(kGenericBlock), 0, st, g.row, g.indptr, g.eid,
                         g.indices, (const float*)el, (const float*)er, (float*)y, n_chunks, h, (float)negative_slope);
    else
      hipLaunchKernelGGL((k_gat_fwd_generic<double>), dim3(nb), dim3(kGenericBlock), 0, st, g.row, g.indptr, g.eid,
                         g.indices, (const double*)el, (const double*)er, (double*)y, n_chunks, h, negative_slope);
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_gat_scores_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                const int64_t* eid_c, const int64_t* indices_c, const void* el, const void* er,
                                const void* dy, void* del, void* der, int64_t n_row_chunks, int64_t n_col_chunks,
                                int64_t n_edges, int64_t n_l, int64_t n_r, int64_t h, double negative_slope,
                                const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gat_scores_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h));
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  GO_TRY(Csr::check_bounds(fn, r.plan, "el / del", n_l, "er", n_r));
  GO_TRY(Csr::check_bounds(fn, c.plan, "er / der", n_r, "el", n_l));
  // an output whose orientation has no chunks may be NULL: that half of the op is skipped
  if (n_l > 0 && !(del == nullptr && n_row_chunks == 0)) {
    GO_PTR(fn, del);
    GO_HIP(zero_async(del, es * (size_t)(n_l * h), st));
  }
  if (n_r > 0 && !(der == nullptr && n_col_chunks == 0)) {
    GO_PTR(fn, der);
    GO_HIP(zero_async(der, es * (size_t)(n_r * h), st));
  }
  if (n_edges == 0) return GRAPHOP_OK;
  if (n_row_chunks > 0) {
    GO_TRY(r.require(fn));
    GO_PTR(fn, el); GO_PTR(fn, er); GO_PTR(fn, dy); GO_PTR(fn, del);
    GO_TRY(gat_bwd_pass<true>(dtype, r, el, er, dy, del, n_l, n_r, h, negative_slope, st));
  }
  if (n_col_chunks > 0) {
    GO_TRY(c.require(fn));
    GO_PTR(fn, el); GO_PTR(fn, er); GO_PTR(fn, dy); GO_PTR(fn, der);
    GO_TRY(gat_bwd_pass<false>(dtype, c, el, er, dy, der, n_l, n_r, h, negative_slope, st));
  }
  return GRAPHOP_OK;
}

}  // extern "C"
