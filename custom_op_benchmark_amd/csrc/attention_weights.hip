// Attention weights of the fused dot-product attention ops (extra op, not one of the reference's eight;
// include/graphop_hip.h): a[e, k] = exp(min(s_e - m_i, 0)) * linv_i from the row statistics the fused
// forward left, with s_e = <Q_i, K_j> (+ b[e]) or <Q_i, K_j + xe[e]>.
//   plain / bias: composed inside the library -- graphop_maskedmm_csr_forward writes s into a with whatever SDDMM driver
//                 its own dispatch picks, then k_attn_weights_norm normalises a in place (one (E, h) stream pass)
//   edge        : k_attn_weights_xe_f32 (fp32, the (h, d) pairs of GO_DISPATCH_GAT_HD, a matching plan, 16-byte aligned
//                 operands), else k_attn_weights_xe_generic
// Host-side dispatch only.  No workspace and no atomics in any mode; a[e] is written once for every edge id a slot names
// and nothing else of a is touched.
#include "common.h"
#include "host.h"
#include "host_attn_rows.h"
#include "host_gat.h"
#include "kernels_attn_weights.h"

using namespace graphop;

extern "C" {

int graphop_attention_weights(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, const void* Q, const void* K, const void* stats, const void* b,
                              const void* xe, void* a, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                              int64_t h, int64_t d, const graphop_plan_t* plan, void* stream) {
  const char* fn = "attention_weights";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, dtype, n_chunks, 0, n_edges, n_q, n_k, h, d));
  GO_CHECK_ARG(b == nullptr || xe == nullptr, "%s: at most one of b and xe may be given", fn);
  const bool slots = n_chunks > 0 && n_edges > 0 && n_q > 0 && n_k > 0 && h * d > 0;
  if (slots) { GO_PTR(fn, stats); GO_PTR(fn, a); }
  hipStream_t st = (hipStream_t)stream;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "Q / stats", n_q, "K", n_k));
  if (!slots) return GRAPHOP_OK;   // nothing is written, nothing dereferenced
  GO_TRY(g.require(fn)); GO_PTR(fn, Q); GO_PTR(fn, K);

  if (xe == nullptr) {
    // s into a.  A plan that covers every edge id lets the SDDMM entry point choose among all its drivers (any fill it
    // makes is overwritten); without one the partial form runs, which fills nothing: edge ids no slot names stay as
    // the caller left them.
    if (pm && pm->info.full_coverage)
      GO_TRY(graphop_maskedmm_csr_forward(dtype, row, indptr, eid, indices, Q, K, a, n_chunks, n_edges, n_q, n_k, h, d,
                                          pm, stream));
    else
      GO_TRY(graphop_maskedmm_csr_forward_partial(dtype, row, indptr, eid, indices, Q, K, a, n_chunks, n_edges, n_edges,
                                                  n_q, n_k, h, d, stream));
    ProfScope prof("attn_weights_norm", st, "k_attn_weights_norm");
    const ChunkGeometry geo = chunk_geometry(n_chunks, kGatGroup, 16);
    const i64* ids = pm ? g.eid_or_null() : g.eid;
    const bool bias = b != nullptr;
    GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(bias, BIAS, {
      hipLaunchKernelGGL((k_attn_weights_norm<T, BIAS>), dim3(geo.blocks), dim3(kFastBlock), 0, st, g.row,
                         g.indptr, ids, (const T*)stats, (const T*)b, (T*)a, n_chunks, (i64)h, (int)geo.cpg);
    }));
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }

  if (pm && gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k, {Q, K, stats, xe, a})) {
    ProfScope prof("attn_weights_xe", st, "k_attn_weights_xe_f32");
    const int cpg = gat_cpg(n_chunks, tuning().sddmm_cpg);
    GO_DISPATCH_GAT_HD(h, d, {
      hipLaunchKernelGGL((k_attn_weights_xe_f32<H, D>), dim3((unsigned)gat_grid(n_chunks, cpg)), dim3(kFastBlock), 0, st,
                         g.row, g.indptr, g.eid_or_null(), g.indices, (const float*)Q,
                         (const float*)K, (const float*)stats, (const float*)xe, (float*)a, n_chunks, cpg);
    });
  } else {
    ProfScope prof("attn_weights_xe_generic", st, "k_attn_weights_xe_generic");
    const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
    GO_DISPATCH_FLOAT(dtype, T, {
      hipLaunchKernelGGL((k_attn_weights_xe_generic<T>), grid, dim3(kGenericBlock), 0, st, g.row,
                         g.indptr, g.eid, g.indices, (const T*)Q, (const T*)K,
                         (const T*)stats, (const T*)xe, (T*)a, n_chunks, (i64)h, (i64)d);
    });
  }
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // extern "C"
