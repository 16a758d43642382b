// Fused GATv2 attention (extra op, not one of the reference's eight; include/graphop_hip.h):
//   forward : o[i] = sum_j softmax_j(att . LeakyReLU(xl[i] + xr[j])) xr[j] per head, leaving only o and the row statistics
//   backward: dxl, dxr, datt from (xl, xr, att, o, stats, dO), z, s and a recomputed per slot (kernels_gatv2_attn.h).
// No E-sized tensor exists in either direction.  Host-side dispatch in the style of gatv2.hip and gat_attention.hip:
// validation, fills, and the choice between the fp32 fast kernels (a plan of the same arrays, the (h, d) pairs of the
// fused GAT layer, ids below 2^31, 16-byte-aligned tables) and the generic ones (fp64, other shapes, NULL plans; the
// forward also where the plan is not row_owned).  Checks, fast conditions, dispatch and launch geometry: host_gat.h; the
// op itself: host_gatv2_attn_ops.h, here with EDGE = false (gatv2_edge_attention.hip is the same op with the edge row).
// The *_dropout_* entry points are the same op with attention dropout (kernels_dropout.h: the keep decision of an edge
// is recomputed from Philox in each gather pass, so still no E-sized tensor); p == 0 is the op without it.
#include "common.h"
#include "host.h"
#include "host_gatv2_attn_ops.h"

using namespace graphop;

namespace graphop {

// datt[p] = sum over the n_part rows of the row pass's partials, piece p = blockIdx.x: each thread sums its rows in
// order, then the workgroup's 256 sums are added in a fixed tree
__global__ __launch_bounds__(kFastBlock) void k_gv2attn_datt_fin_f32(const float4* __restrict__ part,
                                                                     float4* __restrict__ datt, i64 n_part, int f4) {
  __shared__ float4 red[kFastBlock / kWave];
  const int p = blockIdx.x;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (i64 i = threadIdx.x; i < n_part; i += kFastBlock) {
    const float4 o = part[i * f4 + p];
    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
  }
  t.x = wave_sum(t.x); t.y = wave_sum(t.y); t.z = wave_sum(t.z); t.w = wave_sum(t.w);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < kFastBlock / kWave; ++q) {
      t.x += red[q].x; t.y += red[q].y; t.z += red[q].z; t.w += red[q].w;
    }
    datt[p] = t;
  }
}

void gv2attn_datt_fin(const void* part, void* datt, i64 n_part, i64 f4, hipStream_t st) {
  hipLaunchKernelGGL(k_gv2attn_datt_fin_f32, dim3((unsigned)f4), dim3(kFastBlock), 0, st, (const float4*)part,
                     (float4*)datt, n_part, (int)f4);
}

}  // namespace graphop

extern "C" {

int graphop_gatv2_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* xl, const void* xr, const void* att, void* o,
                                    void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                    int64_t h, int64_t d, double negative_slope, const graphop_plan_t* plan,
                                    void* stream) {
  const char* fn = "gatv2_attention_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  return gv2attn_forward<false>(fn, dtype, row, indptr, eid, indices, xl, xr, nullptr, att, o, stats, n_chunks, n_edges,
                                n_l, n_r, h, d, negative_slope, nullptr, plan, stream);
}

int graphop_gatv2_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* xl, const void* xr,
                                     const void* att, const void* o, const void* stats, const void* dO, void* dxl,
                                     void* dxr, void* datt, void* workspace, int64_t workspace_bytes,
                                     int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_l,
                                     int64_t n_r, int64_t h, int64_t d, double negative_slope,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gatv2_attention_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  return gv2attn_backward<false>(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr,
                                 nullptr, att, o, stats, dO, dxl, dxr, nullptr, datt, workspace, workspace_bytes,
                                 n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d, negative_slope, nullptr, plan_r,
                                 plan_c, stream);
}

// p == 0 runs the kernels of the entry points above: bit-identical results
int graphop_gatv2_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                            const int64_t* indices, const void* xl, const void* xr, const void* att,
                                            void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_l,
                                            int64_t n_r, int64_t h, int64_t d, double negative_slope, double p,
                                            uint64_t seed, uint32_t offset, const graphop_plan_t* plan, void* stream) {
  const char* fn = "gatv2_attention_dropout_forward";
  GO_TRY(gat_check(fn, dtype, n_chunks, 0, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gv2attn_forward<false>(fn, dtype, row, indptr, eid, indices, xl, xr, nullptr, att, o, stats, n_chunks, n_edges,
                                n_l, n_r, h, d, negative_slope, p > 0.0 ? &drop : nullptr, plan, stream);
}

int graphop_gatv2_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                                             const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                                             const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                                             const void* xl, const void* xr, const void* att, const void* o,
                                             const void* stats, const void* dO, void* dxl, void* dxr, void* datt,
                                             void* workspace, int64_t workspace_bytes, int64_t n_row_chunks,
                                             int64_t n_col_chunks, int64_t n_edges, int64_t n_l, int64_t n_r,
                                             int64_t h, int64_t d, double negative_slope, double p, uint64_t seed,
                                             uint32_t offset, const graphop_plan_t* plan_r,
                                             const graphop_plan_t* plan_c, void* stream) {
  const char* fn = "gatv2_attention_dropout_backward";
  GO_TRY(gat_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d));
  HostDrop drop;
  GO_TRY(drop_check(fn, p, seed, n_l, n_r, offset, &drop));
  return gv2attn_backward<false>(fn, dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c, xl, xr,
                                 nullptr, att, o, stats, dO, dxl, dxr, nullptr, datt, workspace, workspace_bytes,
                                 n_row_chunks, n_col_chunks, n_edges, n_l, n_r, h, d, negative_slope,
                                 p > 0.0 ? &drop : nullptr, plan_r, plan_c, stream);
}

}  // extern "C"
