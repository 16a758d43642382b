// Fused dot-product attention with edge-type embeddings (extra op, not one of the reference's eight;
// include/graphop_hip.h): for edge e = (i, j) of type t_e = etype[e] (by edge id), kx = K_j + R[t_e] and
// vx = V_j + R[t_e],
//   forward : o[i] = sum_e softmax_e(<Q_i, kx_e>) mult_e vx_e per head, leaving o and the row statistics
//   backward: dQ, dK, dV and dR[t] = sum_{e : t_e = t} (ds_e Q_i + a_e mult_e dO_i) from (Q, K, V, R, etype, o, stats, dO)
// etype is the only edge-sized operand; nothing else edge-sized exists, the dropout mask included.  The host side is
// attention_edge.hip's with the table where the edge rows are.  The fp32 fast kernels (kernels_attn_etype.h: the
// chunk-driver passes with the edge piece read from the table) run for the (h, d) pairs of GO_DISPATCH_GAT_HD with
// 16-byte aligned operands and matching plans; the row pass with dR sums it in LDS and so also wants
// n_types <= attn_etype_max_types(h d).  The generic kernels of the same header run for everything else, pass by pass.
// No kernel trusts a type: each clamps it into [0, n_types - 1], and nothing here scans etype (a scan would synchronise
// and break stream capture).  force_generic selects the generic kernels.  p == 0 takes the kernels without the keep
// decision.
#include "common.h"
#include "host.h"
#include "host_attn_rows.h"
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_attn_etype.h"

using namespace graphop;

namespace {

// what the fast kernels ask of the shape (the pointers are checked where they are known: gat_hd_fast_ok)
inline bool etype_shape_ok(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k) {
  return gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k, {});
}

// ONE plan of the fast kernels: neighbour ids, id ranges inside the tables (own rows n_own, gathered table n_tab)
inline bool etype_plan_ok(const graphop_plan* plan, i64 n_own, i64 n_tab) {
  return plan && plan->indices && plan->info.max_row < n_own && plan->info.max_index < n_tab;
}

// the row pass may sum dR on chip
inline bool etype_table_ok(i64 n_types, i64 F) { return n_types <= attn_etype_max_types(F); }

// fast: (K | V), (Q | dO) packed, stats4 per (row, head) and, LAST, the replicas of dR where the table fits (the size
// does not depend on whether dR is wanted); generic: P (n_q, h, 4) alone, at offset 0
struct EtypeBwdWs {
  size_t o_st4, o_kv, o_qdo, o_rep, total;
  EtypeBwdWs(bool fast, size_t es, i64 n_q, i64 n_k, i64 h, i64 F, i64 n_types) {
    o_st4 = 0;
    o_kv = o_st4 + up256(es * 4 * (size_t)(n_q * h));
    o_qdo = o_kv + (fast ? up256(sizeof(float) * (size_t)(n_k * 2 * F)) : 0);
    o_rep = o_qdo + (fast ? up256(sizeof(float) * (size_t)(n_q * 2 * F)) : 0);
    total = o_rep + (fast && etype_table_ok(n_types, F) ? rep_bytes(n_types, F) : 0);
  }
  static size_t rep_bytes(i64 n_types, i64 F) { return up256(sizeof(float) * (size_t)(kAttnEtypeReplicas * n_types * F)); }
};

// the fast forward applies to this plan and these sizes: its launch geometry and piece records
inline bool etype_fwd_fast_shape(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan,
                                 i64 n_chunks, ChunkGeometry* geo) {
  if (!etype_shape_ok(dtype, h, d, n_edges, n_q, n_k) || !etype_plan_ok(plan, n_q, n_k)) return false;
  if (!plan->info.rows_sorted || n_q >= kWalkRowMask || n_chunks == 0) return false;
  *geo = attn_rows_geometry(n_chunks);
  return 2 * geo->groups < 0x7fffffffLL;
}

inline bool etype_has_slots(i64 n_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h, i64 d) {
  return n_chunks > 0 && n_edges * h * d > 0 && n_q > 0 && n_k > 0;
}

// the checks of the table, after those of the dropout arguments
inline int etype_check(const char* fn, const void* R, const void* etype, i64 n_edges, i64 h, i64 d, i64 n_types) {
  GO_CHECK_ARG(n_types >= 0 && (n_edges == 0 || n_types >= 1), "%s: n_types must be >= 1 with n_edges > 0, got %lld", fn,
               (long long)n_types);
  GO_CHECK_ARG(n_edges * h * d == 0 || R != nullptr, "%s: R is NULL", fn);
  GO_CHECK_ARG(n_edges * h * d == 0 || etype != nullptr, "%s: etype is NULL", fn);
  return GRAPHOP_OK;
}

// rep: the replicas of dR (COL = false, NULL: dR is not wanted), n_types * F floats each
template <bool COL>
int launch_etype_rows(const char* tag, const graphop_plan* plan, const i64* eid, i64 n_chunks, i64 h, i64 d,
                      const float* own, const float* xt, const float4* st4, const float* R, const int* etype,
                      i64 n_types, float* out0, float* out1, float* rep, const AttnEtypeDrop* drop, hipStream_t st) {
  ProfScope prof(tag, st, "k_attn_etype_bwd_rows_f32");
  const bool owned = plan->info.rows_sorted != 0, dropped = drop != nullptr;
  const ChunkGeometry geo = attn_rows_geometry(n_chunks);
  const size_t lds = rep ? sizeof(float) * (size_t)(n_types * h * d) : 0;
  GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
    hipLaunchKernelGGL((k_attn_etype_bwd_rows_f32<H, D, COL, OWNED, DROP>), dim3(geo.blocks), dim3(kFastBlock), lds, st,
                       (const i64*)plan->row, (const i64*)plan->indptr, eid, (const i64*)plan->indices, own, xt, st4, R,
                       etype, (unsigned)(n_types - 1), kAttnEtypeReplicas, out0, out1, rep, n_chunks, (int)geo.cpg,
                       drop_if_arg<DROP>(drop));
  })));
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace

extern "C" {

int graphop_attention_etype_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                            int64_t d, int64_t n_types, const graphop_plan_t* plan_r,
                                            const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out) {
  const char* fn = "attention_etype_workspace_bytes";
  (void)stream;
  GO_CHECK_ARG(bytes_out != nullptr, "%s: bytes_out is NULL", fn);
  GO_CHECK_ARG(dtype == GRAPHOP_F32 || dtype == GRAPHOP_F64, "%s: bad dtype", fn);
  GO_CHECK_ARG(n_edges >= 0 && n_q >= 0 && n_k >= 0 && h >= 1 && d >= 0 && n_types >= 0, "%s: negative size", fn);
  *bytes_out = 0;
  if (n_edges * h * d == 0 || n_q == 0 || n_k == 0) return GRAPHOP_OK;
  if (!backward) {
    ChunkGeometry geo;   // the generic forward keeps its sums in stats: no workspace
    if (plan_r && etype_fwd_fast_shape(dtype, h, d, n_edges, n_q, n_k, plan_r, plan_r->info.n_chunks, &geo))
      *bytes_out = (int64_t)AttnRowsFwdWs(nullptr, 2 * geo.groups, n_q, h, h * d).total;
    return GRAPHOP_OK;
  }
  const bool fast = etype_shape_ok(dtype, h, d, n_edges, n_q, n_k) &&
                    (etype_plan_ok(plan_r, n_q, n_k) || etype_plan_ok(plan_c, n_k, n_q));
  *bytes_out = (int64_t)EtypeBwdWs(fast, esize(dtype), n_q, n_k, h, h * d, n_types).total;
  return GRAPHOP_OK;
}

int graphop_attention_etype_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                    const int64_t* indices, const void* Q, const void* K, const void* V, const void* R,
                                    const int32_t* etype, void* o, void* stats, int64_t n_chunks, int64_t n_edges,
                                    int64_t n_q, int64_t n_k, int64_t h, int64_t d, int64_t n_types, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan, void* stream, double p,
                                    uint64_t seed, uint32_t offset, int64_t head0) {
  const char* fn = "attention_etype_forward";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, dtype, n_chunks, 0, n_edges, n_q, n_k, h, d));
  HostDrop hdrop;
  GO_TRY(attn_drop_check(fn, DropIn{p, seed, offset, head0}, n_q, n_k, &hdrop));
  GO_TRY(etype_check(fn, R, etype, n_edges, h, d, n_types));
  const HostDrop* drop = p > 0.0 ? &hdrop : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const i64 F = h * d;
  const graphop_plan* pm = plan_matches_full(plan, (const i64*)row, (const i64*)indptr, (const i64*)eid,
                                             (const i64*)indices, n_chunks, n_edges) ? plan : nullptr;
  GO_TRY(gat_check_plan(fn, pm, "Q / o", n_q, "K / V", n_k));
  const bool slots = etype_has_slots(n_chunks, n_edges, n_q, n_k, h, d);
  ChunkGeometry geo{};
  bool fast = slots && !(drop && head0 + h >= 0x7fffffffLL) && n_types < 0x7fffffffLL / (F > 0 ? F : 1) &&
              etype_fwd_fast_shape(dtype, h, d, n_edges, n_q, n_k, pm, n_chunks, &geo) &&
              gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k, {Q, K, V, R, etype, o, stats, workspace});
  const AttnRowsFwdWs w(workspace, 2 * geo.groups, n_q, h, F);
  GO_TRY(attn_ws_check(fn, "attention_etype_workspace_bytes", fast, w.total, workspace, workspace_bytes));
  if (n_q == 0) return GRAPHOP_OK;
  // rows without slots keep o = 0 and stats = (-1e9, 0)
  GO_PTR(fn, stats);
  GO_DISPATCH_FLOAT(dtype, T, {
    hipLaunchKernelGGL((k_attn_etype_stats_init_generic<T>), dim3(grid_of(n_q * h)), dim3(256), 0, st, (T*)stats, n_q * h);
  });
  GO_LAUNCH_CHECK();
  if (F > 0) {
    GO_PTR(fn, o);
    GO_HIP(zero_async(o, es * (size_t)(n_q * F), st));
  }
  if (!slots) return GRAPHOP_OK;
  GO_PTR(fn, row); GO_PTR(fn, indptr); GO_PTR(fn, eid); GO_PTR(fn, indices);
  GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V);
  const bool dropped = drop != nullptr;
  const unsigned tmax = (unsigned)(n_types - 1);
  if (fast) {
    const AttnEtypeDrop hd{drop ? drop->as<float>() : DropArgs<float>{}, (int)head0};
    AttnEtypeFwdArgs a;
    a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V;
    a.R = (const float*)R; a.etype = (const int*)etype; a.tmax = tmax;
    a.o = (float*)o; a.stats = (float*)stats;
    a.p_row = w.p_row; a.p_ml = w.p_ml; a.p_o = w.p_o;
    attn_pieces_fill("attn_etype_fwd_setup", w, kAttnNegBig, st);
    GO_LAUNCH_CHECK();
    {
      ProfScope prof("attn_etype_fwd_rows", st, "k_attn_etype_fwd_rows_f32");
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((k_attn_etype_fwd_rows_f32<H, D, DROP>), dim3(geo.blocks), dim3(kFastBlock), 0, st,
                           (const i64*)pm->row, (const i64*)pm->indptr, eid_arg(pm, eid), (const i64*)pm->indices, a,
                           n_chunks, (int)geo.cpg, drop_if_arg<DROP>(drop ? &hd : nullptr));
      }));
      GO_LAUNCH_CHECK();
    }
    attn_pieces_merge(
        "attn_etype_fwd_merge", "k_attn_etype_piece_add", w, geo.lanes, st,
        [&](dim3 grid, dim3 block) {
          hipLaunchKernelGGL(k_attn_etype_piece_max, grid, block, 0, st, w.p_row, w.p_ml, w.Mtmp, w.np * h, (int)h);
        },
        [&](dim3 grid, dim3 block) {
          GO_DISPATCH_GAT_HD(h, d, {
            hipLaunchKernelGGL((k_attn_etype_piece_add<H, D>), grid, block, 0, st, w.p_row, w.p_ml, w.p_o, w.Mtmp, w.Ltmp,
                               a.o, w.np);
          });
        },
        [&](dim3 grid, dim3 block) {
          GO_DISPATCH_GAT_HD(h, d, {
            hipLaunchKernelGGL((k_attn_etype_piece_fin<H, D>), grid, block, 0, st, w.p_row, w.Mtmp, w.Ltmp, a.o, a.stats,
                               w.np);
          });
        });
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
  const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
  GO_DISPATCH_FLOAT(dtype, T, {
    {
      ProfScope prof("attn_etype_generic_stats", st, "k_attn_etype_stats_generic");
      hipLaunchKernelGGL((k_attn_etype_stats_generic<T, false>), grid, dim3(kGenericBlock), 0, st, (const i64*)row,
                         (const i64*)indptr, (const i64*)eid, (const i64*)indices, (const T*)Q, (const T*)K, (const T*)R,
                         (const int*)etype, tmax, (T*)stats, n_chunks, h, d);   // the maxima
      hipLaunchKernelGGL((k_attn_etype_stats_generic<T, true>), grid, dim3(kGenericBlock), 0, st, (const i64*)row,
                         (const i64*)indptr, (const i64*)eid, (const i64*)indices, (const T*)Q, (const T*)K, (const T*)R,
                         (const int*)etype, tmax, (T*)stats, n_chunks, h, d);   // the sums of exp(s - m)
      hipLaunchKernelGGL((k_attn_etype_stats_fin_generic<T>), dim3(grid_of(n_q * h)), dim3(256), 0, st, (T*)stats, n_q * h);
    }
    ProfScope prof("attn_etype_generic_fwd", st, "k_attn_etype_fwd_generic");
    GO_DISPATCH_BOOL(dropped, DROP, {
      hipLaunchKernelGGL((k_attn_etype_fwd_generic<T, DROP>), grid, dim3(kGenericBlock), 0, st, (const i64*)row,
                         (const i64*)indptr, (const i64*)eid, (const i64*)indices, (const T*)Q, (const T*)K, (const T*)V,
                         (const T*)R, (const int*)etype, tmax, (const T*)stats, (T*)o, n_chunks, h, d, (i64)head0,
                         drop_arg<DROP, T>(drop));
    });
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

int graphop_attention_etype_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                     const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                     const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                     const void* V, const void* R, const int32_t* etype, const void* o, const void* stats,
                                     const void* dO, void* dQ, void* dK, void* dV, void* dR, int64_t n_row_chunks,
                                     int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                                     int64_t n_types, void* workspace, int64_t workspace_bytes,
                                     const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream, double p,
                                     uint64_t seed, uint32_t offset, int64_t head0) {
  const char* fn = "attention_etype_backward";
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d));
  HostDrop hdrop;
  GO_TRY(attn_drop_check(fn, DropIn{p, seed, offset, head0}, n_q, n_k, &hdrop));
  GO_TRY(etype_check(fn, R, etype, n_edges, h, d, n_types));
  const HostDrop* drop = p > 0.0 ? &hdrop : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const i64 F = h * d;
  const graphop_plan* pr = plan_matches_full(plan_r, (const i64*)row, (const i64*)indptr_r, (const i64*)eid_r,
                                             (const i64*)indices_r, n_row_chunks, n_edges) ? plan_r : nullptr;
  const graphop_plan* pc = plan_matches_full(plan_c, (const i64*)col, (const i64*)indptr_c, (const i64*)eid_c,
                                             (const i64*)indices_c, n_col_chunks, n_edges) ? plan_c : nullptr;
  GO_TRY(gat_check_plan(fn, pr, "Q / dQ", n_q, "K / V", n_k));
  GO_TRY(gat_check_plan(fn, pc, "K / dK / dV", n_k, "Q", n_q));
  const bool row_slots = etype_has_slots(n_row_chunks, n_edges, n_q, n_k, h, d);
  const bool col_slots = etype_has_slots(n_col_chunks, n_edges, n_q, n_k, h, d);
  const bool slots = row_slots || col_slots;
  // the fast kernels: the shape, every operand 16-byte aligned, and a plan for at least one of the two passes; the row
  // pass with dR also a table that fits
  const bool ok = slots && !(drop && head0 + h >= 0x7fffffffLL) && n_types < 0x7fffffffLL / (F > 0 ? F : 1) &&
                  gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k,
                                 {Q, K, V, R, etype, o, stats, dO, dQ, dK, dV, dR, workspace});
  const bool fast_r = ok && row_slots && etype_plan_ok(pr, n_q, n_k) && (dR == nullptr || etype_table_ok(n_types, F));
  const bool fast_c = ok && col_slots && etype_plan_ok(pc, n_k, n_q);
  const EtypeBwdWs w(fast_r || fast_c, es, n_q, n_k, h, F, n_types);
  GO_TRY(attn_ws_check(fn, "attention_etype_workspace_bytes", slots, w.total, workspace, workspace_bytes));
  if (n_q * F > 0) { GO_PTR(fn, dQ); GO_HIP(zero_async(dQ, es * (size_t)(n_q * F), st)); }
  if (n_k * F > 0) {
    GO_PTR(fn, dK); GO_PTR(fn, dV);
    GO_HIP(zero_async(dK, es * (size_t)(n_k * F), st));
    GO_HIP(zero_async(dV, es * (size_t)(n_k * F), st));
  }
  // types no edge carries get dR = 0; the fast row pass writes dR from its replicas instead (below)
  if (dR != nullptr && n_types * F > 0 && !fast_r) GO_HIP(zero_async(dR, es * (size_t)(n_types * F), st));
  if (!slots) return GRAPHOP_OK;
  GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  const bool dropped = drop != nullptr;
  const unsigned tmax = (unsigned)(n_types - 1);
  const AttnEtypeDrop hd{drop ? drop->as<float>() : DropArgs<float>{}, (int)head0};
  char* base = (char*)workspace;
  void* P = base + w.o_st4;   // (m, 1 / l, D, 0) per (row, head): stats4 of the fast passes, P of the generic ones
  float* kv = (float*)(base + w.o_kv);
  float* qdo = (float*)(base + w.o_qdo);
  float* rep = fast_r && dR != nullptr ? (float*)(base + w.o_rep) : nullptr;
  if (fast_r || fast_c) {
    ProfScope prof("attn_etype_pack", st, "k_attn_etype_pack");
    constexpr int RPB = kFastBlock / kGatGroup;
    GO_DISPATCH_GAT_HD(h, d, {
      hipLaunchKernelGGL((k_attn_etype_pack<H, D, false>), dim3((unsigned)ceil_div(n_k, RPB)), dim3(kFastBlock), 0, st,
                         (const float*)K, (const float*)V, kv, n_k, (const float*)nullptr, (const float*)nullptr,
                         (float4*)nullptr);
      hipLaunchKernelGGL((k_attn_etype_pack<H, D, true>), dim3((unsigned)ceil_div(n_q, RPB)), dim3(kFastBlock), 0, st,
                         (const float*)Q, (const float*)dO, qdo, n_q, (const float*)o, (const float*)stats, (float4*)P);
    });
    GO_LAUNCH_CHECK();
  } else {
    ProfScope prof("attn_etype_generic_pack", st, "k_attn_etype_pack_generic");
    GO_DISPATCH_FLOAT(dtype, T, {
      hipLaunchKernelGGL((k_attn_etype_pack_generic<T>), dim3(grid_of(n_q * h)), dim3(256), 0, st, (const T*)stats,
                         (const T*)dO, (const T*)o, (T*)P, n_q * h, d);
    });
    GO_LAUNCH_CHECK();
  }
  if (rep) GO_HIP(zero_async(rep, EtypeBwdWs::rep_bytes(n_types, F), st));
  if (row_slots) {
    GO_PTR(fn, row); GO_PTR(fn, indptr_r); GO_PTR(fn, eid_r); GO_PTR(fn, indices_r);
    if (fast_r) {
      GO_TRY((launch_etype_rows<false>("attn_etype_rows_row", pr, eid_arg(pr, eid_r), n_row_chunks, h, d, qdo, kv,
                                       (const float4*)P, (const float*)R, (const int*)etype, n_types, (float*)dQ, nullptr,
                                       rep, drop ? &hd : nullptr, st)));
      if (rep) {
        ProfScope prof("attn_etype_dr_reduce", st, "k_attn_etype_dr_reduce");
        hipLaunchKernelGGL(k_attn_etype_dr_reduce, dim3(grid_of(n_types * F)), dim3(256), 0, st, (const float*)rep,
                           (float*)dR, (int)(n_types * F), kAttnEtypeReplicas);
        GO_LAUNCH_CHECK();
      }
    } else {
      ProfScope prof("attn_etype_generic_bwd_row", st, "k_attn_etype_bwd_row_generic");
      const dim3 grid((unsigned)ceil_div(n_row_chunks, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((k_attn_etype_bwd_row_generic<T, DROP>), grid, dim3(kGenericBlock), 0, st, (const i64*)row,
                           (const i64*)indptr_r, (const i64*)eid_r, (const i64*)indices_r, (const T*)Q, (const T*)K,
                           (const T*)V, (const T*)R, (const int*)etype, tmax, (const T*)P, (const T*)dO, (T*)dQ, (T*)dR,
                           n_row_chunks, h, d, (i64)head0, drop_arg<DROP, T>(drop));
      }));
      GO_LAUNCH_CHECK();
    }
  }
  if (col_slots) {
    GO_PTR(fn, col); GO_PTR(fn, indptr_c); GO_PTR(fn, eid_c); GO_PTR(fn, indices_c);
    if (fast_c) {
      // the column pass always reads eid_c: no eid_arg here
      GO_TRY((launch_etype_rows<true>("attn_etype_rows_col", pc, (const i64*)eid_c, n_col_chunks, h, d, kv, qdo,
                                      (const float4*)P, (const float*)R, (const int*)etype, n_types, (float*)dK,
                                      (float*)dV, nullptr, drop ? &hd : nullptr, st)));
    } else {
      ProfScope prof("attn_etype_generic_bwd_col", st, "k_attn_etype_bwd_col_generic");
      const dim3 grid((unsigned)ceil_div(n_col_chunks, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((k_attn_etype_bwd_col_generic<T, DROP>), grid, dim3(kGenericBlock), 0, st, (const i64*)col,
                           (const i64*)indptr_c, (const i64*)eid_c, (const i64*)indices_c, (const T*)Q, (const T*)K,
                           (const T*)V, (const T*)R, (const int*)etype, tmax, (const T*)P, (const T*)dO, (T*)dK, (T*)dV,
                           n_col_chunks, h, d, (i64)head0, drop_arg<DROP, T>(drop));
      }));
      GO_LAUNCH_CHECK();
    }
  }
  return GRAPHOP_OK;
}

}  // extern "C"
