// The workspace query, the forward and the backward of the fused dot-product attention ops that add a per-edge row to
// the key and the value, behind the entry points of attention_edge.hip (the row is xe[e]) and
// attention_etype.hip (the row is R[etype[e]]; 4.5o), and of the op that adds a per-type scalar to the score instead,
// behind those of attention_tbias.hip (the "row" is the h words B[etype[e], :]; 4.5p: that form carries h in its Rows
// and ignores the F = h d it is handed).  One implementation: the checks and their order, the early
// returns, the fast / generic decisions, the workspace layouts, the zero fills and the sequence of launches are the same
// for all.  Each form's kernel header emits kernels without a template, so it belongs to its own translation unit and
// is not included here: the including unit describes its form in a struct F and this text is a template over it.
// A form states
//   GO_ATTN_EDGE_FORM_NAMES(edge, Edge)   its kernels, its record types (Drop, FwdArgs), its profile tags and labels;
//   Rows                                  the operands that bring the edge rows and take their gradient, as they arrive;
//   check(fn, x, n_edges, h, d)           the argument checks of Rows, made after those of the dropout arguments;
//   fast_ok(x, F, backward)               what the fast kernels ask of Rows beyond gat_hd_fast_ok;
//   row_fast_ok(x, F)                     what the fast row pass asks on top;
//   ws_tail(x, F)                         bytes the fast backward keeps after (stats4, K | V, Q | dO);
//   grad_fill(x, es, F, fast_r, st)       the zero fill the rows' gradient needs here (not in the binding);
//   set_fwd(a, x)                         Rows in the fast forward's argument record;
//   rows_args(x), generic_args<T>(x)      Rows in the parameter lists of the chunk-driver passes and the generic kernels;
//   row_grad(x, fast_r, tail), grad(x)    the gradient argument of the fast row pass (tail: its ws_tail) and of the
//                                         generic one; row_lds(x, g, F) the fast row pass's dynamic LDS;
//   row_open / row_close(x, g, F, st)     what runs before and after the fast row pass for g = row_grad(...).
// A translation unit instantiates only its own form, so only its own kernels.  Not part of the C ABI.
#pragma once
#include <tuple>

#include "host_attn_rows.h"
#include "host_dropout.h"
#include "host_gat.h"

namespace graphop {

struct AttnEdgeLabel {
  const char *tag, *kernel;   // of a ProfScope
};

#define GO_ATTN_EDGE_LABEL(p, tag, kernel) {"attn_" #p "_" tag, "k_attn_" #p "_" kernel}
#define GO_ATTN_EDGE_FORM_NAMES(p, P)                                                                                  \
  using Drop = Attn##P##Drop;                                                                                          \
  using FwdArgs = Attn##P##FwdArgs;                                                                                    \
  static constexpr const char* query = "attention_" #p "_workspace_bytes";                                             \
  static constexpr const char* l_fwd_setup = "attn_" #p "_fwd_setup";                                                  \
  static constexpr AttnEdgeLabel l_fwd_rows = GO_ATTN_EDGE_LABEL(p, "fwd_rows", "fwd_rows_f32");                       \
  static constexpr AttnEdgeLabel l_fwd_merge = GO_ATTN_EDGE_LABEL(p, "fwd_merge", "piece_add");                        \
  static constexpr AttnEdgeLabel l_generic_stats = GO_ATTN_EDGE_LABEL(p, "generic_stats", "stats_generic");            \
  static constexpr AttnEdgeLabel l_generic_fwd = GO_ATTN_EDGE_LABEL(p, "generic_fwd", "fwd_generic");                  \
  static constexpr AttnEdgeLabel l_pack = GO_ATTN_EDGE_LABEL(p, "pack", "pack");                                       \
  static constexpr AttnEdgeLabel l_generic_pack = GO_ATTN_EDGE_LABEL(p, "generic_pack", "pack_generic");               \
  static constexpr AttnEdgeLabel l_rows_row = GO_ATTN_EDGE_LABEL(p, "rows_row", "bwd_rows_f32");                       \
  static constexpr AttnEdgeLabel l_rows_col = GO_ATTN_EDGE_LABEL(p, "rows_col", "bwd_rows_f32");                       \
  static constexpr AttnEdgeLabel l_generic_bwd_row = GO_ATTN_EDGE_LABEL(p, "generic_bwd_row", "bwd_row_generic");      \
  static constexpr AttnEdgeLabel l_generic_bwd_col = GO_ATTN_EDGE_LABEL(p, "generic_bwd_col", "bwd_col_generic");      \
  template <int H, int D, bool DROP> static constexpr auto fwd_rows = &k_attn_##p##_fwd_rows_f32<H, D, DROP>;          \
  static constexpr auto piece_max = &k_attn_##p##_piece_max;                                                           \
  template <int H, int D> static constexpr auto piece_add = &k_attn_##p##_piece_add<H, D>;                             \
  template <int H, int D> static constexpr auto piece_fin = &k_attn_##p##_piece_fin<H, D>;                             \
  template <int H, int D, bool STATS> static constexpr auto pack = &k_attn_##p##_pack<H, D, STATS>;                    \
  template <int H, int D, bool COL, bool OWNED, bool DROP>                                                             \
  static constexpr auto bwd_rows = &k_attn_##p##_bwd_rows_f32<H, D, COL, OWNED, DROP>;                                 \
  template <class T> static constexpr auto stats_init = &k_attn_##p##_stats_init_generic<T>;                           \
  template <class T> static constexpr auto stats_fin = &k_attn_##p##_stats_fin_generic<T>;                             \
  template <class T, bool SUM> static constexpr auto stats = &k_attn_##p##_stats_generic<T, SUM>;                      \
  template <class T, bool DROP> static constexpr auto fwd = &k_attn_##p##_fwd_generic<T, DROP>;                        \
  template <class T> static constexpr auto pack_generic = &k_attn_##p##_pack_generic<T>;                               \
  template <class T, bool DROP> static constexpr auto bwd_row = &k_attn_##p##_bwd_row_generic<T, DROP>;                \
  template <class T, bool DROP> static constexpr auto bwd_col = &k_attn_##p##_bwd_col_generic<T, DROP>

// what the fast kernels ask of the shape (the pointers are checked where they are known: gat_hd_fast_ok)
inline bool attn_edge_shape_ok(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k) {
  return gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k, {});
}

// ONE plan of the fast kernels: neighbour ids, id ranges inside the tables (own rows n_own, gathered table n_tab)
inline bool attn_edge_plan_ok(const graphop_plan* plan, i64 n_own, i64 n_tab) {
  return plan && plan->indices && plan->info.max_row < n_own && plan->info.max_index < n_tab;
}

// fast: (K | V), (Q | dO) packed, stats4 per (row, head) and, LAST, the form's tail; generic: P (n_q, h, 4) alone, at
// offset 0
struct AttnEdgeBwdWs {
  size_t o_st4, o_kv, o_qdo, o_tail, total;
  AttnEdgeBwdWs(bool fast, size_t es, i64 n_q, i64 n_k, i64 h, i64 F, size_t tail) {
    o_st4 = 0;
    o_kv = o_st4 + up256(es * 4 * (size_t)(n_q * h));
    o_qdo = o_kv + (fast ? up256(sizeof(float) * (size_t)(n_k * 2 * F)) : 0);
    o_tail = o_qdo + (fast ? up256(sizeof(float) * (size_t)(n_q * 2 * F)) : 0);
    total = o_tail + (fast ? tail : 0);
  }
};

// the fast forward applies to this plan and these sizes: its launch geometry and piece records
inline bool attn_edge_fwd_fast_shape(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan,
                                     i64 n_chunks, ChunkGeometry* geo) {
  if (!attn_edge_shape_ok(dtype, h, d, n_edges, n_q, n_k) || !attn_edge_plan_ok(plan, n_q, n_k)) return false;
  if (!plan->info.rows_sorted || n_q >= kWalkRowMask || n_chunks == 0) return false;
  *geo = attn_rows_geometry(n_chunks);
  return 2 * geo->groups < 0x7fffffffLL;
}

inline bool attn_edge_has_slots(i64 n_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h, i64 d) {
  return n_chunks > 0 && n_edges * h * d > 0 && n_q > 0 && n_k > 0;
}

// x: Rows with the sizes the form's ws_tail reads; fn names the entry point
template <class F>
int attn_edge_workspace_bytes(const char* fn, int dtype, int backward, i64 n_edges, i64 n_q, i64 n_k, i64 h, i64 d,
                              bool sizes_ok, const typename F::Rows& x, const graphop_plan* plan_r,
                              const graphop_plan* plan_c, int64_t* bytes_out) {
  GO_CHECK_ARG(bytes_out != nullptr, "%s: bytes_out is NULL", fn);
  GO_CHECK_ARG(dtype == GRAPHOP_F32 || dtype == GRAPHOP_F64, "%s: bad dtype", fn);
  GO_CHECK_ARG(n_edges >= 0 && n_q >= 0 && n_k >= 0 && h >= 1 && d >= 0 && sizes_ok, "%s: negative size", fn);
  *bytes_out = 0;
  if (n_edges * h * d == 0 || n_q == 0 || n_k == 0) return GRAPHOP_OK;
  if (!backward) {
    ChunkGeometry geo;   // the generic forward keeps its sums in stats: no workspace
    if (plan_r && attn_edge_fwd_fast_shape(dtype, h, d, n_edges, n_q, n_k, plan_r, plan_r->info.n_chunks, &geo))
      *bytes_out = (int64_t)AttnRowsFwdWs(nullptr, 2 * geo.groups, n_q, h, h * d).total;
    return GRAPHOP_OK;
  }
  const bool fast = attn_edge_shape_ok(dtype, h, d, n_edges, n_q, n_k) &&
                    (attn_edge_plan_ok(plan_r, n_q, n_k) || attn_edge_plan_ok(plan_c, n_k, n_q));
  *bytes_out = (int64_t)AttnEdgeBwdWs(fast, esize(dtype), n_q, n_k, h, h * d, F::ws_tail(x, h * d)).total;
  return GRAPHOP_OK;
}

template <class F>
int attn_edge_forward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                      const int64_t* indices, const void* Q, const void* K, const void* V, const typename F::Rows& x,
                      void* o, void* stats, i64 n_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h, i64 d, void* workspace,
                      i64 workspace_bytes, const graphop_plan* plan, void* stream, const DropIn& din) {
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, dtype, n_chunks, 0, n_edges, n_q, n_k, h, d));
  HostDrop hdrop;
  GO_TRY(attn_drop_check(fn, din, n_q, n_k, &hdrop));
  GO_TRY(F::check(fn, x, n_edges, h, d));
  const HostDrop* drop = din.p > 0.0 ? &hdrop : nullptr;
  const i64 head0 = din.head0;
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const i64 Fd = h * d;
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  GO_TRY(Csr::check_bounds(fn, pm, "Q / o", n_q, "K / V", n_k));
  const bool slots = attn_edge_has_slots(n_chunks, n_edges, n_q, n_k, h, d);
  ChunkGeometry geo{};
  bool fast = slots && !(drop && head0 + h >= 0x7fffffffLL) && F::fast_ok(x, Fd, false) &&
              attn_edge_fwd_fast_shape(dtype, h, d, n_edges, n_q, n_k, pm, n_chunks, &geo) &&
              gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k, {Q, K, V, o, stats, workspace});
  const AttnRowsFwdWs w(workspace, 2 * geo.groups, n_q, h, Fd);
  GO_TRY(attn_ws_check(fn, F::query, fast, w.total, workspace, workspace_bytes));
  if (n_q == 0) return GRAPHOP_OK;
  // rows without slots keep o = 0 and stats = (-1e9, 0)
  GO_PTR(fn, stats);
  GO_DISPATCH_FLOAT(dtype, T, {
    hipLaunchKernelGGL(F::template stats_init<T>, dim3(grid_of(n_q * h)), dim3(256), 0, st, (T*)stats, n_q * h);
  });
  GO_LAUNCH_CHECK();
  if (Fd > 0) {
    GO_PTR(fn, o);
    GO_HIP(zero_async(o, es * (size_t)(n_q * Fd), st));
  }
  if (!slots) return GRAPHOP_OK;
  GO_TRY(g.require(fn));
  GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V);
  const bool dropped = drop != nullptr;
  if (fast) {
    const typename F::Drop hd{drop ? drop->as<float>() : DropArgs<float>{}, (int)head0};
    typename F::FwdArgs a;
    a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V;
    F::set_fwd(a, x);
    a.o = (float*)o; a.stats = (float*)stats;
    a.p_row = w.p_row; a.p_ml = w.p_ml; a.p_o = w.p_o;
    attn_pieces_fill(F::l_fwd_setup, w, kAttnNegBig, st);
    GO_LAUNCH_CHECK();
    {
      ProfScope prof(F::l_fwd_rows.tag, st, F::l_fwd_rows.kernel);
      GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, {
        hipLaunchKernelGGL((F::template fwd_rows<H, D, DROP>), dim3(geo.blocks), dim3(kFastBlock), 0, st,
                           g.row, g.indptr, g.eid_or_null(), g.indices, a,
                           n_chunks, (int)geo.cpg, drop_if_arg<DROP>(drop ? &hd : nullptr));
      }));
      GO_LAUNCH_CHECK();
    }
    attn_pieces_merge(
        F::l_fwd_merge.tag, F::l_fwd_merge.kernel, w, geo.lanes, st,
        [&](dim3 grid, dim3 block) {
          hipLaunchKernelGGL(F::piece_max, grid, block, 0, st, w.p_row, w.p_ml, w.Mtmp, w.np * h, (int)h);
        },
        [&](dim3 grid, dim3 block) {
          GO_DISPATCH_GAT_HD(h, d, {
            hipLaunchKernelGGL((F::template piece_add<H, D>), grid, block, 0, st, w.p_row, w.p_ml, w.p_o, w.Mtmp, w.Ltmp,
                               a.o, w.np);
          });
        },
        [&](dim3 grid, dim3 block) {
          GO_DISPATCH_GAT_HD(h, d, {
            hipLaunchKernelGGL((F::template piece_fin<H, D>), grid, block, 0, st, w.p_row, w.Mtmp, w.Ltmp, a.o, a.stats,
                               w.np);
          });
        });
    GO_LAUNCH_CHECK();
    return GRAPHOP_OK;
  }
  const dim3 grid((unsigned)ceil_div(n_chunks, kGenericWavesPerBlock));
  GO_DISPATCH_FLOAT(dtype, T, {
    {
      ProfScope prof(F::l_generic_stats.tag, st, F::l_generic_stats.kernel);
      auto pass = [&](auto sum) {
        go_launch((F::template stats<T, decltype(sum)::value>), grid, dim3(kGenericBlock), st, g.row,
                  g.indptr, g.eid, g.indices, (const T*)Q, (const T*)K,
                  F::template generic_args<T>(x), (T*)stats, n_chunks, h, d);
      };
      pass(std::false_type{});   // the maxima
      pass(std::true_type{});    // the sums of exp(s - m)
      hipLaunchKernelGGL(F::template stats_fin<T>, dim3(grid_of(n_q * h)), dim3(256), 0, st, (T*)stats, n_q * h);
    }
    ProfScope prof(F::l_generic_fwd.tag, st, F::l_generic_fwd.kernel);
    GO_DISPATCH_BOOL(dropped, DROP, {
      go_launch((F::template fwd<T, DROP>), grid, dim3(kGenericBlock), st, g.row, g.indptr,
                g.eid, g.indices, (const T*)Q, (const T*)K, (const T*)V,
                F::template generic_args<T>(x), (const T*)stats, (T*)o, n_chunks, h, d, (i64)head0,
                drop_arg<DROP, T>(drop));
    });
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

// one fast chunk-driver pass of the backward; grad: the rows' gradient argument of the row pass (COL = false), NULL
// where it is not wanted and in the column pass
template <class F, bool COL>
int attn_edge_launch_rows(const AttnEdgeLabel& lab, const Csr& g, const i64* eid, i64 h, i64 d, const float* own,
                          const float* xt, const float4* st4, const typename F::Rows& x, float* out0, float* out1,
                          float* grad, const typename F::Drop* drop, hipStream_t st) {
  ProfScope prof(lab.tag, st, lab.kernel);
  const bool owned = g.owned(), dropped = drop != nullptr;
  const i64 n_chunks = g.n_chunks;
  const ChunkGeometry geo = attn_rows_geometry(n_chunks);
  const size_t lds = F::row_lds(x, grad, h * d);
  GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, {
    go_launch_lds((F::template bwd_rows<H, D, COL, OWNED, DROP>), dim3(geo.blocks), dim3(kFastBlock), lds, st,
                  g.row, g.indptr, eid, g.indices, own, xt, st4,
                  F::rows_args(x), out0, out1, grad, n_chunks, (int)geo.cpg, drop_if_arg<DROP>(drop));
  })));
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

template <class F>
int attn_edge_backward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                       const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c, const int64_t* eid_c,
                       const int64_t* indices_c, const void* Q, const void* K, const void* V,
                       const typename F::Rows& x, const void* o, const void* stats, const void* dO, void* dQ, void* dK,
                       void* dV, i64 n_row_chunks, i64 n_col_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h, i64 d,
                       void* workspace, i64 workspace_bytes, const graphop_plan* plan_r, const graphop_plan* plan_c,
                       void* stream, const DropIn& din) {
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d));
  HostDrop hdrop;
  GO_TRY(attn_drop_check(fn, din, n_q, n_k, &hdrop));
  GO_TRY(F::check(fn, x, n_edges, h, d));
  const HostDrop* drop = din.p > 0.0 ? &hdrop : nullptr;
  const i64 head0 = din.head0;
  hipStream_t st = (hipStream_t)stream;
  const size_t es = esize(dtype);
  const i64 Fd = h * d;
  const Csr r(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr c(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const graphop_plan *pr = r.plan, *pc = c.plan;
  GO_TRY(Csr::check_bounds(fn, pr, "Q / dQ", n_q, "K / V", n_k));
  GO_TRY(Csr::check_bounds(fn, pc, "K / dK / dV", n_k, "Q", n_q));
  const bool row_slots = attn_edge_has_slots(n_row_chunks, n_edges, n_q, n_k, h, d);
  const bool col_slots = attn_edge_has_slots(n_col_chunks, n_edges, n_q, n_k, h, d);
  const bool slots = row_slots || col_slots;
  // the fast kernels: the shape, every operand 16-byte aligned, and a plan for at least one of the two passes; the row
  // pass also what the form asks of it
  const bool ok = slots && !(drop && head0 + h >= 0x7fffffffLL) && F::fast_ok(x, Fd, true) &&
                  gat_hd_fast_ok(dtype, h, d, n_edges, n_q, n_k, {Q, K, V, o, stats, dO, dQ, dK, dV, workspace});
  const bool fast_r = ok && row_slots && attn_edge_plan_ok(pr, n_q, n_k) && F::row_fast_ok(x, Fd);
  const bool fast_c = ok && col_slots && attn_edge_plan_ok(pc, n_k, n_q);
  const AttnEdgeBwdWs w(fast_r || fast_c, es, n_q, n_k, h, Fd, F::ws_tail(x, Fd));
  GO_TRY(attn_ws_check(fn, F::query, slots, w.total, workspace, workspace_bytes));
  if (n_q * Fd > 0) { GO_PTR(fn, dQ); GO_HIP(zero_async(dQ, es * (size_t)(n_q * Fd), st)); }
  if (n_k * Fd > 0) {
    GO_PTR(fn, dK); GO_PTR(fn, dV);
    GO_HIP(zero_async(dK, es * (size_t)(n_k * Fd), st));
    GO_HIP(zero_async(dV, es * (size_t)(n_k * Fd), st));
  }
  GO_TRY(F::grad_fill(x, es, Fd, fast_r, st));
  if (!slots) return GRAPHOP_OK;
  GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
  const bool dropped = drop != nullptr;
  const typename F::Drop hd{drop ? drop->as<float>() : DropArgs<float>{}, (int)head0};
  char* base = (char*)workspace;
  void* P = base + w.o_st4;   // (m, 1 / l, D, 0) per (row, head): stats4 of the fast passes, P of the generic ones
  float* kv = (float*)(base + w.o_kv);
  float* qdo = (float*)(base + w.o_qdo);
  float* grad_r = F::row_grad(x, fast_r, base + w.o_tail);
  if (fast_r || fast_c) {
    ProfScope prof(F::l_pack.tag, st, F::l_pack.kernel);
    constexpr int RPB = kFastBlock / kGatGroup;
    GO_DISPATCH_GAT_HD(h, d, {
      hipLaunchKernelGGL((F::template pack<H, D, false>), dim3((unsigned)ceil_div(n_k, RPB)), dim3(kFastBlock), 0, st,
                         (const float*)K, (const float*)V, kv, n_k, (const float*)nullptr, (const float*)nullptr,
                         (float4*)nullptr);
      hipLaunchKernelGGL((F::template pack<H, D, true>), dim3((unsigned)ceil_div(n_q, RPB)), dim3(kFastBlock), 0, st,
                         (const float*)Q, (const float*)dO, qdo, n_q, (const float*)o, (const float*)stats, (float4*)P);
    });
    GO_LAUNCH_CHECK();
  } else {
    ProfScope prof(F::l_generic_pack.tag, st, F::l_generic_pack.kernel);
    GO_DISPATCH_FLOAT(dtype, T, {
      hipLaunchKernelGGL(F::template pack_generic<T>, dim3(grid_of(n_q * h)), dim3(256), 0, st, (const T*)stats,
                         (const T*)dO, (const T*)o, (T*)P, n_q * h, d);
    });
    GO_LAUNCH_CHECK();
  }
  if (fast_r) GO_TRY(F::row_open(x, grad_r, Fd, st));
  if (row_slots) {
    GO_TRY(r.require(fn));
    if (fast_r) {
      GO_TRY((attn_edge_launch_rows<F, false>(F::l_rows_row, r, r.eid_or_null(), h, d, qdo, kv,
                                              (const float4*)P, x, (float*)dQ, nullptr, grad_r, drop ? &hd : nullptr,
                                              st)));
      GO_TRY(F::row_close(x, grad_r, Fd, st));
    } else {
      ProfScope prof(F::l_generic_bwd_row.tag, st, F::l_generic_bwd_row.kernel);
      const dim3 grid((unsigned)ceil_div(n_row_chunks, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch((F::template bwd_row<T, DROP>), grid, dim3(kGenericBlock), st, r.row, r.indptr,
                  r.eid, r.indices, (const T*)Q, (const T*)K, (const T*)V,
                  F::template generic_args<T>(x), (const T*)P, (const T*)dO, (T*)dQ, (T*)F::grad(x), n_row_chunks, h, d,
                  (i64)head0, drop_arg<DROP, T>(drop));
      }));
      GO_LAUNCH_CHECK();
    }
  }
  if (col_slots) {
    GO_TRY(c.require(fn));
    if (fast_c) {
      // the column pass always reads eid_c: no eid_or_null() here
      GO_TRY((attn_edge_launch_rows<F, true>(F::l_rows_col, c, c.eid, h, d, kv, qdo,
                                             (const float4*)P, x, (float*)dK, (float*)dV, nullptr,
                                             drop ? &hd : nullptr, st)));
    } else {
      ProfScope prof(F::l_generic_bwd_col.tag, st, F::l_generic_bwd_col.kernel);
      const dim3 grid((unsigned)ceil_div(n_col_chunks, kGenericWavesPerBlock));
      GO_DISPATCH_FLOAT(dtype, T, GO_DISPATCH_BOOL(dropped, DROP, {
        go_launch((F::template bwd_col<T, DROP>), grid, dim3(kGenericBlock), st, c.row, c.indptr,
                  c.eid, c.indices, (const T*)Q, (const T*)K, (const T*)V,
                  F::template generic_args<T>(x), (const T*)P, (const T*)dO, (T*)dK, (T*)dV, n_col_chunks, h, d,
                  (i64)head0, drop_arg<DROP, T>(drop));
      }));
      GO_LAUNCH_CHECK();
    }
  }
  return GRAPHOP_OK;
}

}  // namespace graphop
