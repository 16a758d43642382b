// Host side of the fused dot-product attention ops, stated once: the argument checks every entry point makes first, the
// workspace check, the launch geometry of the chunk-driver passes, and the piece-record forward -- its workspace, its
// fills and its merge -- that attn_fwd_walk, attn_bias_fwd_rows (graphop_hip.hip), attn_heads_fwd_rows
// (attention_heads.hip) and attn_edge_forward (host_attn_edge_ops.h: the edge-row ops of attention_edge.hip and
// attention_etype.hip) run around their own pass.
#pragma once
#include <type_traits>

#include "common.h"
#include "host.h"
#include "host_dropout.h"

namespace graphop {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the checks every entry point of the attention ops makes first
inline int attn_check(const char* fn, int dtype, i64 n_row_chunks, i64 n_col_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h,
                      i64 d) {
  GO_CHECK_ARG(dtype == GRAPHOP_F32 || dtype == GRAPHOP_F64, "%s: bad dtype", fn);
  GO_CHECK_ARG(n_row_chunks >= 0 && n_col_chunks >= 0 && n_edges >= 0 && n_q >= 0 && n_k >= 0 && h >= 1 && d >= 0,
               "%s: negative size", fn);
  return GRAPHOP_OK;
}

// the dropout arguments of the entry points that take them, as they arrive; checked after the checks above
struct DropIn {
  double p;
  uint64_t seed;
  uint32_t offset;
  i64 head0;
};

inline int attn_drop_check(const char* fn, const DropIn& in, i64 n_q, i64 n_k, HostDrop* out) {
  GO_TRY(drop_check(fn, in.p, in.seed, n_q, n_k, in.offset, out));
  GO_CHECK_ARG(in.head0 >= 0 && in.head0 < ((i64)1 << 32), "%s: head0 must be in [0, 2^32), got %lld", fn,
               (long long)in.head0);
  return GRAPHOP_OK;
}

// the workspace a form needs against the one the caller brought; query: the graphop_*_workspace_bytes that reports it
inline int attn_ws_check(const char* fn, const char* query, bool needed, size_t need, const void* workspace,
                         i64 workspace_bytes) {
  GO_CHECK_ARG(!needed || (workspace != nullptr && workspace_bytes >= 0 && (size_t)workspace_bytes >= need),
               "%s: workspace of %lld bytes needed (graphop_%s), got %lld", fn, (long long)need, query,
               (long long)workspace_bytes);
  return GRAPHOP_OK;
}

// the kernel argument of a DROP instantiation from the pass's dropout record (AttnDrop, AttnHeadsDrop, AttnEdgeDrop);
// drop is NULL exactly where DROP is false
template <bool DROP, class D>
inline std::conditional_t<DROP, D, NoDrop> drop_if_arg(const D* drop) {
  if constexpr (DROP) return *drop;
  else return NoDrop{};
}

// The one-head chunk-driver passes (k_attn_bwd_rows_f32, k_attn_bias_bwd_rows_f32, k_attn_bias_fwd_rows_f32): lane groups
// of GO_DISPATCH_LNV's L lanes for rows of F floats, at most 16 chunks each.
inline ChunkGeometry attn_one_head_geometry(i64 n_chunks, i64 F) {
  return chunk_geometry(n_chunks, (int)(F / 4 < 64 ? F / 4 : 64), 16);
}

// The several-head and edge passes (kernels_attn_rows_passes.inc): 16-lane groups and four (not eight) rounds of resident
// workgroups wanted -- these kernels hold 150 to 240 VGPRs, two workgroups per CU where the one-head kernels hold four,
// so the same number of rounds per resident slot needs half the groups, and every group of the forward costs two piece
// records of (1 + 2 h + F) words.
inline ChunkGeometry attn_rows_geometry(i64 n_chunks) { return chunk_geometry(n_chunks, 16, 16, /*rounds=*/4); }

// The workspace of a piece-record forward.  A pass whose lane groups (or bins) share rows leaves what it saw of a shared
// row as a piece record -- the row word, (m, l) per head, the o row of F floats -- and np records are merged into o and
// stats through (Mtmp, Ltmp) per (row, head).  base == NULL: the size query, only `total` means anything.
struct AttnRowsFwdWs {
  int* p_row;
  float *p_ml, *p_o, *Mtmp, *Ltmp;
  size_t total = 0;
  i64 np, h, n_ml;   // records; heads; (row, head) pairs
  AttnRowsFwdWs(void* base, i64 np_, i64 n_q, i64 h_, i64 F) : np(np_), h(h_), n_ml(n_q * h_) {
    auto take = [&](size_t bytes) {
      void* p = base ? (char*)base + total : nullptr;
      total += up256(bytes);
      return p;
    };
    p_row = (int*)take(sizeof(int) * (size_t)np);
    p_ml = (float*)take(sizeof(float) * 2 * (size_t)(np * h));
    p_o = (float*)take(sizeof(float) * (size_t)(np * F));
    Mtmp = (float*)take(sizeof(float) * (size_t)n_ml);
    Ltmp = (float*)take(sizeof(float) * (size_t)n_ml);
  }
};

// before the pass: no record, no score yet (the kernels' kAttnNegBig), empty sums.  Ws = AttnRowsFwdWs: a template, as
// the merge is, so that only the translation units that run a forward instantiate k_fill.
template <class Ws>
inline void attn_pieces_fill(const char* tag, const Ws& w, float no_score, hipStream_t st) {
  ProfScope prof(tag, st, "k_fill");
  const i64 most = w.np > w.n_ml ? w.np : w.n_ml;
  const unsigned fb = (unsigned)(ceil_div(most, 256) > 4096 ? 4096 : ceil_div(most, 256));
  hipLaunchKernelGGL((k_fill<int>), dim3(fb), dim3(256), 0, st, w.p_row, w.np, -1);
  hipLaunchKernelGGL((k_fill<float>), dim3(fb), dim3(256), 0, st, w.Mtmp, w.n_ml, no_score);
  hipLaunchKernelGGL((k_fill<float>), dim3(fb), dim3(256), 0, st, w.Ltmp, w.n_ml, 0.f);
}

// after the pass: the maxima per (record, head), then the sums and the division by lane groups of `lanes` lanes.  The
// three kernels are the caller's (each family's piece_max has no template and lives in one translation unit); each
// callable launches its kernel on the (grid, block) it is given.
template <class Max, class Add, class Fin>
inline void attn_pieces_merge(const char* tag, const char* label, const AttnRowsFwdWs& w, int lanes, hipStream_t st,
                              Max piece_max, Add piece_add, Fin piece_fin) {
  ProfScope prof(tag, st, label);
  piece_max(dim3((unsigned)ceil_div(w.np * w.h, 256)), dim3(256));
  const dim3 grid((unsigned)ceil_div(w.np, (i64)(kFastBlock / lanes))), block(kFastBlock);
  piece_add(grid, block);
  piece_fin(grid, block);
}

}  // namespace graphop
