// Several-head forms of the fused dot-product attention passes (kernels_attn_heads.h): the decision,
// the workspace layouts and the launches.  attention.hip calls these from attn_forward / attn_backward for h > 1; the
// entry points, their arguments and the C ABI are unchanged.
#include "common.h"
#include "host.h"
#include "host_attn_rows.h"
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_attn_heads.h"

namespace graphop {
namespace {

// the several-head entries of GO_DISPATCH_GAT_HD
inline bool attn_heads_shape(i64 h, i64 d) {
  bool in_set = false;
  if (h > 1) GO_DISPATCH_GAT_HD(h, d, { in_set = (H == h && D == d); });
  return in_set;
}

// what both directions ask of the knobs, the shape and ONE plan (own rows n_own, gathered table n_tab)
bool attn_heads_plan_ok(int dtype, i64 h, i64 d, i64 n_edges, i64 n_own, i64 n_tab, const graphop_plan* plan) {
  const Tuning& t = tuning();
  if (!t.attn_fused || !t.attn_rows || !t.attn_heads || t.force_generic || dtype != GRAPHOP_F32) return false;
  if (!attn_heads_shape(h, d) || !plan || !plan->indices || n_edges == 0) return false;
  if (n_edges >= 0x7fffffffLL || n_own >= 0x7fffffffLL || n_tab >= 0x7fffffffLL) return false;
  return plan->info.max_row < n_own && plan->info.max_index < n_tab;
}

// The auto rule (attn_heads < 0): attn_rows_ok's two conditions for rows of F = h * d floats.
//  1. The E-sized streams the fused passes avoid must outweigh packing the two operand tables (16 F bytes of traffic
//     per node, x2 margin: at the one-head rule's x1.5 the products shape at 4 x 32 without a bias passed by 1.18 and
//     measured 36.8 ms against 35.4 ms, outside the rounds' spread; 8 x 16 there passes x2 and measured 36.0 against
//     37.0 ms).  Per slot the composed backward moves, beside the rows both forms gather:
//     two scalar gather sectors of 64 B (the column-major passes read a[e, :] and ds[e, :] by edge id: for h <= 16 the
//     slot's h values share one sector), four id pairs, and the (E, h) streams -- s written, s read and a written by
//     the softmax, a read and da written by the SpMM backward's row pass, a and da read and ds written by the softmax
//     backward, ds read by the SDDMM backward's row pass: 9 values = 36 h bytes.  The one-head constant 180 is this
//     sum at h = 1 (144 + 36), so the h-head constant is 144 + 36 h (432 B at h = 8).
//  2. Where the unfused passes would run on the column-window drivers (tables beyond the L2, enough slots per window)
//     those gather faster than any chunk-driver form: keep them.
bool attn_heads_auto_ok(i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r, hipStream_t st) {
  const i64 F = h * d;
  if ((144.0 + 36.0 * (double)h) * (double)n_edges <= 32.0 * (double)F * (double)(n_q + n_k)) return false;
  int windows = 0;
  GO_DISPATCH_LNV((int)F, {
    SweepLaunch sl;
    SweepOpts o;
    o.dry_run = 1;
    o.bpc = sweep_bpc(NV, false);
    windows = choose_sweep(plan_r, n_k, L, NV, st, &sl, false, &o);
  });
  return windows == 0;
}

struct HeadsBwdWs {
  size_t o_kv, o_qdo, o_st4, total;
  HeadsBwdWs(i64 n_q, i64 n_k, i64 h, i64 F) {
    o_kv = 0;
    o_qdo = o_kv + up256(sizeof(float) * (size_t)(n_k * 2 * F));
    o_st4 = o_qdo + up256(sizeof(float) * (size_t)(n_q * 2 * F));
    // (m, 1 / l, D, -) per (row, head) of the attention matrix, sized for either side's node count
    total = o_st4 + up256(sizeof(float4) * (size_t)((n_q + n_k) * h));
  }
};

template <bool COL>
int launch_heads_rows(const char* tag, const Csr& g, i64 h, i64 d, const float* own, const float* xt, const float4* st4,
                      const float* b, float* out0, float* out1, float* db, const AttnHeadsDrop* drop, hipStream_t st) {
  const i64 n_chunks = g.n_chunks;
  if (n_chunks == 0) return GRAPHOP_OK;
  ProfScope prof(tag, st, "k_attn_heads_bwd_rows_f32");
  const bool owned = g.owned(), dropped = drop != nullptr, biased = b != nullptr;
  const ChunkGeometry geo = attn_rows_geometry(n_chunks);
  GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(owned, OWNED, GO_DISPATCH_BOOL(dropped, DROP, GO_DISPATCH_BOOL(biased, BIAS, {
    if constexpr (H > 1)
      hipLaunchKernelGGL((k_attn_heads_bwd_rows_f32<H, D, COL, OWNED, DROP, BIAS>), dim3(geo.blocks), dim3(kFastBlock), 0,
                         st, g.row, g.indptr, g.eid_or_null(), g.indices, own, xt, st4, b, out0, out1, db, n_chunks,
                         (int)geo.cpg, drop_if_arg<DROP>(drop));
  }))));
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace

bool attn_heads_bwd_ok(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r,
                       const graphop_plan* plan_c, hipStream_t st) {
  if (h <= 1) return false;
  if (!attn_heads_plan_ok(dtype, h, d, n_edges, n_q, n_k, plan_r) ||
      !attn_heads_plan_ok(dtype, h, d, n_edges, n_k, n_q, plan_c))
    return false;
  return tuning().attn_heads > 0 || attn_heads_auto_ok(h, d, n_edges, n_q, n_k, plan_r, st);
}

size_t attn_heads_bwd_workspace(i64 n_q, i64 n_k, i64 h, i64 d) { return HeadsBwdWs(n_q, n_k, h, h * d).total; }

int attn_heads_fwd_rows(const Csr& g, i64 n_q, i64 n_k, i64 h, i64 d, int dtype, const void* Q, const void* K,
                        const void* V, const void* b, void* o, void* stats, void* ws, i64 ws_bytes, hipStream_t st,
                        bool dry_run, size_t* ws_needed, const HostDrop* hdrop, i64 head0) {
  const graphop_plan* plan = g.plan;
  const i64 n_chunks = g.n_chunks, n_edges = g.n_edges;
  if (ws_needed) *ws_needed = 0;
  if (hdrop && head0 + h >= 0x7fffffffLL) return 0;
  const AttnHeadsDrop hd{hdrop ? hdrop->as<float>() : DropArgs<float>{}, (int)head0};
  const AttnHeadsDrop* drop = hdrop ? &hd : nullptr;
  if (h <= 1 || n_chunks == 0 || !attn_heads_plan_ok(dtype, h, d, n_edges, n_q, n_k, plan)) return 0;
  if (!g.owned() || n_q >= kWalkRowMask) return 0;
  if (tuning().attn_heads < 0 && !attn_heads_auto_ok(h, d, n_edges, n_q, n_k, plan, st)) return 0;
  const i64 F = h * d;
  const ChunkGeometry geo = attn_rows_geometry(n_chunks);
  if (2 * geo.groups >= 0x7fffffffLL) return 0;
  const AttnRowsFwdWs w(ws, 2 * geo.groups, n_q, h, F);
  if (ws_needed) *ws_needed = w.total;
  if (dry_run) return 1;
  if (!ws || (size_t)ws_bytes < w.total) return 0;
  AttnHeadsFwdArgs a;
  a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V; a.b = (const float*)b;
  a.o = (float*)o; a.stats = (float*)stats;
  a.p_row = w.p_row; a.p_ml = w.p_ml; a.p_o = w.p_o;
  if (zero_async(o, sizeof(float) * (size_t)(n_q * F), st) != hipSuccess) return -GRAPHOP_ERR_HIP;
  attn_pieces_fill("attn_heads_fwd_setup", w, kAttnNegBig, st);
  const bool dropped = drop != nullptr, biased = b != nullptr;
  {
    ProfScope prof("attn_heads_fwd_rows", st, "k_attn_heads_fwd_rows_f32");
    GO_DISPATCH_GAT_HD(h, d, GO_DISPATCH_BOOL(dropped, DROP, GO_DISPATCH_BOOL(biased, BIAS, {
      if constexpr (H > 1)
        hipLaunchKernelGGL((k_attn_heads_fwd_rows_f32<H, D, DROP, BIAS>), dim3(geo.blocks), dim3(kFastBlock), 0, st,
                           g.row, g.indptr, g.eid_or_null(), g.indices, a, n_chunks,
                           (int)geo.cpg, drop_if_arg<DROP>(drop));
    })));
  }
  attn_pieces_merge(
      "attn_heads_fwd_merge", "k_attn_heads_piece_add", w, geo.lanes, st,
      [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(k_attn_heads_piece_max, grid, block, 0, st, w.p_row, w.p_ml, w.Mtmp, w.np * h, (int)h);
      },
      [&](dim3 grid, dim3 block) {
        GO_DISPATCH_GAT_HD(h, d, {
          if constexpr (H > 1)
            hipLaunchKernelGGL((k_attn_heads_piece_add<H, D>), grid, block, 0, st, w.p_row, w.p_ml, w.p_o, w.Mtmp, w.Ltmp,
                               a.o, w.np);
        });
      },
      [&](dim3 grid, dim3 block) {
        GO_DISPATCH_GAT_HD(h, d, {
          if constexpr (H > 1)
            hipLaunchKernelGGL((k_attn_heads_piece_fin<H, D>), grid, block, 0, st, w.p_row, w.Mtmp, w.Ltmp, a.o, a.stats,
                               w.np);
        });
      });
  if (hipGetLastError() != hipSuccess) return -GRAPHOP_ERR_HIP;
  return 1;
}

int attn_heads_backward(const Csr& r, const Csr& c, i64 n_q, i64 n_k, i64 h, i64 d, const void* Q, const void* K,
                        const void* V, const void* b, const void* o, const void* stats, const void* dO, void* dQ, void* dK,
                        void* dV, void* db, void* ws, hipStream_t st, const HostDrop* hdrop, i64 head0) {
  const AttnHeadsDrop hd{hdrop ? hdrop->as<float>() : DropArgs<float>{}, (int)head0};
  const AttnHeadsDrop* drop = hdrop ? &hd : nullptr;
  const i64 F = h * d;
  const HeadsBwdWs w(n_q, n_k, h, F);
  char* base = (char*)ws;
  float* kv = (float*)(base + w.o_kv);
  float* qdo = (float*)(base + w.o_qdo);
  float4* st4 = (float4*)(base + w.o_st4);
  GO_HIP(zero_async(dQ, sizeof(float) * (size_t)(n_q * F), st));
  GO_HIP(zero_async(dK, sizeof(float) * (size_t)(n_k * F), st));
  GO_HIP(zero_async(dV, sizeof(float) * (size_t)(n_k * F), st));
  {
    ProfScope prof("attn_heads_pack", st, "k_attn_heads_pack");
    constexpr int RPB = kFastBlock / 16;
    GO_DISPATCH_GAT_HD(h, d, {
      if constexpr (H > 1) {
        if (n_k > 0)
          hipLaunchKernelGGL((k_attn_heads_pack<H, D, false>), dim3((unsigned)ceil_div(n_k, RPB)), dim3(kFastBlock), 0, st,
                             (const float*)K, (const float*)V, kv, n_k, (const float*)nullptr, (const float*)nullptr,
                             (float4*)nullptr);
        if (n_q > 0)
          hipLaunchKernelGGL((k_attn_heads_pack<H, D, true>), dim3((unsigned)ceil_div(n_q, RPB)), dim3(kFastBlock), 0, st,
                             (const float*)Q, (const float*)dO, qdo, n_q, (const float*)o, (const float*)stats, st4);
      }
    });
    GO_LAUNCH_CHECK();
  }
  GO_TRY((launch_heads_rows<false>("attn_heads_rows_row", r, h, d, qdo, kv, st4, (const float*)b,
                                   (float*)dQ, nullptr, (float*)db, drop, st)));
  GO_TRY((launch_heads_rows<true>("attn_heads_rows_col", c, h, d, kv, qdo, st4, (const float*)b,
                                  (float*)dK, (float*)dV, nullptr, drop, st)));
  return GRAPHOP_OK;
}

}  // namespace graphop
