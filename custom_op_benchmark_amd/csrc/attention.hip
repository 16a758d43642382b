// Fused attention step (extra op next to the reference's eight):
//   forward : o = vector_spmm(sparse_softmax(maskedmm_csr(Q, K)), V), leaving only o and the row
//             statistics (max, 1 / sum) behind -- s and a live in the caller's workspace;
//   backward: dQ, dK, dV from (Q, K, V, o, stats, dO) by two fused passes (kernels_attn.h) that
//             recompute a and ds per slot -- window-owner drivers where a sweepable plan and a table
//             beyond the L2 make column windows pay, chunk drivers otherwise; when neither applies
//             (no plan, fp64, several heads) the same result comes from the composition of the
//             unfused entry points, with the intermediates in the workspace.
// Attention dropout (graphop_attention_dropout_*): o = sum_j a_ij m_ij V_j with the multiplier of
// kernels_dropout.h recomputed per slot.  The forms are chosen by the rules of the undropped op; the fused kernels run
// their DROP instantiations, the composed path multiplies a (and the gradient that comes back) by m with
// k_attn_drop_apply.  drop == nullptr below is the undropped op: the same kernels and launches as before.
// Per-edge score bias (graphop_attention_bias_*): s_e = <Q_i, K_j> + b[e] with b indexed by edge id, db =
// ds.  The composed path adds b to s with k_attn_bias_add and lets the softmax backward write ds into db; the fused
// backward is the chunk-driver form with the bias (k_attn_bias_bwd_rows_f32) wherever the undropped op would run either
// fused form, the fused forward the chunk-driver pass of kernels_attn_bias_fwd.h.  bias == nullptr below is the op
// without a bias: the same kernels and launches as before.
// Several heads: where attention_heads.hip's conditions hold (fp32, (h, d) one of its pairs, plans with
// neighbour ids, the knobs) all three ops run chunk-driver passes over all heads of a row at once
// (kernels_attn_heads.h), asked for first by attn_fused_forward / attn_backward_form; h == 1 and every other
// several-head call go on as before.
// Reference composition: wrapper.py:20-30 (MaskedMMCSR), :8-18 (SparseSoftmax), :44-55 (VectorSPMM).
#include "common.h"
#include "host.h"
#include "host_attn_rows.h"
#include "host_dropout.h"
#include "host_gat.h"
#include "kernels_attn_bias.h"

namespace graphop {
namespace {

// resident workgroups per CU the fused kernels are compiled for: the column-major pass carries two
// accumulators and the statistics pipeline and needs more than 128 VGPRs; so do rows of >= 512 floats
constexpr int attn_bpc(int NV, bool col) { return col ? (NV >= 4 ? 2 : 3) : (NV >= 2 ? 3 : 4); }
// with the ids staged through LDS (4 more VGPRs, 1 KB more LDS per group) the one-row pass runs 3 per CU
constexpr int attn_bpc_staged(int NV, bool col) { return col ? (NV >= 4 ? 2 : 3) : 3; }
// With dropout the d = 128 row pass (L = 32, NV = 1) would spill at its 4 workgroups per CU (128 VGPRs, all in use
// without dropout): that DROP instantiation alone is compiled for one fewer.  The launch geometry stays the undropped
// one; the task queue hands the surplus workgroups whatever is left when they start.
constexpr int attn_bpc_drop(int L, int NV, bool col) { return attn_bpc(NV, col) - ((L == 32 && NV == 1 && !col) ? 1 : 0); }
inline bool attn_staged(int L, int NV) { return (tuning().staged_ids & 4) && L == 16 && NV == 1; }   // d = 64: the other widths would spill in the column pass

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct AttnFast {
  SweepLaunch r, c;   // row-major pass (gathers K|V), column-major pass (gathers Q|dO)
};

SweepOpts attn_opts(int L, int NV, bool col, bool dry_run) {
  const Tuning& t = tuning();
  SweepOpts o;
  o.row_bytes = 2 * 16LL * L * NV;
  o.K = t.attn_k > 0 ? t.attn_k : (4 / NV > 0 ? 4 / NV : 1);
  o.window_scale = t.attn_window_scale > 0 ? t.attn_window_scale : 1;
  o.dry_run = dry_run ? 1 : 0;
  o.staged = attn_staged(L, NV) ? 1 : 0;
  o.no_eids = 1;          // (a, ds are recomputed per slot: neither fused pass reads eid)
  o.stage_lds_per_group = (4 * L > 128 ? 4 * L : 128) * 2 * (int)sizeof(int);   // StageCfg<L, 1>::kLdsIntsPerGroup ints
  const int cap = o.staged ? attn_bpc_staged(NV, col) : attn_bpc(NV, col);
  o.bpc = (t.attn_bpc > 0 && t.attn_bpc < cap) ? t.attn_bpc : cap;
  return o;
}

// Do the fused window-owner passes apply?  1 = yes (launch geometry in *out), 0 = no, < 0 = error.
// dry_run: only decide (and build the cached window structures), take no task queue.
int attn_fast_plan(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r,
                   const graphop_plan* plan_c, hipStream_t st, bool dry_run, AttnFast* out) {
  const Tuning& t = tuning();
  if (!t.attn_fused || t.force_generic || dtype != GRAPHOP_F32 || h != 1) return 0;
  if (!plan_r || !plan_c || d % 4 != 0 || !pow2(d) || d < 16 || d > 1024 || d > t.attn_max_d) return 0;
  if (n_edges >= 0x7fffffffLL || n_q >= 0x7fffffffLL || n_k >= 0x7fffffffLL || n_edges == 0) return 0;
  if (plan_r->info.max_row >= n_q || plan_r->info.max_index >= n_k || plan_c->info.max_row >= n_k ||
      plan_c->info.max_index >= n_q)
    return 0;
  int use_r = 0, use_c = 0;
  GO_DISPATCH_LNV((int)d, {
    SweepOpts o = attn_opts(L, NV, false, dry_run);
    use_r = choose_sweep(plan_r, n_k, L, NV, st, &out->r, true, &o);
    o = attn_opts(L, NV, true, dry_run);
    if (use_r == 1) use_c = choose_sweep(plan_c, n_q, L, NV, st, &out->c, true, &o);
  });
  if (use_r < 0) return use_r;
  if (use_c < 0) return use_c;
  return (use_r == 1 && use_c == 1) ? 1 : 0;
}

// Workspace layouts: byte offsets first (the size queries pass no buffer), pointers only from a real base.
inline char* at_offset(char* base, size_t off) { return base ? base + off : nullptr; }

// The chunk-driver form of the fused passes (k_attn_bwd_rows_f32): any fp32 one-head graph with plans
// (they carry the id ranges that make the gathers safe); no window structure needed.
bool attn_rows_ok(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r,
                  const graphop_plan* plan_c, hipStream_t st) {
  const Tuning& t = tuning();
  if (!t.attn_fused || !t.attn_rows || t.force_generic || dtype != GRAPHOP_F32 || h != 1) return false;
  if (!plan_r || !plan_c || d % 4 != 0 || !pow2(d) || d < 16 || d > 1024 || n_edges == 0) return false;
  if (!plan_r->indices || !plan_c->indices) return false;
  // Worth it only where the E-sized streams the fused passes avoid (~180 B per slot: two 64-B scalar
  // gather sectors, four 16-B id pairs, da / ds) outweigh packing the two operand tables
  // (16*F bytes of traffic per node, x1.5 margin).  Measured: products-shape d=16 (E/N = 25)
  // 16.0 -> 9.5 ms per step; papers100M-shape shard d=128 (E/N = 14.5: the 512-B rows dominate, the
  // step is HBM-gather-bound either way) 139 -> 152 ms, so that shape keeps the unfused passes.
  if (t.attn_rows < 0 && 180.0 * (double)n_edges <= 24.0 * (double)d * (double)(n_q + n_k)) return false;
  // The chunk-driver passes gather at the rate of wherever the tables live; where the unfused passes
  // would run on the column-window drivers (tables beyond the L2 with enough slots per window) those
  // are faster than any chunk-driver form, and this shape was excluded from the fused window passes
  // on purpose (attn_max_d): keep the unfused passes.
  if (t.attn_rows < 0) {
    int windows = 0;
    GO_DISPATCH_LNV((int)d, {
      SweepLaunch sl;
      SweepOpts o;
      o.dry_run = 1;
      o.bpc = sweep_bpc(NV, true);
      windows = choose_sweep(plan_r, n_k, L, NV, st, &sl, false, &o);
    });
    if (windows != 0) return false;
  }
  return plan_r->info.max_row < n_q && plan_r->info.max_index < n_k && plan_c->info.max_row < n_k &&
         plan_c->info.max_index < n_q;
}

// The one-head chunk-driver backward pass over one orientation's chunks: k_attn_bwd_rows_f32, with BIAS
// k_attn_bias_bwd_rows_f32 (b and db by edge id; eid == nullptr: the plan has eid_identity).  Without BIAS eid, b and
// db are not read.
template <bool COL, bool DROP, bool BIAS>
int launch_attn_rows(const char* tag, const Csr& g, int F, const float* own, const float* xt, const float4* st4,
                     const float* b, float* out0, float* out1, float* db, const AttnDrop* drop, hipStream_t st) {
  const i64 n_chunks = g.n_chunks;
  if (n_chunks == 0) return GRAPHOP_OK;
  const i64* eid = g.eid_or_null();
  ProfScope prof(tag, st, BIAS ? (DROP ? "k_attn_bias_bwd_rows_f32<DROP>" : "k_attn_bias_bwd_rows_f32")
                               : (DROP ? "k_attn_bwd_rows_f32<DROP>" : "k_attn_bwd_rows_f32"));
  const ChunkGeometry geo = attn_one_head_geometry(n_chunks, F);
  const dim3 grid(geo.blocks), block(kFastBlock);
  GO_DISPATCH_LNV(F, GO_DISPATCH_BOOL(g.owned(), OWNED, {
    if constexpr (BIAS)
      hipLaunchKernelGGL((k_attn_bias_bwd_rows_f32<L, NV, COL, OWNED, DROP>), grid, block, 0, st, g.row, g.indptr, eid,
                         g.indices, own, xt, st4, b, out0, out1, db, n_chunks, (int)geo.cpg, drop_if_arg<DROP>(drop));
    else
      hipLaunchKernelGGL((k_attn_bwd_rows_f32<L, NV, COL, OWNED, DROP>), grid, block, 0, st, g.row, g.indptr, g.indices,
                         own, xt, st4, out0, out1, n_chunks, (int)geo.cpg, drop_if_arg<DROP>(drop));
  }));
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

struct FastWs {
  float* kv; float* qdo; float4* st4; size_t total;
  FastWs(char* base, i64 n_q, i64 n_k, i64 F) {
    size_t off = 0;
    kv = (float*)at_offset(base, off); off += align_up(sizeof(float) * (size_t)(n_k * 2 * F));
    qdo = (float*)at_offset(base, off); off += align_up(sizeof(float) * (size_t)(n_q * 2 * F));
    st4 = (float4*)at_offset(base, off); off += align_up(sizeof(float4) * (size_t)n_q);
    total = off;
  }
};

// E-sized intermediates of the composed path: n_arrays of n_edges*h values + the softmax scratch (the fifth array is
// the masked weights a * m of the backward with dropout)
struct SlowWs {
  char* arr[5]; char* soft; size_t total;
  SlowWs(char* base, int n_arrays, size_t es, i64 E, i64 h, i64 soft_rows) {
    size_t off = 0;
    for (int i = 0; i < 5; ++i) {
      arr[i] = at_offset(base, off);
      if (i < n_arrays) off += align_up(es * (size_t)(E * h));
    }
    soft = at_offset(base, off); off += align_up(es * (size_t)(2 * soft_rows * h));
    total = off;
  }
};

inline i64 soft_rows_of(const graphop_plan* plan_r, i64 n_q) {
  return (plan_r && plan_r->info.row_owned) ? 0 : n_q;   // general softmax path: max / sum per row
}

template <bool COL, bool DROP>
int launch_attn_pass(const char* tag, const SweepLaunch& sl, int F, i64 n_gathered, const float* own,
                     const float* xt, const float4* st4, float* out0, float* out1, const AttnDrop* drop,
                     hipStream_t st) {
  ProfScope prof(tag, st, DROP ? "k_attn_bwd_wown_f32<DROP>" : "k_attn_bwd_wown_f32");
  const dim3 grid(sl.blocks), block(kFastBlock);
  const AttnDropIf<DROP> dr = drop_if_arg<DROP>(drop);
  GO_DISPATCH_LNV(F, {
    const bool off32 = n_gathered * 2 * 16LL * L * NV < (1LL << 32);
    constexpr int BPC = DROP ? attn_bpc_drop(L, NV, COL) : attn_bpc(NV, COL);
    bool staged = false;
    if constexpr (L == 16 && NV == 1) {
      if (sl.view.rec != nullptr) {
        constexpr int BPS = attn_bpc_staged(NV, COL);
        staged = true;
        if (off32)
          hipLaunchKernelGGL((k_attn_bwd_wown_f32<L, NV, COL, true, BPS, true, DROP>), grid, block, sl.lds_bytes, st,
                             sl.view, own, xt, st4, out0, out1, dr);
        else
          hipLaunchKernelGGL((k_attn_bwd_wown_f32<L, NV, COL, false, BPS, true, DROP>), grid, block, sl.lds_bytes, st,
                             sl.view, own, xt, st4, out0, out1, dr);
      }
    }
    if (staged) {
    } else if (off32)
      hipLaunchKernelGGL((k_attn_bwd_wown_f32<L, NV, COL, true, BPC, false, DROP>), grid, block, sl.lds_bytes, st,
                         sl.view, own, xt, st4, out0, out1, dr);
    else
      hipLaunchKernelGGL((k_attn_bwd_wown_f32<L, NV, COL, false, BPC, false, DROP>), grid, block, sl.lds_bytes, st,
                         sl.view, own, xt, st4, out0, out1, dr);
  });
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

}  // namespace

int attn_prepare_plan(const graphop_plan* plan, i64 n_table_rows, i64 d, bool col, hipStream_t st) {
  const Tuning& t = tuning();
  if (!t.attn_fused || t.force_generic || !plan || d % 4 != 0 || !pow2(d) || d < 16 || d > 1024 || d > t.attn_max_d) return 0;
  int use = 0;
  GO_DISPATCH_LNV((int)d, {
    SweepLaunch sl;
    SweepOpts o = attn_opts(L, NV, col, true);
    use = choose_sweep(plan, n_table_rows, L, NV, st, &sl, true, &o);
  });
  return use;
}
}  // namespace graphop

using namespace graphop;

namespace {

// the bias arguments of the *_bias_* entry points as they arrive; checked after the dropout arguments (attn_check and
// attn_drop_check, host_attn_rows.h, come first)
struct BiasIn {
  const void* b;   // (n_edges, h) by edge id
  void* db;        // backward: NULL = the gradient of b is not wanted (nothing edge-sized is then written)
};

int attn_bias_check(const char* fn, const BiasIn& in, i64 n_edges, i64 h) {
  GO_CHECK_ARG(n_edges * h == 0 || in.b != nullptr, "%s: b is NULL", fn);
  return GRAPHOP_OK;
}

// the chunk-driver fused backward with a bias: wherever the undropped op would run either of its fused forms
bool attn_bias_rows_ok(int fast, int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r,
                       const graphop_plan* plan_c, hipStream_t st) {
  if (!tuning().attn_rows) return false;
  if (attn_rows_ok(dtype, h, d, n_edges, n_q, n_k, plan_r, plan_c, st)) return true;
  return fast == 1 && plan_r->indices && plan_c->indices;   // (attn_fast_plan checked the id ranges)
}

// s += b, both (n_edges, h) by edge id
int attn_bias_add(int dtype, void* s, const void* b, i64 n, hipStream_t st) {
  if (n == 0) return GRAPHOP_OK;
  ProfScope prof("attn_bias_add", st, "k_attn_bias_add");
  const i64 want = ceil_div(n, kGenericBlock);
  const unsigned nb = (unsigned)(want > 65536 ? 65536 : want);
  if (dtype == GRAPHOP_F32)
    hipLaunchKernelGGL((k_attn_bias_add<float>), dim3(nb), dim3(kGenericBlock), 0, st, (float*)s, (const float*)b, n);
  else
    hipLaunchKernelGGL((k_attn_bias_add<double>), dim3(nb), dim3(kGenericBlock), 0, st, (double*)s, (const double*)b, n);
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

// y = x * m over the row-major chunks (k_attn_drop_apply), in place or not
int attn_drop_apply(int dtype, const Csr& g, const void* x, void* y, i64 h, i64 head0, const HostDrop& drop,
                    hipStream_t st) {
  const i64 n_chunks = g.n_chunks;
  if (n_chunks == 0 || g.n_edges * h == 0) return GRAPHOP_OK;
  ProfScope prof("attn_drop_apply", st, "k_attn_drop_apply");
  const unsigned nb = (unsigned)ceil_div(n_chunks, kGenericWavesPerBlock);
  auto launch = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((k_attn_drop_apply<T>), dim3(nb), dim3(kGenericBlock), 0, st, g.row, g.indptr, g.eid, g.indices,
                       (const T*)x, (T*)y, n_chunks, h, head0, drop.as<T>());
  };
  if (dtype == GRAPHOP_F32) launch(0.f);
  else launch(0.0);
  GO_LAUNCH_CHECK();
  return GRAPHOP_OK;
}

// The fused forward of a call where one applies: several heads in one chunk-driver pass (kernels_attn_heads.h, with or
// without a bias); one head with a bias in the chunk-driver pass of kernels_attn_bias_fwd.h (the walk's layouts carry no
// edge id); one head without on the walk (kernels_attn_walk.h).  The contract of the three: 1 = launched (dry_run:
// applies), 0 = does not apply, < 0 = error, *needed = the workspace.  biased with b == NULL: a dry run of the op with a
// bias.  Needs a plan of the call's arrays and n_edges * h > 0.
int attn_fused_forward(const Csr& g, i64 n_q, i64 n_k, i64 h, i64 d, int dtype, const void* Q, const void* K, const void* V, bool biased, const void* b, void* o,
                       void* stats, void* ws, i64 ws_bytes, hipStream_t st, bool dry_run, size_t* needed,
                       const HostDrop* drop = nullptr, i64 head0 = 0, const AttnDrop* hd = nullptr) {
  if (h > 1)
    return attn_heads_fwd_rows(g, n_q, n_k, h, d, dtype, Q, K, V, b, o, stats, ws, ws_bytes, st,
                               dry_run, needed, drop, head0);
  if (biased)
    return attn_bias_fwd_rows(g, n_q, n_k, h, d, dtype, Q, K, V, b, o, stats, ws, ws_bytes, st,
                              dry_run, needed, hd);
  return attn_fwd_walk(g.plan, n_q, n_k, h, d, dtype, Q, K, V, o, stats, ws, ws_bytes, st, dry_run, needed, hd);
}

// The form of a call's backward: the several-head chunk-driver passes (attention_heads.hip), the window-owner passes
// (launch geometry in *af), the one-head chunk-driver passes, or the composition of the unfused entry points.  With a
// bias the chunk-driver form runs wherever either one-head fused form would (the window layouts carry no edge id), and
// the window-owner passes are only asked for their decision.  dry_run: only decide; else a Windows answer has taken its
// task queues.
enum class AttnBwd { Composed, Heads, Windows, Rows };

int attn_backward_form(bool biased, bool dry_run, int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k,
                       const graphop_plan* pr, const graphop_plan* pc, hipStream_t st, AttnFast* af, AttnBwd* form) {
  *form = AttnBwd::Heads;
  if (attn_heads_bwd_ok(dtype, h, d, n_edges, n_q, n_k, pr, pc, st)) return GRAPHOP_OK;
  const int fast = attn_fast_plan(dtype, h, d, n_edges, n_q, n_k, pr, pc, st, dry_run || biased, af);
  if (fast < 0) return -fast;
  if (biased) *form = attn_bias_rows_ok(fast, dtype, h, d, n_edges, n_q, n_k, pr, pc, st) ? AttnBwd::Rows : AttnBwd::Composed;
  else if (fast == 1) *form = AttnBwd::Windows;
  else *form = attn_rows_ok(dtype, h, d, n_edges, n_q, n_k, pr, pc, st) ? AttnBwd::Rows : AttnBwd::Composed;
  return GRAPHOP_OK;
}

// bwd_arrays: E-sized arrays of the composed backward (4; 5 with dropout: the masked weights; with a bias one fewer
// where db takes the place of ds).  bias: the forms of the op with a bias are the ones decided on.
int attn_workspace_bytes(const char* fn, int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                         int64_t d, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream,
                         int bwd_arrays, int64_t* bytes_out, bool bias = false) {
  GO_CHECK_ARG(bytes_out != nullptr, "%s: bytes_out is NULL", fn);
  GO_TRY(attn_check(fn, dtype, 0, 0, n_edges, n_q, n_k, h, d));
  const size_t es = esize(dtype);
  hipStream_t st = (hipStream_t)stream;
  if (!backward) {
    size_t need = 0;
    int fw = 0;
    if (plan_r && n_edges * h > 0)
      // (the plan's own arrays: the plan of a forward with this n_edges, or of none)
      fw = attn_fused_forward(Csr(plan_r->row, plan_r->indptr, plan_r->eid, plan_r->indices, plan_r->info.n_chunks,
                                  n_edges, plan_r),
                              n_q, n_k, h, d, dtype, nullptr, nullptr, nullptr, bias, nullptr, nullptr, nullptr, nullptr, 0,
                              st, /*dry_run=*/true, &need);
    if (fw < 0) return -fw;
    // the one-pass forward only needs the piece records of shared rows; the composed forward keeps s and a here
    *bytes_out = fw == 1 ? (int64_t)need : (int64_t)SlowWs(nullptr, 2, es, n_edges, h, soft_rows_of(plan_r, n_q)).total;
    return GRAPHOP_OK;
  }
  AttnFast af;
  AttnBwd form;
  GO_TRY(attn_backward_form(bias, /*dry_run=*/true, dtype, h, d, n_edges, n_q, n_k, plan_r, plan_c, st, &af, &form));
  if (form == AttnBwd::Heads) *bytes_out = (int64_t)attn_heads_bwd_workspace(n_q, n_k, h, d);
  else if (form == AttnBwd::Composed)
    *bytes_out = (int64_t)SlowWs(nullptr, bwd_arrays, es, n_edges, h, soft_rows_of(plan_r, n_q)).total;
  else *bytes_out = (int64_t)FastWs(nullptr, n_q, n_k, h * d).total;
  return GRAPHOP_OK;
}

// What attn_forward and attn_backward establish first: the checks, then the call's dropout as the forms take it.
struct AttnCall {
  HostDrop hdrop;
  const HostDrop* drop = nullptr;   // NULL: no dropout arguments, or p == 0 (the undropped op)
  i64 head0 = 0;
  AttnDrop hd{};                    // the one-head kernels' record for the call's first head ...
  const AttnDrop* hdp = nullptr;    // ... NULL exactly where drop is
  const char* ws_fn;                // the query that reports this call's workspace
  hipStream_t st;
};

// din == nullptr: the op without dropout arguments; bias != nullptr: the form with a per-edge score bias
int attn_open(const char* fn, int dtype, i64 n_row_chunks, i64 n_col_chunks, i64 n_edges, i64 n_q, i64 n_k, i64 h, i64 d,
              const DropIn* din, const BiasIn* bias, void* stream, AttnCall* c) {
  GO_TRY(check_async_error(false));
  GO_TRY(attn_check(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d));
  if (din) GO_TRY(attn_drop_check(fn, *din, n_q, n_k, &c->hdrop));
  if (bias) GO_TRY(attn_bias_check(fn, *bias, n_edges, h));
  c->st = (hipStream_t)stream;
  c->head0 = din ? din->head0 : 0;
  if (din && din->p > 0.0) {
    c->drop = &c->hdrop;
    c->hd = AttnDrop{c->hdrop.as<float>(), (unsigned)(c->head0 >> 2), (int)(c->head0 & 3)};   // Philox block and word
    c->hdp = &c->hd;
  }
  c->ws_fn = bias ? "attention_bias_workspace_bytes"
                  : (c->drop ? "attention_dropout_workspace_bytes" : "attention_workspace_bytes");
  return GRAPHOP_OK;
}

// din == nullptr: graphop_attention_forward, else its dropout form (p == 0: the undropped op), as `fn`;
// bias != nullptr: the form with a per-edge score bias
int attn_forward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr,
                 const int64_t* eid, const int64_t* indices, const void* Q, const void* K, const void* V, void* o,
                 void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                 void* workspace, int64_t workspace_bytes, const DropIn* din, const graphop_plan_t* plan,
                 void* stream, const BiasIn* bias = nullptr) {
  AttnCall c;
  GO_TRY(attn_open(fn, dtype, n_chunks, 0, n_edges, n_q, n_k, h, d, din, bias, stream, &c));
  const HostDrop* drop = c.drop;
  const int64_t head0 = c.head0;
  hipStream_t st = c.st;
  const size_t es = esize(dtype);
  if (n_q * h > 0) {
    GO_PTR(fn, stats);
    GO_HIP(zero_async(stats, es * (size_t)(n_q * h * 2), st));   // rows without edges: (0, 0)
  }
  const Csr g(row, indptr, eid, indices, n_chunks, n_edges, plan);
  const graphop_plan* pm = g.plan;
  // ONE fused pass where it applies: s and a never leave the chip; its workspace (piece records of the rows that bins or
  // lane groups share) is what the call's workspace query reported
  if (pm && n_edges * h > 0) {
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, o);
    size_t need = 0;
    auto fused_fwd = [&](void* w, int64_t w_bytes, bool dry_run, size_t* needed) {
      return attn_fused_forward(g, n_q, n_k, h, d, dtype, Q, K, V, bias != nullptr,
                                bias ? bias->b : nullptr, o, stats, w, w_bytes, st, dry_run, needed, drop, head0, c.hdp);
    };
    const int ok = fused_fwd(nullptr, 0, /*dry_run=*/true, &need);
    if (ok < 0) return -ok;
    if (ok == 1) {
      GO_TRY(attn_ws_check(fn, c.ws_fn, true, need, workspace, workspace_bytes));
      const int fw = fused_fwd(workspace, workspace_bytes, /*dry_run=*/false, nullptr);
      if (fw < 0) return -fw;
      if (fw == 1) return GRAPHOP_OK;
    }
  }
  const i64 soft_rows = soft_rows_of(pm, n_q);
  SlowWs ws((char*)workspace, 2, es, n_edges, h, soft_rows);
  GO_TRY(attn_ws_check(fn, c.ws_fn, n_edges * h != 0, ws.total, workspace, workspace_bytes));
  void* s = ws.arr[0];
  void* a = ws.arr[1];
  GO_TRY(graphop_maskedmm_csr_forward(dtype, row, indptr, eid, indices, Q, K, s, n_chunks, n_edges, n_q,
                                      n_k, h, d, pm, stream));
  if (bias) GO_TRY(attn_bias_add(dtype, s, bias->b, n_edges * h, st));
  if (n_edges * h > 0)
    GO_TRY(softmax_forward_stats(dtype, Csr(row, indptr, eid, nullptr, n_chunks, n_edges, pm), s, a, h,
                                 soft_rows ? ws.soft : nullptr, soft_rows, st, stats));
  if (drop) GO_TRY(attn_drop_apply(dtype, g, a, a, h, head0, *drop, st));
  return graphop_vector_spmm_forward(dtype, row, indptr, eid, indices, a, V, o, n_chunks, n_edges, n_k,
                                     n_q, h, d, pm, stream);
}

// din == nullptr: graphop_attention_backward, else its dropout form (p == 0: the undropped op), as `fn`;
// bias != nullptr: the form with a per-edge score bias
int attn_backward(const char* fn, int dtype, const int64_t* row, const int64_t* indptr_r,
                  const int64_t* eid_r, const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                  const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K, const void* V,
                  const void* o, const void* stats, const void* dO, void* dQ, void* dK, void* dV,
                  int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                  int64_t d, void* workspace, int64_t workspace_bytes, const DropIn* din,
                  const graphop_plan_t* plan_r, const graphop_plan_t* plan_c, void* stream,
                  const BiasIn* bias = nullptr) {
  AttnCall c;
  GO_TRY(attn_open(fn, dtype, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d, din, bias, stream, &c));
  const HostDrop* drop = c.drop;
  const int64_t head0 = c.head0;
  hipStream_t st = c.st;
  const size_t es = esize(dtype);
  const Csr gr(row, indptr_r, eid_r, indices_r, n_row_chunks, n_edges, plan_r, "row", "indptr_r", "eid_r", "indices_r");
  const Csr gc(col, indptr_c, eid_c, indices_c, n_col_chunks, n_edges, plan_c, "col", "indptr_c", "eid_c", "indices_c");
  const graphop_plan *pr = gr.plan, *pc = gc.plan;
  AttnFast af;
  AttnBwd form;
  GO_TRY(attn_backward_form(bias != nullptr, /*dry_run=*/false, dtype, h, d, n_edges, n_q, n_k, pr, pc, st, &af, &form));
  const float* b = bias ? (const float*)bias->b : nullptr;
  float* db = bias ? (float*)bias->db : nullptr;
  if (form != AttnBwd::Composed) {
    const i64 F = h * d;
    FastWs ws((char*)workspace, n_q, n_k, F);   // (the one-head forms; attn_heads_backward lays out its own)
    GO_TRY(attn_ws_check(fn, c.ws_fn, true, form == AttnBwd::Heads ? attn_heads_bwd_workspace(n_q, n_k, h, d) : ws.total,
                         workspace, workspace_bytes));
    GO_PTR(fn, Q); GO_PTR(fn, K); GO_PTR(fn, V); GO_PTR(fn, o); GO_PTR(fn, stats); GO_PTR(fn, dO);
    GO_PTR(fn, dQ); GO_PTR(fn, dK); GO_PTR(fn, dV);
    if (form == AttnBwd::Heads)
      return attn_heads_backward(gr, gc, n_q, n_k, h, d, Q,
                                 K, V, b, o, stats, dO, dQ, dK, dV, db, workspace, st, drop, head0);
    GO_HIP(zero_async(dQ, sizeof(float) * (size_t)(n_q * F), st));
    GO_HIP(zero_async(dK, sizeof(float) * (size_t)(n_k * F), st));
    GO_HIP(zero_async(dV, sizeof(float) * (size_t)(n_k * F), st));
    {
      ProfScope prof("attn_pack", st, "k_attn_pack");
      GO_DISPATCH_LNV((int)F, {
        constexpr int RPB = kFastBlock / L;
        hipLaunchKernelGGL((k_attn_pack<L, NV, false>), dim3((unsigned)ceil_div(n_k, RPB)), dim3(kFastBlock),
                           0, st, (const float*)K, (const float*)V, ws.kv, n_k, (const float*)nullptr,
                           (const float*)nullptr, (float4*)nullptr);
        hipLaunchKernelGGL((k_attn_pack<L, NV, true>), dim3((unsigned)ceil_div(n_q, RPB)), dim3(kFastBlock),
                           0, st, (const float*)Q, (const float*)dO, ws.qdo, n_q, (const float*)o,
                           (const float*)stats, ws.st4);
      });
      GO_LAUNCH_CHECK();
    }
    // each launch is written once: DROP and BIAS pick the instantiation, the arguments are the same
    GO_DISPATCH_BOOL(drop != nullptr, DROP, {
      if (form == AttnBwd::Windows) {
        GO_TRY((launch_attn_pass<false, DROP>("attn_bwd_row", af.r, (int)F, n_k, ws.qdo, ws.kv, ws.st4, (float*)dQ,
                                              nullptr, c.hdp, st)));
        GO_TRY((launch_attn_pass<true, DROP>("attn_bwd_col", af.c, (int)F, n_q, ws.kv, ws.qdo, ws.st4, (float*)dK,
                                             (float*)dV, c.hdp, st)));
        return GRAPHOP_OK;
      }
      GO_DISPATCH_BOOL(bias != nullptr, BIAS, {
        GO_TRY((launch_attn_rows<false, DROP, BIAS>(BIAS ? "attn_bias_rows_row" : "attn_rows_row", gr, (int)F, ws.qdo,
                                                    ws.kv, ws.st4, b, (float*)dQ, nullptr, db, c.hdp, st)));
        GO_TRY((launch_attn_rows<true, DROP, BIAS>(BIAS ? "attn_bias_rows_col" : "attn_rows_col", gc, (int)F, ws.kv,
                                                   ws.qdo, ws.st4, b, (float*)dK, (float*)dV, nullptr, c.hdp, st)));
      });
    });
    return GRAPHOP_OK;
  }
  // composition of the unfused entry points: recompute s and a, then the three backward ops
  // with a bias and db given, the softmax backward writes ds straight into db: one E-sized array fewer
  const i64 soft_rows = soft_rows_of(pr, n_q);
  const bool ds_is_db = bias && bias->db != nullptr;
  SlowWs ws((char*)workspace, (bias || drop ? 5 : 4) - (ds_is_db ? 1 : 0), es, n_edges, h, soft_rows);
  GO_TRY(attn_ws_check(fn, c.ws_fn, n_edges * h != 0, ws.total, workspace, workspace_bytes));
  void* s = ws.arr[0];
  void* a = ws.arr[1];
  void* da = ws.arr[2];
  void* ds = ds_is_db ? bias->db : ws.arr[3];
  void* am = ds_is_db ? ws.arr[3] : ws.arr[4];   // a * m of the dropout form
  GO_TRY(graphop_maskedmm_csr_forward(dtype, row, indptr_r, eid_r, indices_r, Q, K, s, n_row_chunks,
                                      n_edges, n_q, n_k, h, d, pr, stream));
  if (bias) GO_TRY(attn_bias_add(dtype, s, bias->b, n_edges * h, st));
  GO_TRY(graphop_sparse_softmax_forward(dtype, row, indptr_r, eid_r, s, a, n_row_chunks, n_edges, h,
                                        soft_rows ? ws.soft : nullptr, soft_rows, pr, stream));
  // with dropout: am = a * m feeds the SpMM backward, and the gradient that comes back is that of am: da = d_am * m
  const void* w = a;
  if (drop) {
    GO_TRY(attn_drop_apply(dtype, gr, a, am, h, head0, *drop, st));
    w = am;
  }
  GO_TRY(graphop_vector_spmm_backward(dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                      indices_c, w, dO, V, da, dV, n_row_chunks, n_col_chunks, n_edges,
                                      n_k, n_q, h, d, pr, pc, stream));
  if (drop) GO_TRY(attn_drop_apply(dtype, gr, da, da, h, head0, *drop, st));
  GO_TRY(graphop_sparse_softmax_backward(dtype, row, indptr_r, eid_r, a, da, ds, n_row_chunks, n_edges, h,
                                         soft_rows ? ws.soft : nullptr, soft_rows, pr, stream));
  return graphop_maskedmm_csr_backward(dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                                       indices_c, Q, K, ds, dQ, dK, n_row_chunks, n_col_chunks, n_edges,
                                       n_q, n_k, h, d, pr, pc, stream);
}

}  // namespace

extern "C" {

int graphop_attention_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q,
                                      int64_t n_k, int64_t h, int64_t d,
                                      const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                      void* stream, int64_t* bytes_out) {
  return attn_workspace_bytes("attention_workspace_bytes", dtype, backward, n_edges, n_q, n_k, h, d, plan_r, plan_c,
                              stream, 4, bytes_out);
}

int graphop_attention_dropout_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k,
                                              int64_t h, int64_t d, const graphop_plan_t* plan_r,
                                              const graphop_plan_t* plan_c, void* stream, int64_t* bytes_out) {
  return attn_workspace_bytes("attention_dropout_workspace_bytes", dtype, backward, n_edges, n_q, n_k, h, d, plan_r,
                              plan_c, stream, 5, bytes_out);
}

int graphop_attention_backward_is_fused(int dtype, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                        int64_t d, const graphop_plan_t* plan_r,
                                        const graphop_plan_t* plan_c, void* stream, int* fused_out) {
  GO_CHECK_ARG(fused_out != nullptr, "attention_backward_is_fused: fused_out is NULL");
  AttnFast af;
  AttnBwd form;
  GO_TRY(attn_backward_form(/*biased=*/false, /*dry_run=*/true, dtype, h, d, n_edges, n_q, n_k, plan_r, plan_c,
                            (hipStream_t)stream, &af, &form));
  *fused_out = form != AttnBwd::Composed ? 1 : 0;
  return GRAPHOP_OK;
}

int graphop_attention_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                              const int64_t* indices, const void* Q, const void* K, const void* V,
                              void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q,
                              int64_t n_k, int64_t h, int64_t d, void* workspace,
                              int64_t workspace_bytes, const graphop_plan_t* plan, void* stream) {
  return attn_forward("attention_forward", dtype, row, indptr, eid, indices, Q, K, V, o, stats, n_chunks, n_edges, n_q,
                      n_k, h, d, workspace, workspace_bytes, nullptr, plan, stream);
}

int graphop_attention_backward(int dtype, const int64_t* row, const int64_t* indptr_r,
                               const int64_t* eid_r, const int64_t* indices_r, const int64_t* col,
                               const int64_t* indptr_c, const int64_t* eid_c, const int64_t* indices_c,
                               const void* Q, const void* K, const void* V, const void* o,
                               const void* stats, const void* dO, void* dQ, void* dK, void* dV,
                               int64_t n_row_chunks, int64_t n_col_chunks, int64_t n_edges,
                               int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                               int64_t workspace_bytes, const graphop_plan_t* plan_r,
                               const graphop_plan_t* plan_c, void* stream) {
  return attn_backward("attention_backward", dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c, indices_c,
                       Q, K, V, o, stats, dO, dQ, dK, dV, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d, workspace,
                       workspace_bytes, nullptr, plan_r, plan_c, stream);
}

// p == 0 is the entry point above: the same kernels, bit-identical results
int graphop_attention_dropout_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                      const int64_t* indices, const void* Q, const void* K, const void* V, void* o,
                                      void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                                      int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                      const graphop_plan_t* plan, void* stream, double p, uint64_t seed,
                                      uint32_t offset, int64_t head0) {
  const DropIn din{p, seed, offset, head0};
  return attn_forward("attention_dropout_forward", dtype, row, indptr, eid, indices, Q, K, V, o, stats, n_chunks,
                      n_edges, n_q, n_k, h, d, workspace, workspace_bytes, &din, plan, stream);
}

int graphop_attention_dropout_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                       const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                       const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                       const void* V, const void* o, const void* stats, const void* dO, void* dQ,
                                       void* dK, void* dV, int64_t n_row_chunks, int64_t n_col_chunks,
                                       int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d,
                                       void* workspace, int64_t workspace_bytes, const graphop_plan_t* plan_r,
                                       const graphop_plan_t* plan_c, void* stream, double p, uint64_t seed,
                                       uint32_t offset, int64_t head0) {
  const DropIn din{p, seed, offset, head0};
  return attn_backward("attention_dropout_backward", dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                       indices_c, Q, K, V, o, stats, dO, dQ, dK, dV, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d,
                       workspace, workspace_bytes, &din, plan_r, plan_c, stream);
}

// b == NULL is not an error only for empty problems; p == 0 takes no Philox path
int graphop_attention_bias_workspace_bytes(int dtype, int backward, int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h,
                                           int64_t d, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                           void* stream, int with_db, int64_t* bytes_out) {
  return attn_workspace_bytes("attention_bias_workspace_bytes", dtype, backward, n_edges, n_q, n_k, h, d, plan_r, plan_c,
                              stream, with_db ? 4 : 5, bytes_out, /*bias=*/true);
}

int graphop_attention_bias_forward(int dtype, const int64_t* row, const int64_t* indptr, const int64_t* eid,
                                   const int64_t* indices, const void* Q, const void* K, const void* V, const void* b,
                                   void* o, void* stats, int64_t n_chunks, int64_t n_edges, int64_t n_q, int64_t n_k,
                                   int64_t h, int64_t d, void* workspace, int64_t workspace_bytes,
                                   const graphop_plan_t* plan, void* stream, double p, uint64_t seed, uint32_t offset,
                                   int64_t head0) {
  const DropIn din{p, seed, offset, head0};
  const BiasIn bin{b, nullptr};
  return attn_forward("attention_bias_forward", dtype, row, indptr, eid, indices, Q, K, V, o, stats, n_chunks, n_edges,
                      n_q, n_k, h, d, workspace, workspace_bytes, &din, plan, stream, &bin);
}

int graphop_attention_bias_backward(int dtype, const int64_t* row, const int64_t* indptr_r, const int64_t* eid_r,
                                    const int64_t* indices_r, const int64_t* col, const int64_t* indptr_c,
                                    const int64_t* eid_c, const int64_t* indices_c, const void* Q, const void* K,
                                    const void* V, const void* b, const void* o, const void* stats, const void* dO,
                                    void* dQ, void* dK, void* dV, void* db, int64_t n_row_chunks, int64_t n_col_chunks,
                                    int64_t n_edges, int64_t n_q, int64_t n_k, int64_t h, int64_t d, void* workspace,
                                    int64_t workspace_bytes, const graphop_plan_t* plan_r, const graphop_plan_t* plan_c,
                                    void* stream, double p, uint64_t seed, uint32_t offset, int64_t head0) {
  const DropIn din{p, seed, offset, head0};
  const BiasIn bin{b, db};
  return attn_backward("attention_bias_backward", dtype, row, indptr_r, eid_r, indices_r, col, indptr_c, eid_c,
                       indices_c, Q, K, V, o, stats, dO, dQ, dK, dV, n_row_chunks, n_col_chunks, n_edges, n_q, n_k, h, d,
                       workspace, workspace_bytes, &din, plan_r, plan_c, stream, &bin);
}

}  // extern "C"
