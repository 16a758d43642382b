// Host-side helpers shared by the translation units of libgraphop_hip (graphop_hip.hip defines
// them; attention.hip uses them).  Not part of the C ABI.  What exists once, here: the tuning knobs, the chunk-driver
// geometry, and Csr -- a chunked CSR orientation with its plan resolved (the two plan matches, the coverage rule, the
// bounds check, the NULL checks of the four arrays) -- with the 16-byte alignment test.
#pragma once
#include "common.h"

namespace graphop {

// brackets one kernel launch with two hipEvents when profiling is enabled (graphop_profile_enable)
struct ProfScope {
  hipEvent_t t0 = nullptr, t1 = nullptr;
  hipStream_t st;
  const char* name;
  const char* kernel;   // device kernel family (string literal), may be set after construction
  ProfScope(const char* n, hipStream_t s, const char* k = "");
  ~ProfScope();
};

struct Tuning {
  int sddmm_cpg;  // chunks per lane-group, SDDMM-type kernels
  int spmm_cpg;   // chunks per lane-group, SpMM-type kernels
  int force_generic;
  int sweep;            // use the window-sweep drivers when a plan allows it
  int window_kb;        // target bytes of gathered table per window (must sit in a 4 MiB L2)
  int mall_window_kb;   // window size for tables beyond the Infinity Cache
  int max_windows;
  int sweep_min_kb;     // tables smaller than this are L2-friendly enough for the chunk drivers
  int sweep_bpc;        // resident blocks per CU for the sweep drivers (3: with staged ids 2 % faster than the 4 the kernels are compiled for)
  int sweep_k;          // vrows per lane group (0 = auto)
  int vrow_t;           // vrow length cap (0 = auto from the mean row length)
  int sweep_min_granule;  // mean slots per (row, window) below which the sweep is not worth it
  int dense_blocks;       // use the fp32-MFMA block-dense drivers when the plan found a cover
  int dense_min_fill;     // ... whose 32x32 tiles hold at least this many percent edges
  int dense_detect_min_fill;  // plan creation keeps a block cover only above this fill (percent)
  int sweep_w;            // > 0: number of column windows (overrides window_kb)
  int spmm_window_scale;  // window-owner SpMM over identity-eid slots: windows this many times window_kb
  int attn_fused;         // attention_forward/backward: use the fused window kernels when they apply
  int attn_window_scale;  // fused kernels gather 2 packed rows per slot: windows of this many times window_kb
  int attn_k;             // vrows per lane group in the fused kernels (0 = auto)
  int attn_bpc;           // resident workgroups per CU of the fused kernels
  int staged_ids;         // window-owner passes: plan-time deal + contiguous ids staged through LDS (IdStage);
                          // bit 0: SDDMM, bit 1: SpMM (both orientations), bit 2: the fused backward passes
  int attn_fwd_walk;      // attention_forward as ONE walk-style pass (kernels_attn_walk.h) where it applies (fp32, h = 1, d = 64)
  int spmm_selfzero;      // SpMM-type passes on the chunk driver with row ownership leave their output fully defined
                          // themselves (no zero fill by the entry point) ...
  int spmm_selfzero_min_mb;  // ... for outputs of at least this many MB (below, the fill is noise)
  int spmm_flat;          // row-owning chunk driver in its slot-walking form (k_spmm_flat_f32) where chunks are short ...
  int spmm_flat_max_mean; // ... i.e. below this many slots per chunk on average
  int spmm_flat_cpg;      // chunks per lane group of that form (more than spmm_cpg: a group should see several id batches)
  int spmm_flat_min_chunks;  // ... and only for chunk lists at least this long
  int attn_max_d;         // widest row (floats) the fused window passes are chosen for: beyond 64 the two-row gathers
                          // dominate and the passes measure slower than the unfused ones (d=128: 18.9 vs 16.8 ms)
  int attn_rows;          // chunk-driver fused backward: -1 = by the cost rule, 0 = never, 1 = whenever legal
  int attn_heads;         // several-head fused forms (kernels_attn_heads.h): -1 = by the cost rule, 0 = never (head groups /
                          // the composed path as before), 1 = wherever the conditions allow
  int touch_sddmm;        // SDDMM strips: per-task id-line touches (kernels_fast.h: LineTouch): bit 0 ids, bit 1 edge ids
  int walk;               // walk drivers (kernels_walk.h): bit 1 SpMM-type passes over identity-eid (row-major) slots,
                          // bit 2 SpMM-type over permuted (column-major) slots (bit 0 was the SDDMM-type walk kernel of
                          // round 3: 1.63-1.73 ms against 1.51 on the window-owner strips, removed in round 4)
  int walk_window_kb;     // bytes of gathered table per window of the walk drivers, passes over identity-eid (row-major) slots
  int walk_window_kb_col; // ... passes over permuted (column-major) slots: their per-slot scalars are a gather whose lines
                          // share the L2 with the window (Reddit shape: 2.72 ms at 4 MB, 2.25 at 2 MB; row-major 1.71 / 1.78)
  int walk_drift;         // pacing steps a wave may run ahead of the slowest wave of its XCD (0 = free-running)
  int walk_steps;         // pacing steps per column window
  int walk_min_bin;       // fewest slots per (lane group, round) bin for the walk drivers to be chosen
  int walk_debug;         // 1: every walk launch is followed by a synchronisation and a line of pacing statistics on stderr
  int walk_fault;         // tests only: inject a hand-over fault into the walk kernel (kernels_walk.h: WalkView::fault)
  int walk_blocks;        // > 0: workgroups of the walk launches (tests: a small grid makes several rounds of sizeable bins)
  int sddmm_tile;         // SDDMM-type passes on the tile driver (kernels_tile.h): 0 never, 1 where the plan's repeat fraction pays
                          // (sddmm_tile_min_repeat), 2 wherever the shape is in scope
  int sddmm_tile_rows;    // vrows per tile: 128, 192 (two workgroups of 512 threads per CU; 192 measured best), 256 or 384 (one of 1024)
  int sddmm_tile_min_repeat;  // percent of a plan's slots that repeat a neighbour of their tile from which the tile driver is chosen
  int sddmm_tile_touch;   // 1: a wave touches the next task's record lines (kernels_tile.h: TileView::touch)
  int plan_trim;          // 1: plans drop what only their layout builders read (32-bit mirrors, window tables) once an op has what
                          // it launches with; rebuilt on demand (plan.hip: plan_trim)
  int n_cu;
  Tuning() {
    sweep = env_int("GRAPHOP_SWEEP", 1);
    window_kb = env_int("GRAPHOP_WINDOW_KB", 4096);
    mall_window_kb = env_int("GRAPHOP_MALL_WINDOW_KB", 32768);
    max_windows = env_int("GRAPHOP_MAX_WINDOWS", 128);
    sweep_min_kb = env_int("GRAPHOP_SWEEP_MIN_KB", 4608);
    sweep_bpc = env_int("GRAPHOP_SWEEP_BPC", 3);
    sweep_k = env_int("GRAPHOP_SWEEP_K", 0);
    vrow_t = env_int("GRAPHOP_VROW_T", 0);
    sweep_min_granule = env_int("GRAPHOP_SWEEP_MIN_GRANULE", 4);
    sweep_w = env_int("GRAPHOP_SWEEP_W", 0);
    spmm_window_scale = env_int("GRAPHOP_SPMM_WINDOW_SCALE", 2);
    dense_blocks = env_int("GRAPHOP_DENSE_BLOCKS", 1);
    dense_min_fill = env_int("GRAPHOP_DENSE_MIN_FILL", 40);
    dense_detect_min_fill = env_int("GRAPHOP_DENSE_DETECT_MIN_FILL", 10);
    attn_fused = env_int("GRAPHOP_ATTN_FUSED", 1);
    attn_fwd_walk = env_int("GRAPHOP_ATTN_FWD_WALK", 1);
    spmm_selfzero = env_int("GRAPHOP_SPMM_SELFZERO", 1);
    spmm_selfzero_min_mb = env_int("GRAPHOP_SPMM_SELFZERO_MIN_MB", 256);
    spmm_flat = env_int("GRAPHOP_SPMM_FLAT", 1);
    spmm_flat_max_mean = env_int("GRAPHOP_SPMM_FLAT_MAX_MEAN", 10);
    spmm_flat_cpg = env_int("GRAPHOP_SPMM_FLAT_CPG", 32);
    if (spmm_flat_cpg < 1) spmm_flat_cpg = 1;
    spmm_flat_min_chunks = env_int("GRAPHOP_SPMM_FLAT_MIN_CHUNKS", 1 << 20);
    attn_window_scale = env_int("GRAPHOP_ATTN_WINDOW_SCALE", 2);
    attn_k = env_int("GRAPHOP_ATTN_K", 0);
    attn_bpc = env_int("GRAPHOP_ATTN_BPC", 0);
    attn_rows = env_int("GRAPHOP_ATTN_ROWS", -1);
    attn_heads = env_int("GRAPHOP_ATTN_HEADS", -1);
    attn_max_d = env_int("GRAPHOP_ATTN_MAX_D", 64);
    staged_ids = env_int("GRAPHOP_STAGED_IDS", 7);
    touch_sddmm = env_int("GRAPHOP_TOUCH_SDDMM", 1);
    walk = env_int("GRAPHOP_WALK", 6);
    walk_window_kb = env_int("GRAPHOP_WALK_WINDOW_KB", 4096);
    walk_window_kb_col = env_int("GRAPHOP_WALK_WINDOW_KB_COL", 2048);
    walk_drift = env_int("GRAPHOP_WALK_DRIFT", 3);
    walk_steps = env_int("GRAPHOP_WALK_STEPS", 2);
    walk_min_bin = env_int("GRAPHOP_WALK_MIN_BIN", 1024);
    walk_blocks = env_int("GRAPHOP_WALK_BLOCKS", 0);
    walk_debug = env_int("GRAPHOP_WALK_DEBUG", 0);
    walk_fault = 0;
    sddmm_tile = env_int("GRAPHOP_SDDMM_TILE", 1);
    sddmm_tile_rows = env_int("GRAPHOP_SDDMM_TILE_ROWS", 192);
    sddmm_tile_min_repeat = env_int("GRAPHOP_SDDMM_TILE_MIN_REPEAT", 20);
    sddmm_tile_touch = env_int("GRAPHOP_SDDMM_TILE_TOUCH", 1);
    plan_trim = env_int("GRAPHOP_PLAN_TRIM", 1);
    n_cu = 256;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
        prop.multiProcessorCount > 0)
      n_cu = prop.multiProcessorCount;
    sddmm_cpg = env_int("GRAPHOP_SDDMM_CPG", 8);
    spmm_cpg = env_int("GRAPHOP_SPMM_CPG", 16);
    force_generic = env_int("GRAPHOP_FORCE_GENERIC", 0);
    if (sddmm_cpg < 1) sddmm_cpg = 1;
    if (spmm_cpg < 1) spmm_cpg = 1;
  }
};
Tuning& tuning_mut();
const Tuning& tuning();

// Stream-ordered zero fill (a kernel: runtime.hip, k_zero16).
hipError_t zero_async(void* ptr, size_t bytes, hipStream_t st);

struct SweepView;   // kernels_fast.h
}  // namespace graphop

#include "kernels_fast.h"

namespace graphop {

// Chunks per lane group of a chunk-driver pass whose lane groups have `lanes` lanes: the cap (a tuned value or a
// kernel's own) amortises row switches on big graphs, but a small graph must still put `rounds` rounds of resident lane
// groups on every CU -- Cora-shape, 2.8 K chunks: 16 chunks per group left 13 workgroups walking chunks serially (33 us
// per pass).  Every launch of such a pass and every workspace size that follows from one takes the value from here.
inline i64 chunks_per_group(i64 n_chunks, int lanes, i64 cap, int rounds = 8) {
  const i64 groups_wanted = (i64)tuning().n_cu * (kFastBlock / lanes) * rounds;
  const i64 c = n_chunks / (groups_wanted > 0 ? groups_wanted : 1);
  return c < 1 ? 1 : (c < cap ? c : cap);
}

// ... with the lane groups and the workgroups of kFastBlock threads that follow from it
struct ChunkGeometry {
  i64 cpg, groups;
  unsigned blocks;
  int lanes;
};
inline ChunkGeometry chunk_geometry(i64 n_chunks, int lanes, i64 cap, int rounds = 8) {
  const i64 cpg = chunks_per_group(n_chunks, lanes, cap, rounds), groups = ceil_div(n_chunks, cpg);
  return {cpg, groups, (unsigned)ceil_div(groups, (i64)(kFastBlock / lanes)), lanes};
}

struct SweepLaunch {
  const Sweep* sweep = nullptr;   // the window structure the view was filled from
  SweepView view;
  unsigned blocks;
  size_t lds_bytes;
};

// Overrides for kernels whose gathered rows / per-vrow LDS rows are not one F-float row
// (the fused attention kernels gather two packed rows per slot).
struct SweepOpts {
  i64 row_bytes = 0;      // bytes per gathered table row (0 = 16*L*NV)
  int K = 0;              // vrows per lane group (0 = auto)
  int window_scale = 0;   // > 0: windows of this many times window_kb, vrows as many times longer
  int bpc = 0;            // resident workgroups per CU (0 = tuning().sweep_bpc)
  int dry_run = 0;        // 1: decide and build the cached structure only (no task queue is taken)
  int touch = 0;          // SweepView::touch of the launch
  int staged = 0;         // 1: also fetch / build the dealt (window-major) layout and put it in the view
  int stage_lds_per_group = 0;   // bytes of LDS each lane group needs for staging (added to lds_bytes)
  int tile = 0;           // 1: the caller reads a tile layout (kernels_tile.h): neither a dealt layout nor the window tables at run time
  int no_eids = 0;        // 1: the kernels never read edge ids (fused attention passes): the dealt layout keeps no copy of them
};

// Decide whether the window-sweep driver applies and fetch / build its structure.
// Returns 1 = use sweep, 0 = use the chunk driver, <0 = error code (negated).
int choose_sweep(const graphop_plan* plan, i64 n_table_rows, int L, int NV, hipStream_t st,
                 SweepLaunch* out, bool accumulating = false, const SweepOpts* opts = nullptr);

// plan.hip (setup kernels and the plan's cached structures)
int partition_count(const i64*, i64, i64, i64*, hipStream_t);
int partition_fill(const i64*, const i64*, i64, i64, i64, i64*, i64*, hipStream_t);
int plan_build(graphop_plan*, i64, hipStream_t, int);
int plan_get_sweep(graphop_plan*, int, i64, int, hipStream_t, const Sweep**);
int* plan_take_queue(graphop_plan*, const Sweep*);
int plan_get_dealt(graphop_plan*, const Sweep*, int, int, hipStream_t, const Sweep::Dealt**, bool want_eids = true);
int plan_get_tile(graphop_plan*, const Sweep*, int R, int cap, bool force, int min_repeat_pct, hipStream_t, const Sweep::Tile**);
void plan_free_sweeps(graphop_plan*);
int plan_get_walk(graphop_plan*, int, i64, int, int, int, int, hipStream_t, const Walk**, bool want_widx = true);
int plan_build_seg_eptr(graphop_plan*, hipStream_t);
int* plan_take_walk_sync(graphop_plan*, const Walk*);
int plan_n_sweeps(const graphop_plan* p);
const Sweep* plan_sweep_at(const graphop_plan* p, int i);
int plan_import_arrays(graphop_plan* p, const i64* seg_chunk, const int32_t* idx32, const int32_t* eid32,
                       const int32_t* long_segs, i64 n_long, const int32_t* blk_seg,
                       const int32_t* seg_e0, const int32_t* seg_row, hipStream_t st);
int plan_import_sweep(graphop_plan* p, int W, i64 win_cols, int T, int V, const int32_t* vr_row,
                      const int32_t* wp_lo, const int32_t* wp_hi, hipStream_t st);
void plan_init_sweeps(graphop_plan*);
int plan_ensure_mirrors(graphop_plan* p, hipStream_t st);
int plan_pin_mirrors(graphop_plan* p, hipStream_t st);
int plan_ensure_mirrors_locked(graphop_plan* p, hipStream_t st);
int plan_rebuild_sweep_tables(graphop_plan* p, const Sweep* sw, hipStream_t st);
int plan_pin_sweep_tables(graphop_plan* p, const Sweep* sw, hipStream_t st);
void plan_trim(graphop_plan* p);
// the fused attention passes' window structure for ONE orientation (attention.hip); dry run
int attn_prepare_plan(const graphop_plan* plan, i64 n_table_rows, i64 d, bool col, hipStream_t st);

// Fused attention forward on the walk (graphop_hip.hip; kernels_attn_walk.h): 1 = launched, 0 = does not apply,
// < 0 = error (negated).  dry_run: only decide / build the layout and report the workspace it needs.
// drop: the attention dropout of the call's head (kernels_attn.h), NULL = none; it changes neither the decision nor
// the workspace.
struct AttnDrop;
int attn_fwd_walk(const graphop_plan* plan, i64 n_q, i64 n_k, i64 h, i64 d, int dtype, const void* Q, const void* K,
                  const void* V, void* o, void* stats, void* ws, i64 ws_bytes, hipStream_t st, bool dry_run,
                  size_t* ws_needed, const AttnDrop* drop = nullptr);

// Fused attention forward WITH a per-edge score bias b (indexed by edge id), chunk-driver form (graphop_hip.hip;
// kernels_attn_bias.h): a lane group walks consecutive chunks of a rows_sorted plan with an online
// softmax; rows that groups share leave as piece records merged by the walk's piece kernels.  Same return values and
// dry_run meaning as attn_fwd_walk.  g: the call's row-major orientation (0 where g.plan is NULL).
struct Csr;
int attn_bias_fwd_rows(const Csr& g, i64 n_q, i64 n_k, i64 h, i64 d, int dtype, const void* Q, const void* K,
                       const void* V, const void* b, void* o, void* stats, void* ws, i64 ws_bytes, hipStream_t st,
                       bool dry_run, size_t* ws_needed, const AttnDrop* drop = nullptr);

// Several-head forms of the fused attention passes (attention_heads.hip; kernels_attn_heads.h): fp32,
// (h, d) a several-head pair of GO_DISPATCH_GAT_HD, plans with neighbour ids whose id ranges lie inside the tables.
// attn_heads_fwd_rows: attn_bias_fwd_rows' contract (return values, dry_run, workspace) for h > 1; b == NULL: no bias.
// attn_heads_bwd_ok: will attn_heads_backward run for this call?  Its workspace is attn_heads_bwd_workspace bytes.
struct HostDrop;   // host_dropout.h; drop == NULL: no dropout, else the call's heads are the global heads head0 .. head0 + h - 1
int attn_heads_fwd_rows(const Csr& g, i64 n_q, i64 n_k, i64 h, i64 d, int dtype, const void* Q, const void* K,
                        const void* V, const void* b, void* o, void* stats, void* ws, i64 ws_bytes, hipStream_t st,
                        bool dry_run, size_t* ws_needed, const HostDrop* drop = nullptr, i64 head0 = 0);
bool attn_heads_bwd_ok(int dtype, i64 h, i64 d, i64 n_edges, i64 n_q, i64 n_k, const graphop_plan* plan_r,
                       const graphop_plan* plan_c, hipStream_t st);
size_t attn_heads_bwd_workspace(i64 n_q, i64 n_k, i64 h, i64 d);
int attn_heads_backward(const Csr& r, const Csr& c, i64 n_q, i64 n_k, i64 h, i64 d, const void* Q, const void* K,
                        const void* V, const void* b, const void* o, const void* stats, const void* dO, void* dQ, void* dK,
                        void* dV, void* db, void* ws, hipStream_t st, const HostDrop* drop, i64 head0);

inline size_t esize(int dtype) { return dtype == GRAPHOP_F64 ? 8 : 4; }
inline bool pow2(i64 v) { return v > 0 && (v & (v - 1)) == 0; }
inline i64 pow2ceil(i64 v) { i64 p = 1; while (p < v) p <<= 1; return p; }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One chunked CSR orientation as an entry point receives it, with the caller's plan resolved against it.  Built once
// per orientation where the C ABI's arguments arrive (the only place the ABI's int64_t* become the kernels' i64*) and
// passed down by const reference.  Holds no memory and caches nothing but the two answers to "is this plan the plan of
// these arrays?":
//   plan        the caller's plan if it was made from row, indptr, eid, indices and both counts, else NULL
//   plan_slots  ... from row, indptr, eid and both counts: what is true of the slots' rows and edge ids whatever the
//               neighbour ids are (which edge-sized outputs are written in full; softmax and node_mul_edge, which have
//               no neighbour ids)
struct Csr {
  const i64 *row, *indptr, *eid, *indices;
  i64 n_chunks, n_edges;
  const graphop_plan *plan, *plan_slots;
  const char* names[4];   // of the four arrays in the entry point's signature, for require()

  Csr(const int64_t* row_, const int64_t* indptr_, const int64_t* eid_, const int64_t* indices_, i64 C, i64 E,
      const graphop_plan* p, const char* row_name = "row", const char* indptr_name = "indptr",
      const char* eid_name = "eid", const char* indices_name = "indices")
      : row((const i64*)row_), indptr((const i64*)indptr_), eid((const i64*)eid_), indices((const i64*)indices_),
        n_chunks(C), n_edges(E), names{row_name, indptr_name, eid_name, indices_name} {
    plan_slots = (p && p->row == row_ && p->indptr == indptr_ && p->eid == eid_ && p->info.n_chunks == C &&
                  p->info.n_edges == E) ? p : nullptr;
    plan = (plan_slots && p->indices == indices_) ? p : nullptr;
  }

  // every edge id is written by a pass over the slots: an edge-sized output needs no zero fill.  covered(true) asks
  // plan_slots and is what the core ops use (graphop_hip.hip); covered() asks plan and is what the GAT family uses
  bool covered(bool slots = false) const {
    const graphop_plan* p = slots ? plan_slots : plan;
    return p && p->info.full_coverage && p->info.eid_identity && p->info.indptr_monotone;
  }
  // a row's chunks are adjacent: rows inside one lane group's range need no atomics
  bool owned() const { return plan && plan->info.rows_sorted; }
  // the eid argument of a fast pass over `plan`: NULL where the plan says eid[slot] == slot
  const i64* eid_or_null() const { return plan->info.eid_identity ? nullptr : eid; }

  // the arrays the signature names, in its order; has_indices = false: an op without neighbour ids
  int require(const char* fn, bool has_indices = true) const {
    const void* ps[4] = {row, indptr, eid, indices};
    for (int i = 0; i < (has_indices ? 4 : 3); ++i)
      GO_CHECK_ARG(ps[i] != nullptr, "%s: %s is NULL", fn, names[i]);
    return GRAPHOP_OK;
  }
  // Row ids address the row-side operand / output, neighbour ids the gathered one: with a plan (p: plan or plan_slots,
  // NULL: no check) the largest of each is known, so an operand with too few rows is an error here instead of an
  // out-of-bounds access on the device.  idx_name == NULL: row ids only.
  static int check_bounds(const char* fn, const graphop_plan* p, const char* seg_name, i64 n_seg, const char* idx_name,
                          i64 n_idx) {
    if (!p) return GRAPHOP_OK;
    GO_CHECK_ARG(p->info.max_row < n_seg, "%s: row id %lld but %s has only %lld rows", fn, (long long)p->info.max_row,
                 seg_name, (long long)n_seg);
    GO_CHECK_ARG(!idx_name || p->info.max_index < n_idx, "%s: neighbour id %lld but %s has only %lld rows", fn,
                 (long long)p->info.max_index, idx_name, (long long)n_idx);
    return GRAPHOP_OK;
  }
};

#define GO_DISPATCH_LNV(F, ...)                                      \
  switch (F) {                                                       \
    case 16: { constexpr int L = 4, NV = 1; __VA_ARGS__; } break;    \
    case 32: { constexpr int L = 8, NV = 1; __VA_ARGS__; } break;    \
    case 64: { constexpr int L = 16, NV = 1; __VA_ARGS__; } break;   \
    case 128: { constexpr int L = 32, NV = 1; __VA_ARGS__; } break;  \
    case 256: { constexpr int L = 64, NV = 1; __VA_ARGS__; } break;  \
    case 512: { constexpr int L = 64, NV = 2; __VA_ARGS__; } break;  \
    case 1024: { constexpr int L = 64, NV = 4; __VA_ARGS__; } break; \
    default: break;                                                  \
  }

// sparse_softmax_forward that also leaves the row statistics (max, 1 / sum) behind (stats == NULL: not); graphop_hip.hip
int softmax_forward_stats(int dtype, const Csr& g, const void* x, void* y, i64 h, void* ws, i64 ws_rows, hipStream_t st,
                          void* stats);

#define GO_PTR(fn, p) GO_CHECK_ARG((p) != nullptr, "%s: " #p " is NULL", fn)
#define GO_TRY(expr)                     \
  do {                                   \
    int _rc = (expr);                    \
    if (_rc != GRAPHOP_OK) return _rc;   \
  } while (0)

}  // namespace graphop
